"""-m gpu: every reachable activation-quantiser site pinned to the numpy reference of ggml's rounding, exactly (tests/quant_probe_util.py: selector
weights read back the scale, every quantised value and every block sum of every activation row; tests/test_quant_probe_cpu.py holds the oracle
to the same reference and shows what the probe rejects).

Each test first proves from the plan counters that the graph took the launch form it is about, then asserts the selector rows equal as values and
the heavy Q4_K row inside its bar of roundings. Sites and the counters that show them:
  T = 1 mat-vec, in-kernel prologue (plain / RMS-norm / gate)   kernels_in_last_plan = one per mat-vec, fused_nodes_in_last_plan = the prologue's nodes.
        WHICH mat-vec form ran (direct WS = 1, four-wave staged, eight-wave, the lean variants) is decided inside k_matvec from K, M and the
        residual; no counter tells them apart. The shapes are chosen from that rule: <= 512 tiles of 64 super-blocks direct (Q4_K only),
        513 .. 1535 four waves, >= 1536 eight waves.
  long gate, K = 4352 > 4096       gate_quant_kernel in front of a mat-vec that copies the blocks: two launches per mat-vec
  paired gate                      linear_in writes g = silu(l) r itself, linear_out quantises it plain: two launches for the pair (three unpaired)
  T >= 2 quantised mat-mul         quant_rows / rms_quant_rows / gate_quant_rows (+ the _q80 three) and the MFMA mat-mul are ONE plan step:
        kernels_in_last_plan = 1. Split-K against the rows kernel (M >= 8192) is again decided inside the launch, without a counter.
        Every column also equals the T = 1 launch of the same row.
  general gate values              l in [-8, 8]: expf of the device is within an ulp of the host's, not equal to it, so the exact assertion has no
        reference. assert_probe_tolerant: the block's scale or a neighbour, every element away from a rounding boundary exact.
  BF16 / F16                       T = 1: the float mat-vec (no float mat-mul counted); T >= 2: float_batched_mms_in_last_plan = 1 (f64 MFMA) or,
        with float_accumulate on, float_acc_mms_in_last_plan = 1; cvt_rows / rms_cvt_rows / gate_cvt_rows are part of that one step.

Not reached, and why that is enough:
  heads_streams_kernel   its products pass through a soft_max before anything is stored: expf of the device against expf of the host is not
        exact, so no output is a read-out of the blocks. tests/test_stt_slots_gpu.py holds the launch to the node chain.
  inproj_attn_kernel, the chain engine, the depth_nest and depth_nest80 step programs   their products feed attention or the next phase inside
        the launch. tests/test_chain_engine.py and tests/test_mv_tile_tail_gpu.py hold them bit-identical to the mat-vec launches pinned here, and
        they call the same quantize_block_q8k / quantize_block_q80 on four values per lane assembled by the same expressions.
  norm_quant_kernel (k_norm_quant_q8k) has no caller in the planner (only tests/microbench/chain_bench.hip calls it): no graph reaches it."""
import functools

import numpy as np
import pytest

import float_acc_util as fu
import ggml_util as gu
import quant_probe_util as qp
from ggml_util import Q4_0, Q4_K, Q8_0

f32 = np.float32
WT_IDS = lambda t: qp.NAMES[t]  # noqa: E731


@functools.lru_cache(maxsize=4)
def selectors(wt, K):
    return qp.Selectors(wt, K)


def run(build, T, M, mode=None):
    outs, st = gu.run_graph("hip", build) if mode is None else fu.run_hip(build, mode=mode)
    return qp.collect(outs, T, M), st


def pool(wt, K, T):
    """T rows that go round the families of the weight type: row i is row (i // nf) % 3 of family i % nf (seed i // (3 nf)), so any T >= nf holds every
    family and T >= 3 nf every row of every family - nothing is left to a draw"""
    names = list(qp.families(wt))
    nf = len(names)
    fams = {}
    rows = []
    for i in range(T):
        key = (names[i % nf], i // (3 * nf))
        if key not in fams:
            fams[key] = qp.family(wt, key[0], K, 3, key[1])
        rows.append(fams[key][(i // nf) % 3])
    return np.stack(rows)


def full_set(wt):
    """the row count at which pool() holds all three rows of every family: what each T = 1 site is run on"""
    return 3 * len(qp.families(wt))


def activation(wt, K, T, prologue, seed=0):
    """-> (graph input, alpha, the floats the quantiser sees)"""
    if prologue == "norm":
        x, alpha = qp.norm_inputs(K, T, seed + K + T)
        return x, alpha, qp.norm_values(x, alpha)
    v = pool(wt, K, T)
    if prologue == "gate":
        h, seen = qp.gate_inputs(v, seed + 3)
        return h, None, seen
    return v, None, v


PROLOGUE_NODES = {"plain": 0, "norm": 3, "gate": 3}      # mul_mat + (mul, rms_norm) or (mul, silu): counted as fused only with a prologue or epilogue


# ---- T = 1: the in-kernel prologue of the block mat-vec -----------------------------------------------------------------------------------
# Q4_K 4096 x 4225: 1 057 tiles, 16 rows per workgroup - with a residual the four-wave lean variant (one residual load per thread); 2560 x 4000 holds 26 rows
# per workgroup and stays on the general four-wave kernel; 4096 x 6144 is the eight-wave shape and, with a residual or an RMS norm, its lean variants
MV_SHAPES = [(Q4_K, 256, None), (Q4_K, 1024, None), (Q4_K, 2560, None), (Q4_K, 2560, 4000), (Q4_K, 4096, None), (Q4_K, 4096, 6144),
             (Q8_0, 256, None), (Q8_0, 1024, None), (Q8_0, 2560, None), (Q8_0, 4096, 6144),
             (Q4_0, 256, None), (Q4_0, 1024, None), (Q4_0, 2560, None), (Q4_0, 4096, 6144)]


@pytest.mark.gpu
@pytest.mark.parametrize("residual", [False, True], ids=["", "residual"])
@pytest.mark.parametrize("prologue", ["plain", "norm", "gate"])
@pytest.mark.parametrize("wt,K,M", MV_SHAPES, ids=[f"{qp.NAMES[w]}-{k}-{m or 'sel'}" for w, k, m in MV_SHAPES])
def test_matvec_in_kernel_prologue(wt, K, M, prologue, residual):
    sel = selectors(wt, K)
    M = M or sel.M0
    T = full_set(wt)                                                                   # 18 (Q4_K) / 21 mat-vecs: every row of every family at every shape
    a, alpha, seen = activation(wt, K, T, prologue)
    res = qp.probe_residual(sel, T, M, K) if residual else None
    got, st = run(qp.probe_graph(sel, a, prologue, alpha, res, M, per_row=True), T, M)
    assert st.kernels_in_last_plan == T, st.kernels_in_last_plan                       # one launch per mat-vec: prologue and residual inside
    assert st.fused_nodes_in_last_plan == T * ((PROLOGUE_NODES[prologue] or residual) + residual), st.fused_nodes_in_last_plan
    assert st.chained_matvecs_in_last_plan == 0
    qp.assert_probe(got, qp.reference(wt, seen), f"{qp.NAMES[wt]} K={K} M={M} {prologue} T=1", residual=res)


# ---- long gate: gate_quant_kernel + a mat-vec over pre-quantised blocks ---------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("wt", [Q4_K, Q8_0], ids=WT_IDS)
def test_long_gate_is_quantised_by_its_own_launch(wt):
    K, T = 4352, full_set(wt)
    sel = selectors(wt, K)
    h, _, seen = activation(wt, K, T, "gate")
    got, st = run(qp.probe_graph(sel, h, "gate", per_row=True), T, sel.M0)
    assert st.kernels_in_last_plan == 2 * T, st.kernels_in_last_plan
    qp.assert_probe(got, qp.reference(wt, seen), f"{qp.NAMES[wt]} K={K} long gate")


# ---- paired gate: the producer writes g, linear_out quantises it plain -----------------------------------------------------------------------
@pytest.mark.gpu
def test_paired_gate_hands_linear_out_a_plain_activation():
    # F = 4352 with K = 512 is the smallest pair k_matvec_pair_ok accepts: F > 4096, a multiple of 256, 32 rows of each half per workgroup
    sel = selectors(Q4_K, 4352)
    build, seen = qp.paired_gate_case(sel)
    got, st = run(build, 1, sel.M0)
    assert st.kernels_in_last_plan == 2, st.kernels_in_last_plan                       # unpaired: linear_in, the gate quantiser, linear_out
    qp.assert_probe(got, qp.reference(Q4_K, seen), "paired gate")


# ---- T >= 2: the row quantisers of the batched mat-mul ---------------------------------------------------------------------------------------
def check_batched(wt, K, M, T, prologue):
    sel = selectors(wt, K)
    M = M or sel.M0
    a, alpha, seen = activation(wt, K, T, prologue)
    ref = qp.reference(wt, seen)
    what = f"{qp.NAMES[wt]} K={K} M={M} T={T} {prologue}"
    members = 1 + (2 if prologue != "plain" else 0)                                    # the mat-mul and its row quantiser's nodes: one plan step
    got, st = run(qp.probe_graph(sel, a, prologue, alpha, None, M), T, M)
    assert (st.kernels_in_last_plan, st.fused_nodes_in_last_plan) == (1, members), (st.kernels_in_last_plan, st.fused_nodes_in_last_plan)
    qp.assert_probe(got, ref, what)
    res = qp.probe_residual(sel, T, M, K + T)
    gotr, st = run(qp.probe_graph(sel, a, prologue, alpha, res, M), T, M)
    assert (st.kernels_in_last_plan, st.fused_nodes_in_last_plan) == (1, members + 1), (st.kernels_in_last_plan, st.fused_nodes_in_last_plan)
    qp.assert_probe(gotr, ref, what + " + residual", residual=res)
    one, st = run(qp.probe_graph(sel, a, prologue, alpha, None, M, per_row=True), T, M)
    assert st.kernels_in_last_plan == T
    n = sel.n_val + sel.n_sum
    issel = (np.arange(M) % sel.M0) < n
    assert np.array_equal(got[:, issel], one[:, issel]), f"{what}: a column differs from the T = 1 launch of its row at (column, selector row) {np.argwhere(got[:, issel] != one[:, issel])[:4].tolist()}"


@pytest.mark.gpu
@pytest.mark.parametrize("prologue", ["plain", "norm", "gate"])
@pytest.mark.parametrize("T", [2, 5, 16, 17, 33, 64])
@pytest.mark.parametrize("K", [256, 512, 2560])
@pytest.mark.parametrize("wt", qp.QUANT, ids=WT_IDS)
def test_batched_matmul_row_quantisers(wt, K, T, prologue):
    check_batched(wt, K, None, T, prologue)


@pytest.mark.gpu
@pytest.mark.parametrize("prologue", ["plain", "norm", "gate"])
@pytest.mark.parametrize("T", [2, 5, 16, 17, 33, 64])
def test_batched_q4k_rows_kernel(T, prologue):
    check_batched(Q4_K, 512, 8200, T, prologue)                                        # M >= 8192: the shared activation tile


# ---- general gate values (l in [-8, 8]): the device's expf is within an ulp of the host's, not equal to it - the tolerant form ---------------------
@pytest.mark.gpu
@pytest.mark.parametrize("wt", qp.QUANT, ids=WT_IDS)
@pytest.mark.parametrize("K,T,per_row", [(512, 8, True), (512, 17, False), (4352, 6, True)], ids=["matvec", "rows", "long_gate"])
def test_general_gate_values_under_the_tolerant_form(wt, K, T, per_row):
    # (the shapes and seeds whose share of near-boundary elements tests/test_quant_probe_cpu.py holds under 1 %)
    sel = selectors(wt, K)
    h, v = qp.gate_general(K, T, seed=K + T)
    got, st = run(qp.probe_graph(sel, h, "gate", per_row=per_row), T, sel.M0)
    assert st.kernels_in_last_plan == (T * (2 if K > 4096 else 1) if per_row else 1), st.kernels_in_last_plan
    near, moved = qp.assert_probe_tolerant(got, wt, v, f"{qp.NAMES[wt]} K={K} T={T}")
    print(f"{qp.NAMES[wt]} K={K} T={T}: {near:.4%} of the elements near a boundary, {moved} blocks with a neighbouring scale (device)")
    assert near <= 0.01


# ---- BF16 / F16: the conversion in front of the float products -------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 1], ids=["f64", "float_acc"])
@pytest.mark.parametrize("prologue", ["plain", "norm", "gate"])
@pytest.mark.parametrize("T", [1, 2, 17, 33])
@pytest.mark.parametrize("K", [96, 512])
@pytest.mark.parametrize("wt", qp.FLOAT, ids=WT_IDS)
def test_float_conversion(wt, K, T, prologue, mode):
    sel = selectors(wt, K)
    rows = max(T, full_set(wt))                                                        # at least every row of every family; T = 1: one mat-vec per row
    a, alpha, seen = activation(wt, K, rows, prologue)
    got, st = run(qp.probe_graph(sel, a, prologue, alpha, per_row=T == 1), rows, K, mode=mode)
    if T == 1:
        assert (st.kernels_in_last_plan, st.float_batched_mms_in_last_plan, st.float_acc_mms_in_last_plan) == (rows, 0, 0)
    else:
        assert (st.kernels_in_last_plan, st.float_batched_mms_in_last_plan, st.float_acc_mms_in_last_plan) == (1, 1 - mode, mode)
    qp.assert_probe(got, qp.reference(wt, seen), f"{qp.NAMES[wt]} K={K} T={T} {prologue} mode {mode}")
