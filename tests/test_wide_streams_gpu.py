"""-m gpu: B-column models of 17 .. 64 conversations on the MI355X. The batched int8-MFMA mat-muls take 33 .. 64 activation columns in ONE pass
(three and four 16-column tiles against a weight tile that is staged and unpacked once): against the oracle, and column by column bit-equal to the
same columns computed as a product of 32. Slots models at B = 17, 33 and 64 against the oracle's slots model, the plans of a B = 64 step (one
launch for the 64 mask rows, as many Temporal launches as at B = 16) and slots against lockstep at B = 64."""
import os
import subprocess
import sys

import numpy as np
import pytest

import ggml_util as gu
import hot_util as hu
import sampling_util as sp
import slots_util as sl
import streams_util as su
from ggml_util import F32, Q4_0, Q4_K, Q8_0

pytestmark = pytest.mark.gpu
L = hu.L
RING = 8
GEN = {Q4_K: gu.random_q4_K, Q8_0: gu.random_q8_0, Q4_0: gu.random_q4_0}
MM_TOL = 2e-6      # tests/test_hip_ops.py: test_batched_q4k_matmul_int8_mfma and test_batched_q80_q40_matmul_int8_mfma, atol_rel of every type


def windows(T):
    """column windows of 32 that cover 0 .. T - 1 (the last one overlaps the first where T < 64): every column is in a product of 32 columns"""
    return [0, T - 32]


def mm_case(g, wraw, gt, K, M, T, x, res):
    """-> [the T-column product (+ residual)], [the same over each 32-column window of the same activations (and residual rows)]"""
    w = g.input_raw(wraw, gt, K, M)
    xt = g.input(x)
    rt = g.input(res) if res is not None else None
    full = g.mul_mat(w, xt)
    if rt is not None:
        full = g.add(rt, full)
    parts = []
    for c0 in windows(T):
        y = g.mul_mat(w, g.view_2d(xt, K, 32, K * 4, c0 * K * 4))
        if rt is not None:
            y = g.add(g.view_2d(rt, M, 32, M * 4, c0 * M * 4), y)
        parts.append(y)
    return full, parts


def check_wide_matmul(gt, T, shapes):
    r = np.random.default_rng(1000 * gt + T)
    cases = []
    for K, M, residual in shapes:
        x = (r.standard_normal((T, K)) * r.uniform(0.2, 3.0, (T, 1))).astype(np.float32)
        res = r.standard_normal((T, M)).astype(np.float32) if residual else None
        cases.append((GEN[gt](r, M, K), K, M, x, res))

    def build_full(g):
        return [mm_case(g, wraw, gt, K, M, T, x, res)[0] for wraw, K, M, x, res in cases]
    gu.compare(build_full, atol_rel=MM_TOL)                           # (a) the oracle

    def build_both(g):
        outs = []
        for wraw, K, M, x, res in cases:
            full, parts = mm_case(g, wraw, gt, K, M, T, x, res)
            outs += [full] + parts
        return outs
    got, _ = gu.run_graph("hip", build_both)
    n = 1 + len(windows(T))
    for i, (wraw, K, M, x, res) in enumerate(cases):                  # (b) every column, bit for bit, the column of a 32-column product
        full = got[n * i].reshape(T, M)
        for c0, part in zip(windows(T), got[n * i + 1:n * (i + 1)]):
            assert np.array_equal(full[c0:c0 + 32], part.reshape(32, M)), (gt, T, K, M, res is not None, c0)


@pytest.mark.parametrize("T", [33, 48, 49, 64])
@pytest.mark.parametrize("gt", [Q4_K, Q8_0, Q4_0], ids=["q4_k", "q8_0", "q4_0"])
def test_wide_matmul_matches_oracle_and_32_column_products(gt, T):
    # every tile edge (33: a last tile of one column, 48 / 64: full tiles, 49); M = 16: one workgroup, 40: a ragged last row block; K = 256 / 512: one
    # and two blocks; with and without the residual operand of the graph form
    check_wide_matmul(gt, T, [(K, M, residual) for K in (256, 512) for M in (16, 40) for residual in (False, True)])


def test_wide_matmul_rows_variant():
    check_wide_matmul(Q4_K, 64, [(256, 8192, True)])                  # M >= 8192: the shared-activation-tile kernel, four column tiles


def test_wide_matmul_of_every_family_under_the_switch():
    # MI355X_MMQ_WIDE is read once per process and the Q8_0 / Q4_0 kernel keeps passes of 32 by default: the mat-mul cases above
    # once more in a child process with every kernel family in one pass - there the three- and four-tile Q8_0 / Q4_0 kernels run
    env = dict(os.environ, MI355X_MMQ_WIDE="7")
    p = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", os.path.abspath(__file__), "-k", "test_wide_matmul_matches or rows_variant"],
                       env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert p.returncode == 0 and "13 passed" in p.stdout, p.stdout[-2000:]


def tiny_slots(lt, et, contractive=True):
    cfg = su.lm_only(hu.hot.tiny(L, linear_type=lt, embed_type=et, context=RING))
    cfg.wide_streams = 1
    if contractive:
        cfg.update_scale = 1.0 / 256   # (include/moshi_hot.h) rounding flips stay local instead of compounding over free-running frames
    return cfg


def staggered_events(B):
    """slot b opens at frame b % 6 (the last slot stays closed); slot 0 is reopened after its conversation ran past the 8-slot ring's wrap; slot 3 is
    closed before its ring filled and reopened later"""
    ev = {}
    for b in range(B - 1):
        ev.setdefault(b % 6, []).append(("open", b))
    ev.setdefault(RING + 2, []).extend([("close", 0), ("open", 0)])
    ev.setdefault(8, []).append(("close", 3))
    ev.setdefault(11, []).append(("open", 3))
    return ev


def slot_sampling(b):
    return (4000 + 17 * b, 0.6 + 0.1 * (b % 5), 0.5 + 0.1 * (b % 4), 20 if b % 3 else 6, 25 if b % 3 != 1 else 4)


def run_slots(kind, cfg, B, codes, events, seeded=False):
    s = sp.Slots(kind, cfg, B, seed=0)
    if seeded:
        for b in range(B):
            assert s.set_sampling(b, *slot_sampling(b)) == 0
    rec = sl.run_slots(s, codes, events)
    s.free()
    return rec


def check_tokens(cfg, B, seeded=False):
    n = 2 * RING + 2
    codes = sl.slot_codes(cfg, B, n, seed=B)
    events = staggered_events(B)
    ref = run_slots("oracle", cfg, B, codes, events, seeded)
    got = run_slots("hip", cfg, B, codes, events, seeded)
    bad = [i for i, (a, b) in enumerate(zip(ref, got)) if a[:4] != b[:4]]
    for i in bad[:2]:
        cols = [b for b in range(B) if (ref[i][1][b], ref[i][2][b], ref[i][3][b]) != (got[i][1][b], got[i][2][b], got[i][3][b])]
        print(f"frame {i}: columns {cols} differ")
    assert not bad, f"{len(bad)} of {n} frames differ, first at frame {bad[0]}"
    assert any(r[0] >= B - 2 for r in ref) and len({t for r in ref for t in r[2] if t >= 0}) > 1


@pytest.mark.parametrize("B", [17, 33, 64])
@pytest.mark.parametrize("lt,et", [(Q4_K, Q4_0), (Q8_0, Q8_0)], ids=["q4_k", "q8_0"])
def test_staggered_and_reopened_slots_match_oracle_tokens(lt, et, B):
    check_tokens(tiny_slots(lt, et), B)


def test_seeded_sampled_slots_match_oracle_tokens_at_33():
    check_tokens(sp.sampled(tiny_slots(Q4_K, Q4_0)), 33, seeded=True)


def temporal_plan(cfg, B):
    """-> the launches of the Temporal plan after slots steps that leave the slots at three different positions"""
    s = sl.Slots("hip", cfg, B)
    codes = sl.slot_codes(cfg, B, 3, seed=2)
    for i, fr in enumerate(codes):
        for b in range(B):
            if b % 3 == i:
                s.open(b)
        s.step(fr)
    # the Temporal graph once more on its own (same inputs, same ring slots): its plan is the last one
    assert L.ggml_backend_graph_compute(s.be, L.moshi_hot_graph(s.m, 0)) == 0
    temporal = s.stats().kernels_in_last_plan
    s.free()
    return temporal


def test_b64_temporal_plan_has_the_launch_count_of_b16():
    cfg = tiny_slots(Q4_K, Q4_0)
    assert temporal_plan(cfg, 64) == temporal_plan(cfg, 16)


def test_sampled_b33_depth_plan_has_one_launch_per_sampler_site():
    # a model of more than 16 columns raises its handle's sampler width (ggml_backend_mi355x_set_max_columns): the bound of tests/test_sampling_gpu.py's
    # B = 8 plan test, which has no room for a sampler run as its node chain (about ten launches per site)
    cfg = sp.sampled(tiny_slots(Q4_K, Q4_0))
    B = 33
    s = sp.Slots("hip", cfg, B)
    for b in range(B):
        s.open(b)
        assert s.set_sampling(b, *slot_sampling(b)) == 0
    for fr in sl.slot_codes(cfg, B, 4, seed=2):
        s.step(fr)
    depth = s.stats().kernels_in_last_plan                   # the Depth graph is the last graph of a step
    s.free()
    bound = cfg.dep_q * (6 * cfg.dep_layers + 6)
    assert depth <= bound, f"{depth} launches in the sampled B = 33 Depth plan (bound {bound})"


def test_64_mask_rows_of_the_slots_step_are_one_launch():
    # the scratch graph of the slots step (moshi_hot.cpp transformer_graph_step_slots) as tests/test_slots_gpu.py builds it, for 64 slots
    B, C_ = 64, 24
    width = 3 * C_ - 1
    pattern = np.where(np.arange(width) < 2 * C_, 0.0, -np.inf).astype(np.float32)
    positions = [(7 * b + 3 * (b % 2) * C_) for b in range(B)]
    cols = [2 * C_ - 1 - p if p <= C_ else C_ - p % C_ for p in positions]

    def build(g):
        pat = g.input(pattern)
        dst = g.new(F32, C_, 1, 1, B)
        outs = []
        for b in range(B):
            row = g.cont(g.view_2d(pat, C_, 1, width * 4, cols[b] * 4))
            outs.append(g.cpy(row, g.view_1d(dst, C_, b * C_ * 4)))
        return outs, [dst]
    res, st = gu.run_graph("hip", build)
    want = np.stack([pattern[c:c + C_] for c in cols]).reshape(B, 1, 1, C_)
    assert np.array_equal(res[-1], want)
    assert st.kernels_in_last_plan == 1, f"{st.kernels_in_last_plan} launches for {B} mask rows"


def test_all_64_slots_open_at_frame_zero_equal_device_lockstep():
    cfg = tiny_slots(Q4_K, Q4_0, contractive=False)
    B, n = 64, RING + 4
    codes = sl.slot_codes(cfg, B, n, seed=30 + B)
    ref = su.run_streams("hip", cfg, codes, logits=True)
    s = sl.Slots("hip", cfg, B)
    got = sl.run_slots(s, codes, {0: [("open", b) for b in range(B)]}, logits=True)
    s.free()
    for k, (g, r) in enumerate(zip(got, ref)):
        assert g[1] == [r[0]] * B, k
        if r[0]:
            assert g[2] == r[1] and g[3] == r[2], k
        assert np.array_equal(g[4], r[3]), k
