"""The bits of the three float MFMA batched mat-muls (BF16 / F16 on f64 tiles, BF16 / F16 float-accumulating, F32 on f64 tiles), pinned: every case runs
a one-node (or one fused group) graph through the C-ABI and compares the sha256 of its float32 output bytes with tests/golden/mm_float_bits.json.

The fixture was recorded on an MI355X from the commit BEFORE the three kernels were folded into mm_mfma_kernel<Op, NT> (hip_mm_tile.h): the chunk -> wave
deal, the order of a wave's chunks, the cross-wave sum and the clamps decide every bit below, and a digest that moves means one of them moved. To record
(only ever from a build whose bits are the intended ones): MM_FLOAT_BITS_RECORD=<path of the json to write> python -m pytest tests/test_mm_float_bits_gpu.py -m gpu

Operands, graphs and runners are those of tests/test_float_batched_mm_gpu.py, tests/test_float_acc_mm_gpu.py and tests/test_f32_matrix_mm_gpu.py
(imported, not changed)."""
import hashlib
import json
import os

import numpy as np
import pytest

import float_acc_util as fu
import test_f32_matrix_mm_gpu as f32t
import test_float_batched_mm_gpu as f64t
from ggml_util import BF16, F16

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mm_float_bits.json")
RECORD = os.environ.get("MM_FLOAT_BITS_RECORD")
WT = {"bf16": BF16, "f16": F16}
# the float-accumulating deal is in groups of four chunks: 160 and 544 (5 and 17 chunks) put a ragged group in the first and in the second round;
# then every shape of the f64 list that is not among them
ACC_SHAPES = [(32, 16, 2), (160, 17, 5), (544, 40, 17), (512, 500, 33), (4096, 48, 49), (768, 50, 64)]
ACC_SHAPES += [s for s in f64t.SHAPES if s not in ACC_SHAPES]
F32_SHAPES = [(K, M, T) for K in (32, 64, 288, 512) for M in (16, 17, 48) for T in (2, 16, 17, 64, 65, 128)]
FOLD_SHAPES = [(512, 40, 16), (768, 50, 33)]
FOLDS = {"norm": 4, "gate_prefill": 3, "gate_streams": 3}     # -> the members of the fused group (tests/test_float_batched_mm_gpu.py (c))


def check(case, got):
    digest = hashlib.sha256(np.ascontiguousarray(got, dtype=np.float32).tobytes()).hexdigest()
    if RECORD:
        known = json.load(open(RECORD)) if os.path.exists(RECORD) else {}
        known[case] = digest
        with open(RECORD, "w") as f:
            json.dump(known, f, indent=0, sort_keys=True)
            f.write("\n")
        return
    with open(FIXTURE) as f:
        want = json.load(f)
    assert case in want, f"{case}: not in the fixture"
    assert digest == want[case], f"{case}: the output's bits moved"


def counters(st, mode):
    assert (st.float_batched_mms_in_last_plan, st.float_acc_mms_in_last_plan) == ((0, 1) if mode else (1, 0)), \
        (mode, st.float_batched_mms_in_last_plan, st.float_acc_mms_in_last_plan)


@pytest.mark.parametrize("K,M,T", f64t.SHAPES)
@pytest.mark.parametrize("wt", WT)
def test_f64_form(wt, K, M, T):
    w, x = f64t.operands(WT[wt], K, M, T)
    (got,), st = fu.run_hip(f64t.product(WT[wt], K, M, T, w, x), mode=0)
    counters(st, 0)
    check(f"f64-{wt}-{K}-{M}-{T}", got)


@pytest.mark.parametrize("K,M,T", ACC_SHAPES)
@pytest.mark.parametrize("wt", WT)
def test_float_accumulating_form(wt, K, M, T):
    w, x = f64t.operands(WT[wt], K, M, T)
    (got,), st = fu.run_hip(f64t.product(WT[wt], K, M, T, w, x), mode=1)
    counters(st, 1)
    check(f"f32acc-{wt}-{K}-{M}-{T}", got)


@pytest.mark.parametrize("K,M,T", F32_SHAPES)
def test_f32_form(K, M, T):
    w, x = f32t.operands(K, M, T)
    (got,), n_mms = f32t.run(w, x, 1)
    assert n_mms == 1
    check(f"f32-{K}-{M}-{T}", got)


@pytest.mark.parametrize("K,M,T", FOLD_SHAPES)
@pytest.mark.parametrize("fold", FOLDS)
@pytest.mark.parametrize("mode", [0, 1], ids=["f64", "f32acc"])
@pytest.mark.parametrize("wt", WT)
def test_both_forms_behind_the_prologues_and_the_residual(wt, mode, fold, K, M, T):
    w, x = f64t.operands(WT[wt], K, M, T)
    r = np.random.default_rng(T)
    if fold == "norm":
        alpha = (1.0 + 0.1 * r.standard_normal(K)).astype(np.float32)
        build = f64t.norm_graph(WT[wt], w, x, alpha, r.standard_normal((T, M)).astype(np.float32), T)
    else:
        h = np.random.default_rng(T + 50).standard_normal((T, 2 * K)).astype(np.float32)
        build = f64t.gate_graph(WT[wt], w, h, T, fold == "gate_streams")
    (got,), st = fu.run_hip(build, mode=mode)
    counters(st, mode)
    assert st.fused_nodes_in_last_plan >= FOLDS[fold], f"{st.fused_nodes_in_last_plan} fused nodes: the prologue / epilogue did not fold"
    check(f"fold-{'f32acc' if mode else 'f64'}-{wt}-{fold}-{K}-{M}-{T}", got)
