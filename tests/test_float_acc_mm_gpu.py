"""The float-accumulating batched mat-mul for BF16 / F16 weights (k_mm_f32acc_batched: v_mfma_f32_16x16x32_bf16 / _f16 tiles, 2 .. 64 activation rows),
opted into with ggml_backend_mi355x_set_float_accumulate(backend, 1) or MI355X_MMF=2, through the C-ABI. Shapes, operands and graphs are those of
tests/test_float_batched_mm_gpu.py (imported, not changed).

(a) integers of -8 .. 8: every product and every partial sum (<= 64 x 11264 < 2^24) is exact in float in any order, so the device result is
    bit-identical to the oracle's double sum - layout, tails, chunk deal and tile boundaries with no tolerance.
(b) random operands against the oracle under |got - ref| <= 2^-23 |ref| + C S, S = sum_k |w_k x_k| over the rounded operands. C = 4 x the larger of
    two measured worst (|err| - 2^-23 |ref|) / S over all shapes and both types:
      CPU float32 emulation of the kernel's order (float_acc_util.emulate)    2^-22.40   (F16, K = 160, M = 8200)
      device (MI355X)                                                        2^-23.80   (F16, K = 160, M = 8200)
    and may not exceed 2^-19 (a dropped or doubled 32-k chunk moves a random-sign result by about 2^-10 S at K = 11264).
(c) every column of a 33 .. 64 column product bit-identical to the same column of a 16-column product (and 17 against 2), in mode 1.
(d) the RMS-norm + residual and gate folds in mode 1: one float-accumulating launch, the fused-node counts of the f64 test, equal to the unfused
    mode-1 plan under FOLD_TOL.
(e) off means off: mode 0 plans the f64 kernel; 1 and back to 0 on one handle gives the bits from before; the odd view is declined in mode 1;
    MI355X_MMF=2 in a child process opts in without the setter."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import float_acc_util as fu
import ggml_util as gu
import test_float_batched_mm_gpu as f64t
from ggml_util import BF16, F16

TYPES = f64t.TYPES
SHAPES = f64t.SHAPES
FOLD_TOL = f64t.FOLD_TOL
EMUL_WORST = 2.0 ** -22.40      # measured: the emulation's worst (|err| - 2^-23 |ref|) / S over SHAPES x TYPES
DEVICE_WORST = 2.0 ** -23.80    # measured on the MI355X, the same quantity (the device sits below the sequential emulation at every shape but one)
C_BAR = 4.0 * max(EMUL_WORST, DEVICE_WORST)
assert C_BAR <= 2.0 ** -19


def bar(ref, w, x, wt):
    S = np.abs(f64t.rounded(x, wt).astype(np.float64)) @ np.abs(w.astype(np.float64)).T      # [T, M]
    return 2.0 ** -23 * np.abs(ref.astype(np.float64)) + C_BAR * S, S


def excess_over_S(got, ref, S):
    """worst (|err| - 2^-23 |ref|) / S: what C has to cover"""
    ref = ref.astype(np.float64)
    e = (np.abs(got.astype(np.float64) - ref) - 2.0 ** -23 * np.abs(ref)) / np.where(S > 0, S, 1.0)
    return float(e.max())


def log2(v):
    return math.log2(v) if v > 0 else -math.inf


# ---- CPU companions ---------------------------------------------------------------------------------------------------------------------------
@TYPES
@pytest.mark.parametrize("K,M,T", SHAPES)
def test_oracle_equals_the_exact_integer_product(wt, K, M, T):
    w, x = fu.integer_operands(K, M, T)
    (ref,), _ = gu.run_graph("oracle", f64t.product(wt, K, M, T, w, x))
    exact = x.astype(np.int64) @ w.astype(np.int64).T
    assert np.abs(exact).max() < 2 ** 24
    assert np.array_equal(ref.reshape(T, M).astype(np.int64), exact) and np.array_equal(ref.reshape(T, M), exact.astype(np.float32))


@TYPES
@pytest.mark.parametrize("K,M,T", SHAPES)
def test_emulated_kernel_order_is_inside_the_bar(wt, K, M, T):
    w, x = f64t.operands(wt, K, M, T)
    (ref,), _ = gu.run_graph("oracle", f64t.product(wt, K, M, T, w, x))
    ref = ref.reshape(T, M)
    tol, S = bar(ref, w, x, wt)
    em = fu.emulate(w, f64t.rounded(x, wt))
    err = np.abs(em.astype(np.float64) - ref.astype(np.float64))
    worst = excess_over_S(em, ref, S)
    print(f"K={K} M={M} T={T}: emulation worst (|err| - 2^-23 |ref|) / S = 2^{log2(worst):.2f}, bar C = 2^{log2(C_BAR):.2f}")
    assert (err <= tol).all()


# ---- (a) ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@TYPES
@pytest.mark.parametrize("K,M,T", SHAPES)
def test_integer_product_is_bit_identical_to_oracle(wt, K, M, T):
    w, x = fu.integer_operands(K, M, T)
    build = f64t.product(wt, K, M, T, w, x)
    (ref,), _ = gu.run_graph("oracle", build)
    (got,), st = fu.run_hip(build, mode=1)
    assert st.float_acc_mms_in_last_plan == 1 and st.float_batched_mms_in_last_plan == 0, (st.float_acc_mms_in_last_plan, st.float_batched_mms_in_last_plan)
    ref, got = ref.reshape(T, M), got.reshape(T, M)
    assert np.array_equal(ref, got), f"{int((ref != got).sum())} of {ref.size} differ, first at {np.argwhere(ref != got)[:4].tolist()}"


# ---- (b) ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@TYPES
@pytest.mark.parametrize("K,M,T", SHAPES)
def test_random_product_matches_oracle(wt, K, M, T):
    w, x = f64t.operands(wt, K, M, T)
    build = f64t.product(wt, K, M, T, w, x)
    (ref,), _ = gu.run_graph("oracle", build)
    (got,), st = fu.run_hip(build, mode=1)
    ref, got = ref.reshape(T, M), got.reshape(T, M)
    tol, S = bar(ref, w, x, wt)
    err = np.abs(got.astype(np.float64) - ref.astype(np.float64))
    em = fu.emulate(w, f64t.rounded(x, wt))
    print(f"K={K} M={M} T={T}: device worst (|err| - 2^-23 |ref|) / S = 2^{log2(excess_over_S(got, ref, S)):.2f}, emulation 2^{log2(excess_over_S(em, ref, S)):.2f}, "
          f"bar C = 2^{log2(C_BAR):.2f}, max err / bar = {float((err / tol).max()):.3f}, device == emulation on {float(np.mean(got == em)):.3f} of the elements")
    assert st.float_acc_mms_in_last_plan == 1 and st.float_batched_mms_in_last_plan == 0
    assert (err <= tol).all(), f"{int((err > tol).sum())} of {err.size} beyond the bar, worst {float((err / tol).max()):.2f} x at {np.argwhere(err > tol)[:4].tolist()}"


# ---- (c) ---------------------------------------------------------------------------------------------------------------------------------------
def check_columns(wt, T, width, shapes):
    starts = sorted(set(list(range(0, T - width, width)) + [T - width]))
    for K, M, residual in shapes:
        w, x = f64t.operands(wt, K, M, T)
        res = np.random.default_rng(K + M).standard_normal((T, M)).astype(np.float32) if residual else None
        got, st = fu.run_hip(lambda g: f64t.column_case(g, wt, w, x, res, T, width, starts), mode=1)
        assert st.float_acc_mms_in_last_plan == 1 + len(starts) and st.float_batched_mms_in_last_plan == 0
        full = got[0].reshape(T, M)
        for c0, part in zip(starts, got[1:]):
            assert np.array_equal(full[c0:c0 + width], part.reshape(width, M)), (wt, T, K, M, residual, c0)


@pytest.mark.gpu
@TYPES
@pytest.mark.parametrize("T", [33, 48, 49, 64])
def test_every_column_is_the_column_of_a_16_column_product(wt, T):
    check_columns(wt, T, 16, [(96, 17, False), (512, 40, True), (160, 8200, True)])


@pytest.mark.gpu
@TYPES
def test_every_column_of_17_is_the_column_of_a_2_column_product(wt):
    check_columns(wt, 17, 2, [(512, 40, True)])


# ---- (d) ---------------------------------------------------------------------------------------------------------------------------------------
def check_fold(build, members):
    ref, _ = gu.run_graph("oracle", build)
    got, st = fu.run_hip(build, mode=1)
    assert st.float_acc_mms_in_last_plan == 1 and st.float_batched_mms_in_last_plan == 0
    assert st.fused_nodes_in_last_plan >= members, f"{st.fused_nodes_in_last_plan} fused nodes: the prologue / epilogue did not fold"
    plain, pst = fu.run_hip(build, mode=1, flags=1)     # the same graph with the fusion passes off, still on the float-accumulating kernel
    assert pst.float_acc_mms_in_last_plan == 1 and pst.fused_nodes_in_last_plan == 0 and pst.kernels_in_last_plan > st.kernels_in_last_plan
    scale = float(np.abs(ref[0]).max())
    err = np.abs(plain[0] - got[0])
    assert (err <= FOLD_TOL * scale + 1e-5 * np.abs(ref[0])).all(), f"fused vs unfused: max err {err.max():.3e} at scale {scale:.3e}"


@pytest.mark.gpu
@TYPES
@pytest.mark.parametrize("T", [3, 20])
def test_rms_norm_prologue_and_residual_epilogue(wt, T):
    K, M = 512, 96
    w, x = f64t.operands(wt, K, M, T)
    r = np.random.default_rng(T)
    alpha = (1.0 + 0.1 * r.standard_normal(K)).astype(np.float32)
    res = r.standard_normal((T, M)).astype(np.float32)
    check_fold(f64t.norm_graph(wt, w, x, alpha, res, T), 4)  # mul_mat, mul, rms_norm, add


@pytest.mark.gpu
@TYPES
@pytest.mark.parametrize("streams", [False, True], ids=["prefill_view", "streams_view"])
@pytest.mark.parametrize("T", [3, 20])
def test_gate_prologue(wt, T, streams):
    K, M = 512, 96
    w, _ = f64t.operands(wt, K, M, T)
    h = np.random.default_rng(T + 50).standard_normal((T, 2 * K)).astype(np.float32)
    check_fold(f64t.gate_graph(wt, w, h, T, streams), 3)    # mul_mat, mul, silu


# ---- (e) ---------------------------------------------------------------------------------------------------------------------------------------
OFF_SHAPE = (512, 40, 16)


@pytest.mark.gpu
@TYPES
def test_mode_0_is_the_f64_kernel_and_a_round_trip_through_mode_1_changes_nothing(wt):
    K, M, T = OFF_SHAPE
    w, x = f64t.operands(wt, K, M, T)
    build = f64t.product(wt, K, M, T, w, x)
    (plain,), pst = gu.run_graph("hip", build)               # a handle the setter never touched
    assert pst.float_acc_mms_in_last_plan == 0 and pst.float_batched_mms_in_last_plan == 1
    (a, sa), (b, sb), (c, sc) = fu.run_hip(build, modes=[0, 1, 0])
    assert (sa.float_acc_mms_in_last_plan, sa.float_batched_mms_in_last_plan) == (0, 1)
    assert (sb.float_acc_mms_in_last_plan, sb.float_batched_mms_in_last_plan) == (1, 0)
    assert (sc.float_acc_mms_in_last_plan, sc.float_batched_mms_in_last_plan) == (0, 1)
    assert np.array_equal(a[0], c[0]) and np.array_equal(a[0], plain)


@pytest.mark.gpu
@TYPES
def test_activation_view_at_an_odd_offset_is_declined_in_mode_1(wt):
    K, M, T = 96, 17, 5
    w, x = f64t.operands(wt, K, M, T)
    flat = np.concatenate([np.zeros(1, np.float32), x.reshape(-1)])

    def build(g):
        return [g.mul_mat(g.input(w, wt), g.view_3d(g.input(flat), K, 1, T, K * 4, K * 4, 4))]
    (ref,), _ = gu.run_graph("oracle", build)
    (got,), st = fu.run_hip(build, mode=1)
    ref, got = ref.reshape(T, M), got.reshape(T, M)
    tol, _ = f64t.bar(ref, w, x, wt)                        # the generic product: the f64 test's bar
    assert st.float_acc_mms_in_last_plan == 0 and st.float_batched_mms_in_last_plan == 0
    assert (np.abs(got.astype(np.float64) - ref.astype(np.float64)) <= tol).all()


def child_counters():
    K, M, T = OFF_SHAPE
    w, x = f64t.operands(BF16, K, M, T)
    _, st = gu.run_graph("hip", f64t.product(BF16, K, M, T, w, x))
    return {"float_acc_mms": st.float_acc_mms_in_last_plan, "float_batched_mms": st.float_batched_mms_in_last_plan}


@pytest.mark.gpu
def test_mmf_2_in_the_environment_opts_a_fresh_handle_in():
    # MI355X_MMF is read once per process: a child process, the setter never called
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-counters"], env=dict(os.environ, MI355X_MMF="2"),
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert p.returncode == 0 and lines, p.stdout[-2000:]
    assert json.loads(lines[-1]) == {"float_acc_mms": 1, "float_batched_mms": 0}


if __name__ == "__main__" and sys.argv[1:] == ["--child-counters"]:
    print(json.dumps(child_counters()))
