"""The batched mat-mul for BF16 / F16 weights (k_mm_f_batched: f64 MFMA tiles, 2 .. 64 activation rows) through the C-ABI.

(a) against the oracle's vec_dot_bf16 / vec_dot_f16 (rows rounded to the weight's type, exact products, a double sum, one rounding to float) under
    |got - ref| <= 2^-23 |ref| + 2^-40 S, S = sum_k |w_k x_k| over the rounded operands: one float rounding, plus two double sums of K <= 11264 exact
    products taken in different orders (each within K 2^-53 S <= 2^-39.5 S of the exact sum in the worst case; 2^-40 claims that real error sits well
    below the worst case). The CPU test below holds the oracle's own order against math.fsum to the same bar on the same inputs: it passes with the
    exponent as stated (the oracle's float equals the correctly rounded exact sum on every sampled element), so the exponent is not raised.
(b) every column of a 33 .. 64 column product bit-identical to the same column of a product of at most 16 columns over a view of the same activations
    (and 17 against 2): a column's bits do not depend on T, on the tile count or on its neighbours.
(c) the RMS-norm and gate prologues and the residual epilogue as the graphs the matcher sees, against the oracle and against the unfused plan.

The activations are [K, 1, T] (the shape of the prefill and streams graphs): up to four plain [K, T] columns belong to the float mat-vec."""
import math

import numpy as np
import pytest

import ggml_util as gu
from ggml_util import BF16, F16

TYPES = pytest.mark.parametrize("wt", [BF16, F16], ids=["bf16", "f16"])
# one chunk; a K that is no multiple of 256; an M tail inside a tile; every NT and both sides of each NT boundary; the longest K of moshika (linear_out);
# and one tall shape (513 workgroups, a ragged last one, five chunks dealt 2 + 2 + 1 to the waves)
SHAPES = [(32, 16, 2), (96, 17, 5), (512, 40, 16), (512, 500, 17), (768, 50, 33), (256, 64, 48), (4096, 48, 49), (11264, 32, 64), (160, 8200, 20)]
FOLD_TOL = 2e-6     # tests/test_hip_ops.py test_big_matvec_rmsnorm_prologue_residual_epilogue: atol_rel, with gu.compare's rtol of 1e-5


def rounded(a, wt):
    """float32 array -> the values the weight's type holds (what both sides multiply)"""
    if wt == F16:
        return np.asarray(a, dtype=np.float32).astype(np.float16).astype(np.float32)
    return gu.bf16_bits_to_f32(gu.f32_to_bf16_bits(a))


def operands(wt, K, M, T):
    r = np.random.default_rng(100000 * wt + 7 * K + 3 * M + T)
    w = rounded(r.standard_normal((M, K)) * 0.5, wt)
    x = (r.standard_normal((T, K)) * r.uniform(0.2, 3.0, (T, 1))).astype(np.float32)
    return w, x


def product(wt, K, M, T, w, x):
    def build(g):
        return [g.mul_mat(g.input(w, wt), g.input(x.reshape(T, 1, K)))]
    return build


def bar(ref, w, x, wt):
    S = np.abs(rounded(x, wt).astype(np.float64)) @ np.abs(w.astype(np.float64)).T      # [T, M]
    return 2.0 ** -23 * np.abs(ref.astype(np.float64)) + 2.0 ** -40 * S, S


@TYPES
@pytest.mark.parametrize("K,M,T", SHAPES[:-1])
def test_oracle_sum_order_against_fsum_is_inside_the_bar(wt, K, M, T):
    # CPU: the reference's own summation order against the correctly rounded sum. Rows are sampled where M is large (the bar is per element).
    w, x = operands(wt, K, M, T)
    (ref,), _ = gu.run_graph("oracle", product(wt, K, M, T, w, x))
    ref = ref.reshape(T, M)
    tol, S = bar(ref, w, x, wt)
    xr = rounded(x, wt).astype(np.float64)
    rows = range(0, M, max(1, M // 24))
    worst = 0.0
    for m in rows:
        wm = w[m].astype(np.float64)
        for t in range(T):
            exact = np.float32(math.fsum((wm * xr[t]).tolist()))
            err = abs(float(ref[t, m]) - float(exact))
            assert err <= tol[t, m], (K, M, T, m, t, err, tol[t, m])
            worst = max(worst, err / S[t, m] if S[t, m] else 0.0)
    print(f"K={K} M={M} T={T}: worst |oracle - fsum| / S = 2^{math.log2(worst) if worst else -math.inf:.1f}")


@pytest.mark.gpu
@TYPES
@pytest.mark.parametrize("K,M,T", SHAPES)
def test_product_matches_oracle(wt, K, M, T):
    w, x = operands(wt, K, M, T)
    build = product(wt, K, M, T, w, x)
    (ref,), _ = gu.run_graph("oracle", build)
    (got,), st = gu.run_graph("hip", build)
    ref, got = ref.reshape(T, M), got.reshape(T, M)
    tol, S = bar(ref, w, x, wt)
    err = np.abs(got.astype(np.float64) - ref.astype(np.float64))
    print(f"K={K} M={M} T={T}: max err / bar = {float((err / tol).max()):.3f}, float_batched_mms = {st.float_batched_mms_in_last_plan}")
    assert st.float_batched_mms_in_last_plan == 1, "the product did not run on the f64-MFMA mat-mul"
    assert (err <= tol).all(), f"{int((err > tol).sum())} of {err.size} beyond the bar, worst {float((err / tol).max()):.2f} x at {np.argwhere(err > tol)[:4].tolist()}"


@pytest.mark.gpu
@TYPES
def test_activation_view_at_an_odd_offset_is_declined(wt):
    # the row converters read float4: a contiguous view 4 bytes into its tensor stays on the generic product (same bar, no f64-MFMA launch)
    K, M, T = 96, 17, 5
    w, x = operands(wt, K, M, T)
    flat = np.concatenate([np.zeros(1, np.float32), x.reshape(-1)])

    def build(g):
        return [g.mul_mat(g.input(w, wt), g.view_3d(g.input(flat), K, 1, T, K * 4, K * 4, 4))]
    (ref,), _ = gu.run_graph("oracle", build)
    (got,), st = gu.run_graph("hip", build)
    ref, got = ref.reshape(T, M), got.reshape(T, M)
    tol, _ = bar(ref, w, x, wt)
    assert st.float_batched_mms_in_last_plan == 0
    assert (np.abs(got.astype(np.float64) - ref.astype(np.float64)) <= tol).all()


def column_case(g, wt, w, x, res, T, width, starts):
    K, M = w.shape[1], w.shape[0]
    wtn = g.input(w, wt)
    xt = g.input(x.reshape(T, 1, K))
    rt = g.input(res.reshape(T, 1, M)) if res is not None else None
    full = g.mul_mat(wtn, xt)
    if rt is not None:
        full = g.add(rt, full)
    parts = []
    for c0 in starts:
        y = g.mul_mat(wtn, g.view_3d(xt, K, 1, width, K * 4, K * 4, c0 * K * 4))
        if rt is not None:
            y = g.add(g.view_3d(rt, M, 1, width, M * 4, M * 4, c0 * M * 4), y)
        parts.append(y)
    return [full] + parts


def check_columns(wt, T, width, shapes):
    starts = sorted(set(list(range(0, T - width, width)) + [T - width]))
    for K, M, residual in shapes:
        w, x = operands(wt, K, M, T)
        res = np.random.default_rng(K + M).standard_normal((T, M)).astype(np.float32) if residual else None
        got, st = gu.run_graph("hip", lambda g: column_case(g, wt, w, x, res, T, width, starts))
        assert st.float_batched_mms_in_last_plan == 1 + len(starts)
        full = got[0].reshape(T, M)
        for c0, part in zip(starts, got[1:]):
            assert np.array_equal(full[c0:c0 + width], part.reshape(width, M)), (wt, T, K, M, residual, c0)


@pytest.mark.gpu
@TYPES
@pytest.mark.parametrize("T", [33, 48, 49, 64])
def test_every_column_is_the_column_of_a_16_column_product(wt, T):
    # fewer chunks than the waves take (96: three chunks, two waves idle), many chunks (512), a ragged chunk pair with many workgroups (160 x 8200)
    check_columns(wt, T, 16, [(96, 17, False), (512, 40, True), (160, 8200, True)])


@pytest.mark.gpu
@TYPES
def test_every_column_of_17_is_the_column_of_a_2_column_product(wt):
    check_columns(wt, 17, 2, [(512, 40, True)])


def norm_graph(wt, w, x, alpha, res, T):
    K, M = w.shape[1], w.shape[0]

    def build(g):
        xn = g.mul(g.rms_norm(g.input(x.reshape(T, 1, K)), 1e-8), g.input(alpha))
        return [g.add(g.input(res.reshape(T, 1, M)), g.mul_mat(g.input(w, wt), xn))]
    return build


def gate_graph(wt, w, h, T, streams):
    K = w.shape[1]

    def build(g):
        hh = g.input(h)                                  # [2 K, T]
        nb1 = 2 * K * 4
        if streams:                                      # the B-column step: [F, 1, 1, B]
            left = g.view_4d(hh, K, 1, 1, T, K * 4, K * 4, nb1, 0)
            right = g.view_4d(hh, K, 1, 1, T, K * 4, K * 4, nb1, K * 4)
        else:                                            # prefill: [F, 1, T] (gating.h:16-29)
            left = g.view_4d(hh, K, 1, T, 1, K * 4, nb1, nb1 * T, 0)
            right = g.view_4d(hh, K, 1, T, 1, K * 4, nb1, nb1 * T, K * 4)
        return [g.mul_mat(g.input(w, wt), g.mul(g.silu(left), right))]
    return build


def check_fold(build, members):
    ref, got, st = gu.compare(build, atol_rel=FOLD_TOL)
    assert st.float_batched_mms_in_last_plan == 1
    assert st.fused_nodes_in_last_plan >= members, f"{st.fused_nodes_in_last_plan} fused nodes: the prologue / epilogue did not fold"
    plain, pst = gu.run_graph("hip", build, flags=1)     # the same graph with the fusion passes off
    assert pst.fused_nodes_in_last_plan == 0 and pst.kernels_in_last_plan > st.kernels_in_last_plan
    scale = float(np.abs(ref[0]).max())
    err = np.abs(plain[0] - got[0])
    assert (err <= FOLD_TOL * scale + 1e-5 * np.abs(ref[0])).all(), f"fused vs unfused: max err {err.max():.3e} at scale {scale:.3e}"


@pytest.mark.gpu
@TYPES
@pytest.mark.parametrize("T", [3, 20])
def test_rms_norm_prologue_and_residual_epilogue(wt, T):
    K, M = 512, 96
    w, x = operands(wt, K, M, T)
    r = np.random.default_rng(T)
    alpha = (1.0 + 0.1 * r.standard_normal(K)).astype(np.float32)
    res = r.standard_normal((T, M)).astype(np.float32)
    check_fold(norm_graph(wt, w, x, alpha, res, T), 4)  # mul_mat, mul, rms_norm, add


@pytest.mark.gpu
@TYPES
@pytest.mark.parametrize("streams", [False, True], ids=["prefill_view", "streams_view"])
@pytest.mark.parametrize("T", [3, 20])
def test_gate_prologue(wt, T, streams):
    K, M = 512, 96
    w, _ = operands(wt, K, M, T)
    h = np.random.default_rng(T + 50).standard_normal((T, 2 * K)).astype(np.float32)
    check_fold(gate_graph(wt, w, h, T, streams), 3)    # mul_mat, mul, silu
