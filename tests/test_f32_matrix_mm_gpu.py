"""The f64-MFMA batched mat-mul for F32 weights (k_mm_f32_batched: v_mfma_f64_16x16x4_f64 tiles over 2 .. 128 activation rows as they are), opted into
with ggml_backend_mi355x_set_f32_matrix(backend, 1), as a one-node mul_mat graph through the C-ABI.

The reference is s = W x in numpy float64. The bound is derived, not measured: every product of two floats is exact in double, so the device result
is a sum of K exact terms in some order of double adds (error <= (K - 1) 2^-53 sum |w x|, bounded here by K 2^-52 (|W| @ |x|)) rounded once to float
(half an ulp, <= 2^-24 |s|)."""
import numpy as np
import pytest

import ggml_util as gu

pytestmark = pytest.mark.gpu


def operands(K, M, T):
    r = np.random.default_rng(7 * K + 3 * M + T)
    return r.standard_normal((M, K)).astype(np.float32), r.standard_normal((T, K)).astype(np.float32)


def product(w, x):
    """W [K, M] against activations [K, 1, T] - rows over ne[2], as the codec transformers hold theirs ([512, 2, B]): such a node reaches the generic
    product at every T (a 2-D [K, T] operand of a few columns is a k_matvec product, which the option leaves alone)"""
    return lambda g: [g.mul_mat(g.input(w), g.input(x[:, None, :]))]


def run(w, x, on, repeat=1):
    """the product on a fresh handle with the option set to `on` -> ([T, M] per compute, f32_matrix_mms_in_last_plan)"""
    g = gu.Graph("hip")
    try:
        outs = product(w, x)(g)
        g.build(outs)
        g.alloc()
        g.L.ggml_backend_mi355x_set_f32_matrix(g.backend, on)
        got = []
        for _ in range(repeat):
            g.compute()
            got.append(g.get(outs[0]).reshape(x.shape[0], w.shape[0]))
        return got, g.stats().f32_matrix_mms_in_last_plan
    finally:
        g.free()


# K: one chunk with three idle waves, a pair, 9 chunks with a ragged second round, Mimi's width; M: the row clamp; T: the tile edges and both grid.y halves
@pytest.mark.parametrize("T", [2, 16, 17, 64, 65, 128])
@pytest.mark.parametrize("M", [16, 17, 48])
@pytest.mark.parametrize("K", [32, 64, 288, 512])
def test_product_against_float64(K, M, T):
    w, x = operands(K, M, T)
    (got,), n_mms = run(w, x, 1)
    s = x.astype(np.float64) @ w.astype(np.float64).T
    tol = 2.0 ** -24 * np.abs(s) + K * 2.0 ** -52 * (np.abs(x).astype(np.float64) @ np.abs(w).astype(np.float64).T)
    err = np.abs(got.astype(np.float64) - s)
    print(f"K={K} M={M} T={T}: max err / bound = {float((err / tol).max()):.3f}")
    assert n_mms == 1
    assert (err <= tol).all(), f"{int((err > tol).sum())} of {err.size} beyond the bound, worst {float((err / tol).max()):.2f} x at {np.argwhere(err > tol)[:4].tolist()}"


@pytest.mark.parametrize("K,M", [(288, 17), (512, 48)])
def test_a_column_has_the_same_bits_at_any_index_of_any_width(K, M):
    w, x2 = operands(K, M, 2)
    _, x97 = operands(K, M, 97)
    x97[70] = x2[1]
    (a, a2), n_mms = run(w, x2, 1, repeat=2)
    (b,), _ = run(w, x97, 1)
    assert n_mms == 1 and np.array_equal(a, a2), "two runs of one product differ"
    assert np.array_equal(a[1], b[70])


# the claimed shape with the option off; K = 48, M = 8, T = 1 and T = 129 with it on: the generic product's bits, on a handle that never saw the option
@pytest.mark.parametrize("K,M,T,on", [(512, 48, 16, 0), (48, 16, 2, 1), (32, 8, 2, 1), (32, 16, 1, 1), (32, 16, 129, 1)])
def test_off_or_outside_the_claim_is_the_generic_product(K, M, T, on):
    w, x = operands(K, M, T)
    (plain,), pst = gu.run_graph("hip", product(w, x))
    (got,), n_mms = run(w, x, on)
    assert pst.f32_matrix_mms_in_last_plan == 0 and n_mms == 0
    assert np.array_equal(got, plain.reshape(got.shape))
