"""GPU: one B-column streaming transposed-convolution group (moshi_hot.cpp streaming_conv_transpose) through the C-ABI with bit 1 of
ggml_backend_mi355x_set_f32_matrix: the whole group is one k_convtr_cols_mfma launch (hip_convtr_mfma.h). prev is an uploaded random
tensor, so one compute exercises the tail add, and it is read back as a second result. The reference is numpy float64 with the same formula.

The bound, per element, follows the kernel's arithmetic. A tap Z = sum over ic of x w is an exact sum of IC exact products in SOME order of double
adds: |error| <= IC 2^-52 sum |x||w|. Every float rounding behind it - the tap, the add of the two taps (or of tap and old tail), the bias add - adds
half a float ulp of the value it rounds, <= 2^-24 (|reference value| + error so far). Nothing is fitted to what the device returns."""
import numpy as np
import pytest

import ggml_util as gu
from ggml_util import F16, F32

pytestmark = pytest.mark.gpu


def group(g, x, w, prev, bias, s0, wt, elu):
    """x [B, IC, L], w [IC, OC, K], prev [B, OC, (L - 1) s0 + K], bias [OC] -> (output tensors to expand in order, out, prev)"""
    (B, IC, L), (_, OC, K) = x.shape, w.shape
    OLf, PT = (L - 1) * s0 + K, K - s0
    xt, wn, pv = g.input(x), g.input(w, wt), g.input(prev)
    if elu:
        xt = g.elu(xt)
    y = g.new(F32, OLf, OC, B)
    xn, yn, pn = xt.contents.nb, y.contents.nb, pv.contents.nb
    cps = []
    for b in range(B):
        yb = g.conv_transpose_1d(wn, g.view_2d(xt, L, IC, xn[1], b * xn[2]), s0, 0, 1)
        cps.append(g.cpy(yb, g.view_2d(y, OLf, OC, yn[1], b * yn[2])))
    partial = g.view_3d(pv, PT, OC, B, pn[1], pn[2], pn[0] * (OLf - PT))
    lower = g.add_inplace(g.view_3d(y, PT, OC, B, yn[1], yn[2], 0), partial)
    st = g.cpy(g.view_3d(lower, OLf, OC, B, yn[1], yn[2], 0), pv)
    if bias is not None:
        st = g.add(st, g.input(bias.reshape(OC, 1)))
    out = g.cont(g.view_3d(st, OLf - PT, OC, B, st.contents.nb[1], st.contents.nb[2], 0))
    return cps + [out], out, pv


def run(mode, x, w, prev, bias, s0, wt=F32, elu=False):
    """a fresh handle with set_f32_matrix(mode) -> out [B, OC, L s0], new prev, the plan's counters"""
    g = gu.Graph("hip")
    try:
        g.L.ggml_backend_mi355x_set_f32_matrix(g.backend, mode)
        outs, out, pv = group(g, x, w, prev, bias, s0, wt, elu)
        g.build(outs)
        g.alloc()
        g.compute()
        return g.get(out)[0], g.get(pv)[0], g.stats()
    finally:
        g.free()


def layer(IC, OC, K, s0, L, B, seed=0):
    r = np.random.default_rng([IC, OC, K, L, B, seed])
    x = r.standard_normal((B, IC, L)).astype(np.float32)
    w = (r.standard_normal((IC, OC, K)) / np.sqrt(IC)).astype(np.float32)
    prev = r.standard_normal((B, OC, (L - 1) * s0 + K)).astype(np.float32)
    return x, w, prev, (0.1 * r.standard_normal(OC)).astype(np.float32)


def rounded(ref, err):
    return err + 2.0 ** -24 * (np.abs(ref) + err)


def reference(x, w, prev, bias, s0):
    """float64 (out, prev) and the error bound of each (module docstring)"""
    x, w = x.astype(np.float64), w.astype(np.float64)
    (B, IC, L), OC = x.shape, w.shape[1]
    Z = np.einsum("bil,iok->bolk", x, w)                                         # [B, OC, L, K]
    eZ = rounded(Z, IC * 2.0 ** -52 * np.einsum("bil,iok->bolk", np.abs(x), np.abs(w)))
    lo, hi, elo, ehi = Z[..., :s0], Z[..., s0:], eZ[..., :s0], eZ[..., s0:]
    y, ey = lo.copy(), elo.copy()
    y[:, :, 1:] += hi[:, :, :-1]
    ey[:, :, 1:] = rounded(y[:, :, 1:], elo[:, :, 1:] + ehi[:, :, :-1])
    y[:, :, 0] += prev[:, :, L * s0:].astype(np.float64)
    ey[:, :, 0] = rounded(y[:, :, 0], elo[:, :, 0])
    y, ey = y.reshape(B, OC, L * s0), ey.reshape(B, OC, L * s0)
    out = y + bias[None, :, None].astype(np.float64)
    return (out, rounded(out, ey)), (np.concatenate([y, hi[:, :, -1]], 2), np.concatenate([ey, ehi[:, :, -1]], 2))


CASES = [(32, 4, 8, 4, 2, 2, False),        # one chunk of IC, a partly filled n tile, 4 positions
         (96, 6, 10, 5, 3, 3, False),       # odd s0, a channel group clamped at OC, a ragged position tile that crosses columns
         (128, 16, 12, 6, 17, 5, False),    # columns that cross position tiles and a round: the tap carried between tiles and between rounds
         (64, 8, 16, 8, 2, 33, False),      # many columns, several position tiles, the column split
         (1024, 512, 16, 8, 2, 2, False),   # Mimi's widest layer as it is
         (128, 16, 12, 6, 17, 5, True)]     # an ELU in front, peeled into the launch


@pytest.mark.parametrize("IC,OC,K,s0,L,B,elu", CASES)
def test_group_against_float64(IC, OC, K, s0, L, B, elu):
    x, w, prev, bias = layer(IC, OC, K, s0, L, B)
    got_out, got_prev, st = run(2, x, w, prev, bias, s0, elu=elu)
    assert st.convtr_matrix_groups_in_last_plan == 1 and st.convtr_column_groups_in_last_plan == 1
    # the ELU node alone on the device gives the activations the launch multiplies: expm1f is then no part of the bound
    act = gu.run_graph("hip", lambda g: [g.elu(g.input(x))])[0][0][0] if elu else x
    (out, e_out), (pv, e_pv) = reference(act, w, prev, bias, s0)
    r_out, r_pv = np.abs(got_out - out) / e_out, np.abs(got_prev - pv) / e_pv
    print(f"IC {IC} OC {OC} K {K} L {L} B {B} elu {elu}: worst error / bound: out {r_out.max():.3f} prev {r_pv.max():.3f}")
    assert r_out.max() <= 1 and r_pv.max() <= 1


def test_a_column_has_the_same_bits_at_any_index_of_any_width():
    IC, OC, K, s0, L = 128, 16, 12, 6, 17
    res = []
    for B, at in ((2, 1), (33, 20)):
        x, w, prev, bias = layer(IC, OC, K, s0, L, B, seed=B)
        x1, w, prev1, bias = layer(IC, OC, K, s0, L, 1)
        x[at], prev[at] = x1[0], prev1[0]
        out, pv, st = run(2, x, w, prev, bias, s0)
        assert st.convtr_matrix_groups_in_last_plan == 1
        res.append((out[at], pv[at]))
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])


@pytest.mark.parametrize("mode,IC,K,s0,wt", [(1, 32, 8, 4, F32), (2, 32, 12, 4, F32), (2, 48, 8, 4, F32), (2, 32, 8, 4, F16)])
def test_off_or_outside_the_claim_is_the_present_pair(mode, IC, K, s0, wt):
    x, w, prev, bias = layer(IC, 4, K, s0, 2, 2)
    out, pv, st = run(mode, x, w, prev, bias, s0, wt=wt)
    out0, pv0, st0 = run(0, x, w, prev, bias, s0, wt=wt)
    assert st.convtr_matrix_groups_in_last_plan == 0 and st.convtr_column_groups_in_last_plan == st0.convtr_column_groups_in_last_plan == 1
    assert np.array_equal(out, out0) and np.array_equal(pv, pv0)
