"""GPU: one B-column codec convolution group (moshi_hot.cpp streaming_conv / stateless_conv / resnet_block's add) through the C-ABI with bit 2 of
ggml_backend_mi355x_set_f32_matrix: the whole group is one k_conv_cols_mfma launch (hip_conv_mfma.h). prev is an uploaded random tensor
and is read back as a second result. A case is (IC, OC, Kw, s0, L, B) with L the positions per column: x holds L s0 samples per channel.

The random-operand bound, per element, follows the kernel's arithmetic: operands rounded to F16 give exact float products, and ANY order of the K
float adds errs by at most K 2^-23 S, S = sum |a||w| (each add within one ulp of a partial sum no larger than S). The bias add and the residual add
each round once more: 2^-24 (|value| + error so far). Nothing is fitted to what the device returns."""
import os
import subprocess
import sys

import numpy as np
import pytest

import ggml_util as gu
from ggml_util import F16, F32

pytestmark = pytest.mark.gpu

CASES = [(1, 8, 7, 1, 40, 2, False, False),       # K = 7: one ragged chunk, unaligned weight rows, OC below one tile
         (16, 24, 3, 1, 1, 3, False, False),      # K = 48: a ragged second chunk; a 3-position tile across columns; TP 2 > L 1; a ragged OC tile
         (32, 16, 8, 4, 5, 5, False, False),      # stride; 25 positions across two tiles and column borders
         (64, 32, 7, 1, 2, 33, False, False),     # the decoder's first layer in small: TP 6 > L 2, several runs, the last-arriver tail
         (32, 1, 3, 1, 48, 2, False, False),      # a single output channel
         (32, 64, 1, 1, 17, 3, True, True)]       # the stateless 1-tap block with both folds
WIDEST = (512, 1024, 16, 8, 2, 2, False, False)   # Mimi's widest layer as it is


def group(g, x, w, prev, bias, resid, s0, wt, elu):
    """x [B, IC, Lx], w [OC, IC, Kw], prev [B, IC, TP] or None, bias [OC] or None, resid [B, OC, OW] or None -> (outputs to expand in order, out, prev)"""
    OC = w.shape[0]
    xt, wn = g.input(x), g.input(w, wt)
    pv = g.input(prev) if prev is not None else None
    outs = []
    if elu:
        xt = g.elu(xt)
    if pv is not None:
        TP = prev.shape[2]
        xt = g.concat(pv, xt, 0)
        n = xt.contents
        outs.append(g.cpy(g.view_3d(xt, TP, n.ne[1], n.ne[2], n.nb[1], n.nb[2], n.nb[0] * (n.ne[0] - TP)), pv))
    im = g.im2col(wn, xt, s0, 0, 0, 0, 1, 0, False, F16)
    K, OW, B = (int(im.contents.ne[i]) for i in range(3))
    y = g.mul_mat(g.reshape_2d(im, K, OW * B), g.reshape_2d(wn, K, OC))
    y = g.view_3d(y, OW, OC, B, y.contents.nb[1], OW * y.contents.nb[0], 0)
    y = g.add(y, g.input(bias.reshape(OC, 1))) if bias is not None else g.cont(y)
    if resid is not None:
        y = g.add(g.input(resid), y)
    return outs + [y], y, pv


def run(mode, x, w, prev, bias, resid, s0, wt=F16, elu=False):
    """a fresh handle with set_f32_matrix(mode) -> out [B, OC, OW], the new prev, the plan's counters"""
    g = gu.Graph("hip", mem_mb=128)
    try:
        if mode is not None:
            g.L.ggml_backend_mi355x_set_f32_matrix(g.backend, mode)
        outs, out, pv = group(g, x, w, prev, bias, resid, s0, wt, elu)
        g.build(outs)
        g.alloc()
        g.compute()
        return g.get(out)[0], (g.get(pv)[0] if pv is not None else None), g.stats()
    finally:
        g.free()


def layer(IC, OC, Kw, s0, L, B, residual, ints, seed=0):
    r = np.random.default_rng([IC, OC, Kw, L, B, seed])
    TP, Lx = Kw - s0, L * s0

    def draw(*shape, scale=1.0):
        return r.integers(-8, 9, shape).astype(np.float32) if ints else (scale * r.standard_normal(shape)).astype(np.float32)
    x, w = draw(B, IC, Lx), draw(OC, IC, Kw, scale=1 / np.sqrt(IC * Kw))
    prev = draw(B, IC, TP) if TP else None
    return x, w, prev, draw(OC, scale=0.1), (draw(B, OC, L) if residual else None)


def reference(act, w, prev, bias, resid, s0):
    """act: the activations behind the ELU. float64 (out, its error bound, the new prev) with both operands rounded to F16 as the kernel rounds them"""
    xcat = act if prev is None else np.concatenate([prev, act], 2)
    TP = 0 if prev is None else prev.shape[2]
    a, wh = xcat.astype(np.float16).astype(np.float64), w.astype(np.float16).astype(np.float64)
    (B, IC, _), (OC, _, Kw) = a.shape, w.shape
    OW = (a.shape[2] - Kw) // s0 + 1
    col = np.stack([a[:, :, t:t + (OW - 1) * s0 + 1:s0] for t in range(Kw)], 3)      # [B, IC, OW, Kw]
    out = np.einsum("biok,cik->bco", col, wh)
    err = IC * Kw * 2.0 ** -23 * np.einsum("biok,cik->bco", np.abs(col), np.abs(wh))
    for term in (bias[None, :, None] if bias is not None else None, resid):
        if term is not None:
            out = out + term.astype(np.float64)
            err = err + 2.0 ** -24 * (np.abs(out) + err)
    return out, err, (xcat[:, :, xcat.shape[2] - TP:] if TP else None)


@pytest.mark.parametrize("IC,OC,Kw,s0,L,B,elu,residual", CASES + [WIDEST])
def test_integers_are_exact(IC, OC, Kw, s0, L, B, elu, residual):
    x, w, prev, bias, resid = layer(IC, OC, Kw, s0, L, B, residual, ints=True)
    out, _, tail = reference(x, w, prev, bias, resid, s0)
    assert np.abs(out).max() + 8 * 8 * IC * Kw < 2 ** 24        # every partial sum in any order is an exact float
    got_out, got_prev, st = run(4, x, w, prev, bias, resid, s0)
    assert st.conv_matrix_groups_in_last_plan == 1
    assert np.array_equal(got_out, out)
    assert prev is None or np.array_equal(got_prev, tail)


@pytest.mark.parametrize("IC,OC,Kw,s0,L,B,elu,residual", CASES)
def test_group_against_float64(IC, OC, Kw, s0, L, B, elu, residual):
    x, w, prev, bias, resid = layer(IC, OC, Kw, s0, L, B, residual, ints=False)
    got_out, got_prev, st = run(4, x, w, prev, bias, resid, s0, elu=elu)
    assert st.conv_matrix_groups_in_last_plan == 1
    # the ELU node alone on the device gives the activations the launch rounds and multiplies: expm1f is then no part of the bound
    act = gu.run_graph("hip", lambda g: [g.elu(g.input(x))])[0][0][0] if elu else x
    out, err, tail = reference(act, w, prev, bias, resid, s0)
    ratio = np.abs(got_out - out) / err
    print(f"IC {IC} OC {OC} Kw {Kw} s0 {s0} L {L} B {B} elu {elu} residual {residual}: worst error / bound {ratio.max():.3f}")
    assert ratio.max() <= 1
    assert prev is None or np.array_equal(got_prev, tail)


def test_a_column_has_the_same_bits_at_any_index_of_any_width():
    IC, OC, Kw, s0, L = 64, 32, 7, 1, 2
    res = []
    for B, at in ((2, 1), (33, 20)):
        x, w, prev, bias, _ = layer(IC, OC, Kw, s0, L, B, False, False, seed=B)
        x1, w, prev1, bias, _ = layer(IC, OC, Kw, s0, L, 1, False, False)
        x[at], prev[at] = x1[0], prev1[0]
        out, pv, st = run(4, x, w, prev, bias, None, s0)
        assert st.conv_matrix_groups_in_last_plan == 1
        res.append((out[at], pv[at]))
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])


def small_group_count(mode):
    x, w, prev, bias, _ = layer(32, 16, 8, 4, 5, 5, False, True)
    return run(mode, x, w, prev, bias, None, 4)[2].conv_matrix_groups_in_last_plan


def test_the_setter_masks_with_7():
    assert [small_group_count(mode) for mode in (8 | 4, 8 | 3, 16)] == [1, 0, 0]


@pytest.mark.parametrize("env,want", [("4", 1), ("7", 1), ("3", 0), ("8", 0)])
def test_the_environment_variable_sets_the_starting_value(env, want):
    """MI355X_MMF32 is read once per process: a child that never calls the setter"""
    code = "import test_conv_matrix_gpu as t; print('groups', t.small_group_count(None))"
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, MI355X_MMF32=env, PYTHONPATH=os.path.dirname(__file__)),
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and f"groups {want}" in out.stdout, out.stderr[-2000:]


@pytest.mark.parametrize("mode,wt", [(3, F16), (4, F32)])
def test_off_or_outside_the_claim_is_the_present_plan(mode, wt):
    x, w, prev, bias, _ = layer(32, 16, 8, 4, 5, 5, False, False)
    out, pv, st = run(mode, x, w, prev, bias, None, 4, wt=wt)
    out0, pv0, _ = run(0, x, w, prev, bias, None, 4, wt=wt)
    assert st.conv_matrix_groups_in_last_plan == 0
    assert np.array_equal(out, out0) and np.array_equal(pv, pv0)
