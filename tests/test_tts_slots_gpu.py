"""-m gpu: tts-shaped B-column models on the MI355X.

Op level: the cross-attention node sequence over K / V [D, Tc, H, B] and q [D * H, 1, B] as ONE launch (cross_attn_streams_kernel, one workgroup per
(head, column)). Column b of the result is the single-column launch's result for that column's q / K / V bit for bit - it is the same device function
in the same order - and within the F32 bar of tests/test_slots_gpu.py (1e-5 of the largest value) of the oracle; with MI355X_NO_CROSS_ATTN_FUSION (a
fresh process: the switch is read once) the plain nodes meet the same bar. The weight-and-bias LayerNorm group over the B rows of a [dim, 1, B]
activation: one launch, every row bit-equal to the one-row launch.

Model level (contractive tiny_tts, ring of 8 so that it wraps, cross_len 5, per-column conditions and text streams): bars as tests/test_slots_gpu.py -
status and tokens equal the oracle's slots model, text logits per weight type in that module's statistical form."""
import os
import subprocess
import sys

import numpy as np
import pytest

import ggml_util as gu
import hot_util as hu
import tts_slots_util as tu
from ggml_util import F32, Q4_0, Q4_K, Q8_0
from test_slots_gpu import RING, TYPE_TOL, staggered_events

pytestmark = pytest.mark.gpu
L = hu.L
TOL = TYPE_TOL[F32]

# D, Tc, H, B
XATTN_CASES = [(128, 5, 4, 2), (128, 5, 4, 3), (128, 5, 4, 16),   # the tiny shape: the t0 + u < Tc clamp, waves with no rows, two P x V groups with an uneven split
               (128, 1, 4, 3),                                     # soft_max of one value; the second P x V group is empty
               (64, 17, 4, 3),                                     # four P x V groups; the scores spill into a second 16-row round
               (256, 7, 2, 2),                                     # G = 1
               (128, 64, 16, 2)]                                   # the tts_like shape


def xattn_inputs(D, Tc, H, B, big_column=None, seed=0):
    rng = np.random.default_rng(seed + D + 7 * Tc + 31 * B)
    K = rng.standard_normal((B, H, Tc, D)).astype(np.float32)
    V = rng.standard_normal((B, H, Tc, D)).astype(np.float32)
    q = rng.standard_normal((B, 1, D * H)).astype(np.float32)
    if big_column is not None:     # a column mix-up or a wrong nb3 cannot pass: this column's values are 64 times anybody else's
        K[big_column] *= 64
        V[big_column] *= 64
    return K, V, q


def run_xattn(kind, K, V, q):
    """-> (x [B, 1, D * H], launches or None)"""
    H, D = K.shape[1], K.shape[3]
    g = gu.Graph(kind)
    try:
        x = tu.cross_attention_nodes(g, g.input(K), g.input(V), g.input(q), H, 1.0 / np.sqrt(D))
        g.build([x])
        g.alloc()
        g.compute()
        return g.get(x).reshape(q.shape), (g.stats().kernels_in_last_plan if kind == "hip" else None)
    finally:
        g.free()


def check_xattn(D, Tc, H, B, big_column=None):
    K, V, q = xattn_inputs(D, Tc, H, B, big_column)
    ref, _ = run_xattn("oracle", K, V, q)
    got, launches = run_xattn("hip", K, V, q)
    assert launches == 1, f"{launches} launches"
    for b in range(B):
        one, n1 = run_xattn("hip", K[b:b + 1], V[b:b + 1], q[b:b + 1])
        assert n1 == 1
        assert np.array_equal(one[0], got[b]), f"column {b} differs from the single-column launch"
        err = hu.rel_err(ref[b], got[b])
        print(f"cross-attention D {D} Tc {Tc} H {H} B {B} column {b}: rel err {err:.2e}")
        assert np.all(np.isfinite(got[b])) and err < TOL, (b, err)


@pytest.mark.parametrize("D,Tc,H,B", XATTN_CASES)
def test_cross_attention_columns_are_one_launch_bit_equal_to_single_column_launches(D, Tc, H, B):
    check_xattn(D, Tc, H, B)


@pytest.mark.parametrize("D,Tc,H,B,big", [(128, 5, 4, 3, 1), (128, 64, 16, 2, 0), (64, 17, 4, 3, 2)])
def test_cross_attention_with_one_large_column(D, Tc, H, B, big):
    check_xattn(D, Tc, H, B, big_column=big)


PLAIN_CHILD = r'''
import numpy as np
import hot_util as hu
import test_tts_slots_gpu as t
for D, Tc, H, B in t.XATTN_CASES:
    K, V, q = t.xattn_inputs(D, Tc, H, B)
    ref, _ = t.run_xattn("oracle", K, V, q)
    got, launches = t.run_xattn("hip", K, V, q)
    assert launches > 1, launches
    for b in range(B):
        err = hu.rel_err(ref[b], got[b])
        assert np.all(np.isfinite(got[b])) and err < t.TOL, (D, Tc, H, B, b, err)
print("OK")
'''


def test_plain_nodes_meet_the_bar_with_the_fusion_switched_off():
    env = dict(os.environ, PYTHONPATH=os.path.dirname(os.path.abspath(__file__)), MI355X_NO_CROSS_ATTN_FUSION="1")
    r = subprocess.run([sys.executable, "-c", PLAIN_CHILD], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and "OK" in r.stdout, (r.stdout + r.stderr)[-2000:]


def run_layernorm(kind, x, w, b):
    """LayerNorm (eps 0) with weight and bias over the rows of x [B, 1, n] -> ([B, 1, n], launches)"""
    g = gu.Graph(kind)
    try:
        y = g.add(g.mul(g.norm(g.input(x), 0.0), g.input(w)), g.input(b))
        g.build([y])
        g.alloc()
        g.compute()
        return g.get(y).reshape(x.shape), (g.stats().kernels_in_last_plan if kind == "hip" else None)
    finally:
        g.free()


@pytest.mark.parametrize("B", [2, 3, 16])
def test_layernorm_group_over_b_rows_is_one_launch(B):
    n = 512
    rng = np.random.default_rng(B)
    x = (rng.standard_normal((B, 1, n)) * (1 + np.arange(B)).reshape(B, 1, 1) + 0.5).astype(np.float32)
    w = (1.0 + 0.1 * rng.standard_normal(n)).astype(np.float32)
    bias = (0.02 * rng.standard_normal(n)).astype(np.float32)
    ref, _ = run_layernorm("oracle", x, w, bias)
    got, launches = run_layernorm("hip", x, w, bias)
    assert launches == 1, launches
    for r in range(B):
        one, n1 = run_layernorm("hip", x[r:r + 1], w, bias)
        assert n1 == 1 and np.array_equal(one[0], got[r]), r
        assert hu.rel_err(ref[r], got[r]) < TOL, (r, hu.rel_err(ref[r], got[r]))


# ---- model level --------------------------------------------------------------------------------------------------------------------------------
TYPES = pytest.mark.parametrize("lt,et", [(F32, F32), (Q8_0, Q8_0), (Q4_K, Q4_0)], ids=["f32", "q8_0", "q4_k"])


def tiny_tts_slots(lt, et):
    cfg = tu.tts_cfg(linear_type=lt, embed_type=et, layers=2, cross_len=5)
    cfg.context = RING
    cfg.update_scale = 1.0 / 256   # (include/moshi_hot.h) rounding flips stay local instead of compounding over free-running frames
    return cfg


def run_slots(kind, cfg, B, n, events, recondition=None):
    """-> per frame (n_valid, status, texts, audios, text_logits [B, text_card], transformer_out [B, dim]); column b: conditions of seed 4 + b, text
    stream b by the frame index; recondition = (frame, column, seed): that column's conditions are set again before that frame"""
    s = tu.Slots(kind, cfg, B, seed=0)
    for b in range(B):
        assert s.set_conditions(b, 4 + b) == 0
    streams = [tu.text_stream(cfg, b, n) for b in range(B)]
    out = []
    for i in range(n):
        for what, b in events.get(i, []):
            assert (s.open(b) if what == "open" else s.close(b)) == 0
        if recondition and recondition[0] == i:
            assert s.set_conditions(recondition[1], recondition[2]) == 0
        r = s.step([streams[b][i] for b in range(B)])
        out.append(r + (s.read("text_logits", cfg.text_card), s.read("transformer_out", cfg.dim)))
    s.free()
    return out


@pytest.mark.parametrize("B", [3, 8])
@TYPES
def test_staggered_tts_slots_match_oracle(lt, et, B):
    cfg = tiny_tts_slots(lt, et)
    n = 2 * RING + 2               # past delay_steps + max(delays) of every conversation and the wrap of the 8-slot ring
    events = staggered_events(B)
    ref = run_slots("oracle", cfg, B, n, events)
    got = run_slots("hip", cfg, B, n, events)
    errs = []
    for i, (a, b) in enumerate(zip(ref, got)):
        assert a[:4] == b[:4], f"frame {i}: status or tokens differ: oracle {a[:4]} vs hip {b[:4]}"
        for s in range(B):
            if a[1][s] != -1:
                errs.append(hu.rel_err(a[4][s], b[4][s]))
    assert any(r[0] > 0 for r in ref) and any(0 in r[1] for r in ref)
    errs = np.array(errs)
    tol = TYPE_TOL[lt]
    print(f"text logit rel errors: median {np.median(errs):.2e} max {errs.max():.2e}")
    assert np.median(errs) < min(tol, 1e-5), f"median logit error {np.median(errs):.2e}"
    assert np.mean(errs < tol) >= 0.9 and errs.max() < 0.1, f"logit errors over the bar {tol:.0e}: {np.sort(errs)[-8:]}"


@TYPES
def test_lockstep_tts_streams_match_oracle(lt, et):
    cfg = tiny_tts_slots(lt, et)
    n, B = RING + 4, 2

    def run(kind):
        s = tu.Streams(kind, cfg, B, seed=0)
        for b in range(B):
            assert s.set_conditions(b, 4 + b) == 0
        streams = [tu.text_stream(cfg, b, n) for b in range(B)]
        out = [s.step([streams[b][i] for b in range(B)]) for i in range(n)]
        s.free()
        return out
    ref, got = run("oracle"), run("hip")
    assert any(r[0] for r in ref)
    for i, (a, b) in enumerate(zip(ref, got)):
        assert a[0] == b[0] and (not a[0] or a == b), f"frame {i}: oracle {a} vs hip {b}"


def test_conditions_of_one_column_leave_a_live_neighbour_bit_identical():
    cfg = tiny_tts_slots(Q4_K, Q4_0)
    n, B = RING + 2, 3
    events = {0: [("open", 0), ("open", 1)], 2: [("open", 2)]}
    base = run_slots("hip", cfg, B, n, events)
    changed = run_slots("hip", cfg, B, n, events, recondition=(5, 1, 40))
    moved = False
    for i, (a, c) in enumerate(zip(base, changed)):
        for col in (0, 2):
            assert a[1][col] == c[1][col] and a[2][col] == c[2][col] and a[3][col] == c[3][col], (i, col)
            assert np.array_equal(a[4][col], c[4][col]) and np.array_equal(a[5][col], c[5][col]), (i, col)
        same = np.array_equal(a[5][1], c[5][1])
        assert same or i >= 5, i
        moved = moved or not same
    assert moved
