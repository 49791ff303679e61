"""-m gpu: stt-shaped B-column models on the MI355X (dep_q = 0, extra heads on transformer_out computed by the Temporal graph's tail).

Op level: the heads group {mul_mat -> soft_max -> cpy into a view of heads_out} x heads as ONE launch (heads_streams_kernel) against the oracle:
probabilities within 1e-4 absolute (the bar test_stt_shape_no_depth_graph_and_vad_head sets for the VAD value), every row sums to 1 within 1e-6.
The graphs are run through ggml_util.Graph, the class behind ggml_util.run_graph, because the result is read from the destination tensor: the
copies' own outputs are strided views, which run_graph's read-back does not take.

Model level (contractive tiny_stt, ring of 8): bars as tests/test_slots_gpu.py - tokens bit-exact against the oracle's slots model, text logits per
weight type in that module's statistical form, head probabilities of status-1 slots within 1e-4."""
import ctypes as C

import numpy as np
import pytest

import ggml_util as gu
import hot_util as hu
import slots_util as sl
import stt_slots_util as st
from ggml_util import BF16, F32, Q4_0, Q4_K, Q8_0
from test_slots_gpu import RING, TYPE_TOL, staggered_events

pytestmark = pytest.mark.gpu
L = hu.L
libc = C.CDLL(None)
HEADS_TOL = 1e-4
RANDOM_ROWS = {Q4_K: gu.random_q4_K, Q8_0: gu.random_q8_0, Q4_0: gu.random_q4_0}
X_SCALE = {Q4_K: 1.0 / 32, Q8_0: 0.25, Q4_0: 0.25, F32: 1.0}   # logits of order 1 under the synthetic rows of ggml_util (so that no row is one-hot)


def run_heads(kind, wt, K, nh, M, B, x_mul=1.0, seed=0):
    """-> (heads_out [B, nh, M], launches in the plan or None)"""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((B, 1, K)) * X_SCALE[wt] * x_mul).astype(np.float32)
    g = gu.Graph(kind)
    try:
        xt = g.input(x)
        dst = g.new(F32, M, nh, B)
        outs = []
        for k in range(nh):
            if wt == F32:
                w = g.input((rng.standard_normal((M, K)) / np.sqrt(K)).astype(np.float32))
            else:
                w = g.input_raw(RANDOM_ROWS[wt](rng, M, K), wt, K, M)
            sm = g.soft_max(g.mul_mat(w, xt))
            outs.append(g.cpy(sm, g.view_3d(dst, M, 1, B, M * 4, nh * M * 4, k * M * 4)))
        g.build(outs)
        g.alloc()
        g.set(dst, np.full((B, nh, M), -3.0, np.float32))
        g.compute()
        return g.get(dst).reshape(B, nh, M), (g.stats().kernels_in_last_plan if kind == "hip" else None)
    finally:
        g.free()


HEAD_CASES = [(wt, 512, 3, 6, B, 1.0) for wt in (Q4_K, Q8_0, Q4_0) for B in (2, 3, 16)] + [
    (Q4_K, 256, 1, 1, 2, 1.0),       # one block, one row: soft_max of one value = 1
    (Q4_K, 2048, 3, 16, 3, 1.0),     # the stt width, the M limit
    (Q4_K, 512, 3, 6, 3, 64.0),      # logits spread beyond expf's range unless the maximum is subtracted
]


@pytest.mark.parametrize("wt,K,nh,M,B,x_mul", HEAD_CASES)
def test_heads_group_is_one_launch_and_matches_oracle(wt, K, nh, M, B, x_mul):
    ref, _ = run_heads("oracle", wt, K, nh, M, B, x_mul)
    got, launches = run_heads("hip", wt, K, nh, M, B, x_mul)
    err = float(np.abs(ref - got).max())
    sums = float(np.abs(got.sum(axis=2) - 1.0).max())
    print(f"heads group type {wt} K {K} {nh} x {M} B {B} x * {x_mul}: max abs err {err:.2e}, |row sum - 1| {sums:.2e}, {launches} launch(es), "
          f"probabilities between {float(ref.min()):.2e} and {float(ref.max()):.3f}")
    assert np.all(np.isfinite(got)) and err < HEADS_TOL
    assert sums < 1e-6
    assert launches == 1
    if M == 1:
        assert np.all(got == 1.0)


def test_float_weight_heads_are_left_to_the_plain_nodes_and_still_match():
    ref, _ = run_heads("oracle", F32, 512, 3, 6, 3)
    got, launches = run_heads("hip", F32, 512, 3, 6, 3)
    assert float(np.abs(ref - got).max()) < HEADS_TOL and float(np.abs(got.sum(axis=2) - 1.0).max()) < 1e-6
    assert launches > 1


# ---- model level --------------------------------------------------------------------------------------------------------------------------------
def tiny_stt_slots(lt, et, contractive=True, heads=True):
    cfg = hu.hot.tiny_stt(L, linear_type=lt, embed_type=et, context=RING)
    if contractive:
        cfg.update_scale = 1.0 / 256
    if not heads:
        cfg.extra_heads = cfg.extra_heads_dim = 0
    return cfg


def run(kind, cfg, B, codes, events, srand=False):
    """-> per frame (n_valid, status, texts, audios, text_logits [B, text_card], heads [B, nh, hd])"""
    s = st.Slots(kind, cfg, B, seed=0)
    out = []
    for i, fr in enumerate(codes):
        for what, b in events.get(i, []):
            assert (s.open(b) if what == "open" else s.close(b)) == 0
        if srand:
            libc.srand(1000 + i)   # the sampler's exponential noise is drawn from rand() on the host: both executors see the same draws
        out.append(s.step(fr) + (s.read("text_logits", cfg.text_card), s.heads()))
    s.free()
    return out


def check_against_oracle(ref, got, B, tol, logits=True):
    errs, herrs = [], []
    for i, (a, b) in enumerate(zip(ref, got)):
        assert a[:4] == b[:4], f"frame {i}: tokens differ: oracle {a[:4]} vs hip {b[:4]}"
        for s in range(B):
            if a[1][s] != -1:
                errs.append(hu.rel_err(a[4][s], b[4][s]))
            if a[1][s] == 1:
                herrs.append(float(np.abs(a[5][s] - b[5][s]).max()))
                assert abs(float(b[5][s].sum(axis=1).max()) - 1.0) < 1e-5
            else:
                assert np.all(b[5][s] == -1) and np.all(a[5][s] == -1)
    assert any(r[0] > 0 for r in ref) and herrs
    errs, herrs = np.array(errs), np.array(herrs)
    print(f"text logit rel errors: median {np.median(errs):.2e} max {errs.max():.2e}; head probability errors: max {herrs.max():.2e}")
    assert herrs.max() < HEADS_TOL, f"head probability errors {np.sort(herrs)[-8:]}"
    if logits:
        assert np.median(errs) < min(tol, 1e-5), f"median logit error {np.median(errs):.2e}"
        assert np.mean(errs < tol) >= 0.9 and errs.max() < 0.1, f"logit errors over the bar {tol:.0e}: {np.sort(errs)[-8:]}"


@pytest.mark.parametrize("B", [3, 8])
@pytest.mark.parametrize("lt,et", [(Q4_K, Q4_0), (Q8_0, Q8_0), (BF16, BF16), (F32, F32)])
def test_staggered_and_reopened_stt_slots_match_oracle(lt, et, B):
    cfg = tiny_stt_slots(lt, et)
    n = 2 * RING + 2
    codes = sl.slot_codes(cfg, B, n, seed=B)
    events = staggered_events(B)
    check_against_oracle(run("oracle", cfg, B, codes, events), run("hip", cfg, B, codes, events), B, TYPE_TOL[lt])


def test_sampled_stt_slots_match_oracle_with_the_same_noise():
    cfg = tiny_stt_slots(Q4_K, Q4_0)
    cfg.temp, cfg.temp_text, cfg.top_k, cfg.top_k_text = 0.8, 0.7, 20, 25
    n = 2 * RING + 2
    codes = sl.slot_codes(cfg, 3, n, seed=9)
    events = staggered_events(3)
    ref = run("oracle", cfg, 3, codes, events, srand=True)
    got = run("hip", cfg, 3, codes, events, srand=True)
    for i, (a, b) in enumerate(zip(ref, got)):
        assert a[:4] == b[:4], f"frame {i}: sampled tokens differ: oracle {a[:4]} vs hip {b[:4]}"
    assert len({t for r in ref for t in r[2] if t >= 0}) > 1


@pytest.mark.parametrize("B", [3, 8])
def test_all_stt_slots_open_at_frame_zero_equal_device_lockstep(B):
    cfg = tiny_stt_slots(Q4_K, Q4_0, contractive=False)
    n = RING + 4
    codes = sl.slot_codes(cfg, B, n, seed=30 + B)
    a = st.Streams("hip", cfg, B)
    ref = []
    for fr in codes:
        ref.append(a.step(fr) + (a.read("text_logits", cfg.text_card), a.heads()))
    a.free()
    got = run("hip", cfg, B, codes, {0: [("open", b) for b in range(B)]})
    for k, (g, r) in enumerate(zip(got, ref)):
        assert g[1] == [r[0]] * B and r[0] == 1, k
        assert g[2] == r[1], k
        assert np.array_equal(g[4], r[3]) and np.array_equal(g[5], r[4]), k


def temporal_plan_launches(cfg, B):
    s = st.Slots("hip", cfg, B)
    codes = sl.slot_codes(cfg, B, 6, seed=2)
    for i, fr in enumerate(codes):
        if i < B - 2:
            s.open(i)
        s.step(fr)
    assert L.ggml_backend_graph_compute(s.be, L.moshi_hot_graph(s.m, 0)) == 0   # the Temporal graph once more on its own: its plan is the last one
    n = s.stats().kernels_in_last_plan
    s.free()
    return n


def test_heads_add_exactly_one_launch_to_the_temporal_plan():
    B = 8
    with_heads = temporal_plan_launches(tiny_stt_slots(Q4_K, Q4_0), B)
    without = temporal_plan_launches(tiny_stt_slots(Q4_K, Q4_0, heads=False), B)
    cfg = tiny_stt_slots(Q4_K, Q4_0)
    print(f"Temporal plan at B = {B}: {with_heads} launches with 3 heads, {without} without")
    assert with_heads == without + 1
    assert with_heads <= 6 * cfg.num_layers + 8 + 1


def test_prefill_and_snapshots_between_a_live_neighbours_frames_change_nothing_of_it():
    cfg = tiny_stt_slots(Q4_K, Q4_0)
    n = RING + 4
    live = st.codes(cfg, n, seed=61)
    other = st.codes(cfg, n, seed=62)
    hist = [[int(t)] + c for t, c in zip(np.random.default_rng(63).integers(0, cfg.text_card, 5), st.codes(cfg, 5, seed=64))]

    def neighbour(busy):
        s = st.Slots("hip", cfg, 3)
        assert s.open(0) == 0
        out = []
        for k in range(n):
            if busy and k == 2:
                assert s.open(1) == 0 and s.prefill([(1, hist)], 4) == 5
            if busy and k == 4:
                assert s.fork(1, 2) == 0
            if busy and k == 6:
                blob = s.save(2)
                assert blob is not None and s.close(2) == 0 and s.load(2, blob) == 0
            per = {0: live[k]}
            if busy and k >= 2:
                per[1] = other[k]
            if busy and k >= 4:
                per[2] = other[k]
            r = st.step_all(s, per)
            if busy and k >= 4:
                assert r[1][1] == r[1][2] and r[2][1] == r[2][2] and np.array_equal(r[4][1], r[4][2]) and np.array_equal(r[5][1], r[5][2]), k
            out.append(r)
        s.free()
        return out
    alone, beside = neighbour(False), neighbour(True)
    for k, (a, b) in enumerate(zip(alone, beside)):
        assert a[1][0] == b[1][0] == 1 and a[2][0] == b[2][0], k
        assert np.array_equal(a[4][0], b[4][0]) and np.array_equal(a[5][0], b[5][0]), k
