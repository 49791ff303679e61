"""CPU: stt-shaped B-column models (dep_q = 0: no Depth transformer, every codebook an input, extra heads on transformer_out) on the host device
with the oracle attached - lockstep streams, slots, seeded sampling, slot prefill and slot snapshots. hot.tiny_stt, ring of 24. Every conversation of
a B-column model equals, bit for bit, a single-stream stt model fed that conversation's codes with the VAD value requested: status, text token, text
logits and the VAD probability (head 2, element 0: all a single-stream step computes of the heads).

The full heads_out rows are compared with a float64 numpy soft_max of transformer_out times the heads' weights within 1e-6. That reference is the
oracle's arithmetic only where the oracle multiplies floats: the F32-weight model, where the check is asserted (measured: 4.4e-8 at most). With Q4_K
weights the oracle, as ggml, first rounds transformer_out to Q8_K blocks (a step of amax / 127 per value), which moves a head's logits by ~1e-2 and
its probabilities by up to 9.3e-3 (measured, printed by the test) - no implementation of ggml's Q4_K product can meet a float product to 1e-6, so on
those runs the rows are pinned through the bit-exact VAD value, their sums and the F32 run's numpy check instead."""
import ctypes as C
import functools

import numpy as np
import pytest

import hot_util as hu
import sampling_util as sp
import slot_prefill_util as pu
import streams_util as su
import stt_slots_util as st
from ggml_util import F32, Q4_K

L = hu.L
CONTEXT = 24
N = CONTEXT + 4                              # across the 24-row ring's wrap
SAMPLING = (4321, 0.9, 0.6, 12, 17)          # seed, temp, temp_text, top_k, top_k_text


def cfg_of(lt=Q4_K, text_delay=0, sampled=False):
    cfg = hu.hot.tiny_stt(L, linear_type=lt, embed_type=F32 if lt == F32 else 2, context=CONTEXT)
    cfg.delays[0] = text_delay
    return sp.sampled(cfg) if sampled else cfg


def conv(i, n=N):
    """conversation i's codes (n frames of n_q codes)"""
    return st.codes(cfg_of(), n, seed=500 + i)


@functools.lru_cache(maxsize=None)
def reference(i, lt=Q4_K, text_delay=0, n=N):
    """conversation i through a fresh single-stream stt model. Shared by the tests and never changed"""
    return st.single_reference("oracle", cfg_of(lt, text_delay), [], conv(i, n), seed=5)


def run_lockstep(cfg, B, n):
    s = st.Streams("oracle", cfg, B, seed=5)
    w = st.head_weights(s.m, cfg)
    out = []
    for k in range(n):
        ok, txt, aud = s.step([conv(b)[k] for b in range(B)])
        assert aud == [[]] * B
        out.append((ok, [ok] * B, txt, aud, s.read("text_logits", cfg.text_card), s.heads(), s.read("transformer_out", cfg.dim)))
    s.free()
    return out, w


@pytest.mark.parametrize("B", [2, 3])
@pytest.mark.parametrize("lt", [Q4_K, F32], ids=["q4_k", "f32"])
def test_lockstep_streams_equal_single_stream_models_heads_included(lt, B):
    cfg = cfg_of(lt)
    got, w = run_lockstep(cfg, B, N)
    for b in range(B):
        st.assert_column_equals_single(got, b, reference(b, lt), "lockstep")
    assert all(g[0] == 1 for g in got)
    worst = 0.0
    for g in got:
        for b in range(B):
            worst = max(worst, float(np.abs(g[5][b] - st.numpy_heads(w, g[6][b])).max()))
    print(f"heads_out against the float64 numpy soft_max, B = {B}, linear type {lt}: max abs difference {worst:.2e}")
    if lt == F32:
        assert worst < 1e-6, worst


def test_text_delay_gives_the_delay_rings_a_filling_phase_with_minus_one_head_rows():
    cfg = cfg_of(text_delay=2)
    n = 8
    s = st.Streams("oracle", cfg, 2, seed=5)
    got = []
    for k in range(n):
        ok, txt, aud = s.step([conv(b)[k] for b in range(2)])
        got.append((ok, [ok] * 2, txt, aud, s.read("text_logits", cfg.text_card), s.heads()))
    s.free()
    for b in range(2):
        st.assert_column_equals_single(got, b, reference(b, Q4_K, 2, n), "text delay")
    assert [g[0] for g in got] == [0, 0] + [1] * (n - 2)
    assert np.all(got[0][5] == -1) and np.all(got[1][5] == -1) and np.all(got[2][5] >= 0)


def test_slots_staggered_closed_reopened_and_held_equal_their_single_stream_models():
    # conversations 0 / 1 / 2 open at frames 0 / 2 / 5; slot 1 is closed at frame 10 and reopened at 12 with conversation 3; slot 2 is held for frames
    # 8 and 9. A text delay of 2 gives every conversation a filling phase: closed, held and filling slots all report -1 rows
    cfg = cfg_of(text_delay=2)
    s = st.Slots("oracle", cfg, 3, seed=5)
    start = {0: 0, 1: 2, 2: 5}
    seen = {0: [], 1: [], 2: [], 3: []}      # per conversation: the step_all results of its frames
    who = {}                                  # slot -> (conversation, frames stepped)
    for k in range(N):
        for b, f in start.items():
            if f == k:
                assert s.open(b) == 0
                who[b] = [b, 0]
        if k == 10:
            assert s.close(1) == 0
            del who[1]
        if k == 12:
            assert s.open(1) == 0
            who[1] = [3, 0]
        if k == 8:
            assert s.hold(2, True) == 0
        if k == 10:
            assert s.hold(2, False) == 0
        held = {2} if k in (8, 9) else set()
        r = st.step_all(s, {b: conv(c)[i] for b, (c, i) in who.items() if b not in held})
        for b in range(3):
            if b not in who:
                assert r[1][b] == -1 and r[2][b] == -1 and np.all(r[5][b] == -1), (k, b)
            elif b in held:
                assert r[1][b] == -2 and r[2][b] == -1 and np.all(r[5][b] == -1), (k, b)
            else:
                seen[who[b][0]].append(r)
                who[b][1] += 1
    s.free()
    slot_of = {0: 0, 1: 1, 2: 2, 3: 1}
    for c, frames in seen.items():
        assert len(frames) >= 8
        st.assert_column_equals_single(frames, slot_of[c], reference(c, Q4_K, 2)[:len(frames)], f"conversation {c}")
        assert [f[1][slot_of[c]] for f in frames[:3]] == [0, 0, 1]


def test_seeded_conversation_gets_the_same_tokens_in_any_column_and_single_stream():
    cfg = cfg_of(sampled=True)
    n = 12
    ref = st.single_reference("oracle", cfg_of(), [], conv(0, n), sampling=SAMPLING, seed=5)
    a = st.Streams("oracle", cfg, 2, seed=5)
    assert a.set_sampling(0, *SAMPLING) == 0
    b = st.Slots("oracle", cfg, 3, seed=5)
    assert b.set_sampling(2, *SAMPLING) == 0
    for c in range(3):
        assert b.open(c) == 0
    for k in range(n):
        ra = a.step([conv(0)[k], conv(1)[k]])
        rb = b.step([conv(2)[k], conv(3)[k], conv(0)[k]])
        assert ra[0] in (0, 1) and rb[1][2] == 1
        assert ra[1][0] == rb[2][2] == ref[k][1], (k, ra[1], rb[2], ref[k][1])
        assert np.array_equal(a.read("text_logits", cfg.text_card)[0], ref[k][3]) and np.array_equal(b.read("text_logits", cfg.text_card)[2], ref[k][3])
        assert b.heads()[2, 2, 0] == np.float32(ref[k][4])
    a.free(); b.free()
    greedy = [r[1] for r in reference(0)[:n]]
    assert [r[1] for r in ref] != greedy     # the sampler did sample


@pytest.mark.parametrize("chunk", [4, 64])
def test_prefilled_slot_equals_single_stream_model_after_prefill(chunk):
    cfg = cfg_of()
    hist = pu.history(cfg, 10, seed=31)
    live = conv(4, 6)
    ref = st.single_reference("oracle", cfg, hist, live, seed=5, chunk=chunk)
    s = st.Slots("oracle", cfg, 3, seed=5)
    assert s.open(0) == 0 and s.open(1) == 0
    st.step_all(s, {0: conv(0)[0]})          # (slot 1 steps one frame on zeros, then is reopened for the history)
    assert s.close(1) == 0 and s.open(1) == 0
    assert s.prefill([(1, hist)], chunk) == 10 and s.position(1) == 10
    got = [st.step_all(s, {0: conv(0)[1 + k], 1: live[k]}) for k in range(6)]
    s.free()
    st.assert_column_equals_single(got, 1, ref, f"prefilled, chunk {chunk}")
    st.assert_column_equals_single(got, 0, reference(0)[1:7], "live neighbour")


def test_forked_and_saved_slots_continue_bit_for_bit():
    cfg = cfg_of()
    A = conv(5, CONTEXT + 3 + 4)
    ref = st.single_reference("oracle", cfg, [], A, seed=5)
    s = st.Slots("oracle", cfg, 3, seed=5)
    assert s.open(0) == 0
    before = [st.step_all(s, {0: A[k]}) for k in range(5)]
    assert s.fork(0, 2) == 0 and s.position(2) == 5
    mid = [st.step_all(s, {0: A[k], 2: A[k]}) for k in range(5, CONTEXT + 3)]
    blob = s.save(2)
    assert blob is not None and s.position(2) == CONTEXT + 3
    t = st.Slots("oracle", cfg, 2, seed=5)
    assert t.load(1, blob) == 0 and t.position(1) == CONTEXT + 3
    tail_s = [st.step_all(s, {0: A[k], 2: A[k]}) for k in range(CONTEXT + 3, len(A))]
    tail_t = [st.step_all(t, {1: A[k]}) for k in range(CONTEXT + 3, len(A))]
    st.assert_column_equals_single(before + mid + tail_s, 0, ref, "source")
    st.assert_column_equals_single(mid + tail_s, 2, ref[5:], "fork")
    st.assert_column_equals_single(tail_t, 1, ref[CONTEXT + 3:], "loaded")
    # a moshika-shaped blob does not load into an stt model, nor the reverse (the fingerprint carries n_q and dep_q)
    mk = su.lm_only(hu.hot.tiny(L, context=CONTEXT))
    import slot_state_util as ss
    m = ss.Slots("oracle", mk, 2, seed=5)
    assert m.open(0) == 0
    ss.step_all(m, {0: [0] * (mk.n_q - mk.dep_q)})
    mblob = m.save(0)
    assert m.load(1, blob) == -1 and t.load(0, mblob) == -1
    assert m.position(1) == -1 and t.position(0) == -1
    m.free(); s.free(); t.free()


def _created(cfg, n, fn="moshi_hot_create_slots"):
    be = hu.make_backend("oracle")
    m = getattr(L, fn)(be, C.byref(cfg), 0, n)
    if m:
        L.moshi_hot_free(m)
    L.ggml_backend_free(be)
    return bool(m)


def test_refusals():
    for fn in ("moshi_hot_create_slots", "moshi_hot_create_streams"):
        assert _created(cfg_of(), 2, fn) and _created(cfg_of(), 16, fn)
        assert not _created(cfg_of(), 17, fn)
        for hd in (17, 0):
            c = cfg_of(); c.extra_heads_dim = hd
            assert not _created(c, 2, fn), hd
        c = cfg_of(); c.extra_heads = 0; c.extra_heads_dim = 0
        assert _created(c, 2, fn)                       # the stt shape without heads
        for half in ("enable_mimi_encoder", "enable_mimi_decoder"):
            c = cfg_of(); setattr(c, half, 1)
            assert not _created(c, 2, fn), half
        c = su.lm_only(hu.hot.tiny(L, layers=1)); c.extra_heads, c.extra_heads_dim = 3, 6
        assert not _created(c, 2, fn)                   # heads on a model with a Depth transformer
    buf = np.zeros(3 * 3 * 6, np.float32)
    m = hu.Model("oracle", cfg_of())
    assert L.moshi_hot_last_heads(m.m, buf.ctypes.data, buf.size) == -1
    m.free()
    s = su.Streams("oracle", su.lm_only(hu.hot.tiny(L, layers=1)), 2)
    assert L.moshi_hot_last_heads(s.m, buf.ctypes.data, buf.size) == -1
    s.free()
    s = st.Slots("oracle", cfg_of(), 3)
    assert L.moshi_hot_last_heads(s.m, buf.ctypes.data, buf.size - 1) == -1 and L.moshi_hot_last_heads(s.m, None, buf.size) == -1
    assert L.moshi_hot_last_heads(s.m, buf.ctypes.data, buf.size) == buf.size and np.all(buf == -1)   # nothing stepped yet
    s.free()
