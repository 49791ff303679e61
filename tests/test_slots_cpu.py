"""CPU: stream slots (moshi_hot_create_slots) on the host device with the oracle attached - conversations admitted and retired mid-batch, each at a
stream position of its own, give every conversation exactly what a fresh single-stream model gives it, across the Temporal ring's wrap and across
reuse of a slot's ring rows by a new conversation."""
import ctypes as C

import numpy as np
import pytest

import hot_util as hu
import slots_util as sl
import streams_util as su


def check_conversations(cfg, codes, got, events, seed):
    """every conversation of `events` against a fresh single-stream oracle model fed that conversation's codes from its own first frame"""
    n = len(codes)
    spans = sl.conversations(events, n)
    open_at = {}
    for b, convs in spans.items():
        for s, e in convs:
            ref = su.run_single("oracle", cfg, [codes[k][b] for k in range(s, e)], seed=seed, logits=True)
            for k in range(s, e):
                g, r = got[k], ref[k - s]
                assert g[1][b] == r[0], (b, s, k)
                if r[0]:
                    assert g[2][b] == r[1] and g[3][b] == r[2], (b, s, k)
                else:
                    assert g[2][b] == -1 and g[3][b] == [-1] * cfg.dep_q, (b, s, k)
                # the oracle computes every column on its own: slot b's logits are the single-stream model's, bit for bit
                assert np.array_equal(g[4][b], r[3]), (b, s, k)
                open_at.setdefault(k, set()).add(b)
    for k, g in enumerate(got):
        live = open_at.get(k, set())
        assert g[0] == sum(1 for b in live if g[1][b] == 1), k
        for b in range(len(g[1])):
            if b not in live:
                assert g[1][b] == -1 and g[2][b] == -1 and g[3][b] == [-1] * cfg.dep_q, (b, k)
    return spans


def test_staggered_opens_equal_fresh_single_stream_models():
    cfg = su.lm_only(hu.hot.tiny(hu.L))
    n = cfg.context + 8                                     # every conversation but the last runs past the 24-slot ring's wrap
    B = 4                                                   # slot 3 stays closed throughout
    codes = sl.slot_codes(cfg, B, n, seed=11)
    events = {0: [("open", 0)], 5: [("open", 1)], 11: [("open", 2)]}
    s = sl.Slots("oracle", cfg, B, seed=5)
    got = sl.run_slots(s, codes, events, logits=True)
    s.free()
    check_conversations(cfg, codes, got, events, seed=5)
    # the conversations really differ: not copies of one another
    assert len({tuple(g[2][:3]) for g in got[-4:]}) > 1 or any(len(set(g[2][:3])) > 1 for g in got[-4:])


def test_reopened_slots_see_nothing_of_the_previous_conversation():
    cfg = su.lm_only(hu.hot.tiny(hu.L))
    C_ = cfg.context
    n = C_ + 16
    # slot 0: one conversation past the ring's wrap, then a new one in the same slot; slot 1: a short conversation (ring never filled), closed for
    # three frames, then a new one
    events = {0: [("open", 0)], 2: [("open", 1)], 9: [("close", 1)], 12: [("open", 1)], C_ + 4: [("close", 0), ("open", 0)]}
    codes = sl.slot_codes(cfg, 2, n, seed=13)
    s = sl.Slots("oracle", cfg, 2, seed=3)
    got = sl.run_slots(s, codes, events, logits=True)
    s.free()
    spans = check_conversations(cfg, codes, got, events, seed=3)
    assert spans == {0: [(0, C_ + 4), (C_ + 4, n)], 1: [(2, 9), (12, n)]}


def test_closed_slots_report_nothing_and_positions_count_frames():
    cfg = su.lm_only(hu.hot.tiny(hu.L, layers=1))
    s = sl.Slots("oracle", cfg, 3)
    codes = sl.slot_codes(cfg, 3, 4, seed=1)
    assert [s.position(b) for b in range(3)] == [-1, -1, -1]
    r, st, txt, aud = s.step(codes[0])                     # no slot open: no device work
    assert r == 0 and st == [-1, -1, -1] and txt == [-1, -1, -1] and aud == [[-1] * cfg.dep_q] * 3
    assert s.open(1) == 0 and s.position(1) == 0
    for k in range(3):
        r, st, txt, aud = s.step(codes[k + 1])
        assert st[0] == st[2] == -1 and txt[0] == txt[2] == -1 and aud[0] == aud[2] == [-1] * cfg.dep_q
        assert st[1] in (0, 1) and r == (st[1] == 1)
        assert s.position(1) == k + 1 and s.position(0) == -1 and s.position(2) == -1
    s.set_fill(1, 100)
    assert s.position(1) == 100
    assert s.close(1) == 0 and s.position(1) == -1
    r, st, _, _ = s.step(codes[0])
    assert r == 0 and st == [-1, -1, -1]
    assert s.open(1) == 0 and s.position(1) == 0          # a reopened slot starts over
    s.free()


@pytest.mark.parametrize("B", [2, 3])
def test_all_slots_open_at_frame_zero_equal_lockstep_streams(B):
    cfg = su.lm_only(hu.hot.tiny(hu.L))
    n = cfg.context + 4
    codes = sl.slot_codes(cfg, B, n, seed=7 + B)
    ref = su.run_streams("oracle", cfg, codes, seed=9, logits=True)
    s = sl.Slots("oracle", cfg, B, seed=9)
    got = sl.run_slots(s, codes, {0: [("open", b) for b in range(B)]}, logits=True)
    s.free()
    for k, (g, r) in enumerate(zip(got, ref)):
        assert g[0] == (B if r[0] == 1 else 0) and g[1] == [r[0]] * B, k
        if r[0]:
            assert g[2] == r[1] and g[3] == r[2], k
        assert np.array_equal(g[4], r[3]), k


def _created(cfg, n):
    be = hu.make_backend("oracle")
    m = hu.L.moshi_hot_create_slots(be, C.byref(cfg), 0, n)
    if m:
        hu.L.moshi_hot_free(m)
    hu.L.ggml_backend_free(be)
    return bool(m)


def test_create_slots_refuses_what_create_streams_refuses():
    base = lambda: su.lm_only(hu.hot.tiny(hu.L, layers=1))
    assert _created(base(), 2) and _created(base(), 16)
    assert not _created(base(), 1) and not _created(base(), 17) and not _created(base(), 0)
    pp = hu.hot.tiny_personaplex(hu.L, layers=1)
    pp.enable_mimi_encoder = pp.enable_mimi_decoder = 0
    assert not _created(pp, 2)
    tp = base(); tp.tp_world = 1
    assert not _created(tp, 2)
    assert not _created(hu.hot.tiny(hu.L, layers=1), 2)     # codec halves on
    for field in ("chain_depth", "delay_steps", "extra_heads", "codec_stream"):
        c = base(); setattr(c, field, 1)
        assert not _created(c, 3), field


def test_slot_calls_and_step_calls_refuse_the_other_kinds():
    cfg = su.lm_only(hu.hot.tiny(hu.L, layers=1))
    s = sl.Slots("oracle", cfg, 2)
    for b in (-1, 2, 99):
        assert s.open(b) == -1 and s.close(b) == -1 and s.position(b) == -1
    ia = (C.c_int32 * 64)()
    out = (C.c_int32 * 64)()
    assert hu.L.moshi_hot_lm_step(s.m, ia, out, out) == -1
    assert hu.L.moshi_hot_lm_step_streams(s.m, ia, out, out) == -1
    assert hu.L.moshi_hot_ring_bytes(s.m, 0, 0, 0, None, 0, 0) == -1
    assert hu.L.moshi_hot_host_ring(s.m, None, 0) == -1
    assert hu.L.moshi_hot_n_streams(s.m) == 2
    s.free()
    st = su.Streams("oracle", cfg, 2)
    assert hu.L.moshi_hot_slot_open(st.m, 0) == -1 and hu.L.moshi_hot_slot_close(st.m, 0) == -1
    assert hu.L.moshi_hot_slot_position(st.m, 0) == -1
    assert hu.L.moshi_hot_lm_step_slots(st.m, ia, out, out, out) == -1
    st.free()
    m = hu.Model("oracle", cfg)
    assert hu.L.moshi_hot_slot_open(m.m, 0) == -1
    assert hu.L.moshi_hot_lm_step_slots(m.m, ia, out, out, out) == -1
    m.free()
