"""CPU (oracle backend): Q8_0 K / V rings for streams and slots, moshi_hot_config::kv_q8 (include/moshi_hot.h), on a tiny model with an
8-slot ring: a conversation gets the lockstep kv_q8 model's numbers in any slot beside any neighbours, the rings are 136 / 256 of the BF16 model's bytes,
the creators and calls that do not take such a model refuse it and change nothing, and kv_q8 = 0 is the BF16 model it was."""
import ctypes as C

import numpy as np

import codec_slots_util as cu
import encoder_slots_util as eu
import hot_util as hu
import persona_util as pu
import slots_util as sl
import streams_util as su

L = hu.L
RING, FRAMES = 8, 12   # across the ring's wrap


def tiny(kv_q8=1, **kw):
    cfg = su.lm_only(hu.hot.tiny(L, context=RING, **kw))
    cfg.kv_q8 = kv_q8
    return cfg


def slot_run(cfg, B, slot, conv, first, seed, disturb=None):
    """`conv` in `slot` of a B-slot model from frame `first`, every other slot open from frame 0 on codes of `seed` -> the slot's text logits per frame"""
    others = sl.slot_codes(cfg, B, first + len(conv), seed=seed)
    s = sl.Slots("oracle", cfg, B)
    for b in range(B):
        if b != slot:
            assert s.open(b) == 0
    out = []
    for k in range(first + len(conv)):
        if k == first:
            assert s.open(slot) == 0
        if disturb and k == first + 3:
            disturb(s, slot)
        codes = [list(c) for c in others[k]]
        if k >= first:
            codes[slot] = list(conv[k - first])
        s.step(codes)
        if k >= first:
            out.append(s.read("text_logits", cfg.text_card)[slot].copy())
    s.free()
    return out


def refused_calls(s, b):
    """every call a kv_q8 slots model refuses, on open slot b: -1, and the slot stays where it was"""
    pos = s.position(b)
    toks = np.zeros((2, s.cfg.n_q + 1), np.int32)
    slots, n = (C.c_int32 * 1)(b), (C.c_int32 * 1)(2)
    rows = (C.c_void_p * 1)(toks.ctypes.data)
    persona = hu.hot.Persona()
    buf = np.zeros(1 << 16, np.uint8)
    free_slot = (b + 1) % s.B
    assert s.close(free_slot) == 0
    for name in ("moshi_hot_slots_prefill", "moshi_hot_slots_prefill_long", "moshi_hot_slots_replay"):
        assert getattr(L, name)(s.m, 1, slots, rows, n, 2) == -1, name
    assert L.moshi_hot_slots_persona(s.m, 1, slots, C.byref(persona), 2) == -1
    for full in ("", "_full"):
        assert getattr(L, "moshi_hot_slot_fork" + full)(s.m, b, free_slot) == -1
        assert getattr(L, "moshi_hot_slot_save" + full)(s.m, b, buf.ctypes.data, buf.nbytes) == -1
        assert getattr(L, "moshi_hot_slot_load" + full)(s.m, free_slot, buf.ctypes.data, buf.nbytes) == -1
    assert s.position(b) == pos
    assert s.open(free_slot) == 0   # (the neighbour starts a new conversation: not refused, and nothing the slot's own numbers depend on)


def test_a_conversation_gets_the_lockstep_numbers_in_any_slot_and_refused_calls_change_nothing():
    cfg = tiny()
    codes = su.stream_codes(cfg, 2, FRAMES, seed=5)
    lock = [r[3][0] for r in su.run_streams("oracle", cfg, codes, logits=True)]
    conv = [fr[0] for fr in codes]
    a = slot_run(cfg, 3, 2, conv, first=3, seed=1)
    b = slot_run(cfg, 2, 0, conv, first=1, seed=2, disturb=refused_calls)
    off = [r[3][0] for r in su.run_streams("oracle", tiny(kv_q8=0), codes, logits=True)]
    assert np.isfinite(lock).all() and not np.array_equal(lock[-1], off[-1])      # the option changes the numbers it is meant to change
    for k in range(FRAMES):
        assert np.array_equal(a[k], lock[k]) and np.array_equal(b[k], lock[k]), f"frame {k}"


def test_ring_bytes_and_refused_creators():
    q8, bf = sl.Slots("oracle", tiny(), 3), sl.Slots("oracle", tiny(kv_q8=0), 3)
    cfg = q8.cfg
    assert L.moshi_hot_kv_bytes(bf.m) == 2 * cfg.num_layers * cfg.dim * RING * 3 * 2
    assert L.moshi_hot_kv_bytes(q8.m) * 256 == L.moshi_hot_kv_bytes(bf.m) * 136
    q8.free()
    bf.free()
    be = hu.make_backend("oracle")
    lm = tiny()
    assert not L.moshi_hot_create(be, C.byref(lm), 0) and not L.moshi_hot_create_streams(be, C.byref(lm), 0, 1)
    narrow = tiny()
    narrow.num_heads = 32                                                          # head rows of 16 values: no whole Q8_0 block
    assert not L.moshi_hot_create_slots(be, C.byref(narrow), 0, 2) and not L.moshi_hot_create_streams(be, C.byref(narrow), 0, 2)
    persona = pu.make_cfg()
    persona.kv_q8 = 1
    assert not L.moshi_hot_create_slots(be, C.byref(persona), 0, 2)
    for create, codec in ((L.moshi_hot_create_codec_slots, cu.cfg_of()), (L.moshi_hot_create_encoder_slots, eu.cfg_of())):
        codec.kv_q8 = 1
        assert not create(be, C.byref(codec), 0, 2)
    L.ggml_backend_free(be)
