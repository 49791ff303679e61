"""CPU (oracle): snapshots of tts-shaped slots that carry the conversation's conditions. moshi_hot_slot_fork_full copies a slot with its cond_sum /
cond_cross columns and its column of every layer's cross-attention K / V; moshi_hot_slot_save_full / _load_full move it through a version-2 blob
that holds the conditions (load recomputes K / V from them). The copy continues bit for bit, the source and the neighbours are untouched, the
destination's earlier conditions are gone. On a model that is not tts-shaped the _full calls are the plain ones; the plain ones still refuse tts."""
import struct

import numpy as np
import pytest

import ggml_util as gu
import hot_util as hu
import slot_state_util as ss
import streams_util as su
import tts_replay_util as ru
import tts_slots_util as tu

L = hu.L
SEED = 5
KEEP = tu.KEEP
AFTER = 5                  # live frames after a snapshot


def cfg_of(context=24, cross_len=5):
    cfg = tu.tts_cfg(linear_type=gu.F32, embed_type=gu.F32, layers=1, cross_len=cross_len)
    cfg.context = context
    return cfg


def reference(cfg, cond_seed, text_b, n):
    return ru.single_reference("oracle", cfg, cond_seed, tu.text_stream(cfg, text_b, n), seed=SEED)[0]


def advance(s, cfg, per_slot, first, n):
    """n live frames from frame `first` of every listed slot's text stream: per_slot = {slot: text stream}"""
    out = []
    for i in range(first, first + n):
        text_in = [KEEP] * s.B
        for b, texts in per_slot.items():
            text_in[b] = texts[i]
        out.append(ru.step(s, text_in, i >= cfg.delay_steps))
    return out


@pytest.mark.parametrize("pos,context", [(0, 24), (5, 24), (11, 8)], ids=["at-0", "at-5", "past-the-ring"])
def test_fork_full(pos, context):
    cfg = cfg_of(context)
    n = pos + AFTER
    t0, t2 = tu.text_stream(cfg, 0, n), tu.text_stream(cfg, 2, n)
    s = ru.Slots("oracle", cfg, 3, seed=SEED)
    assert s.set_conditions(0, 4) == 0 and s.set_conditions(1, 9) == 0 and s.set_conditions(2, 6) == 0      # slot 1: conditions of an earlier conversation
    assert s.open(0) == 0 and s.open(2) == 0
    before = advance(s, cfg, {0: t0, 2: t2}, 0, pos)
    assert s.fork(0, 1) == -1 and s.position(1) == -1          # the plain call still refuses the shape
    assert s.fork_full(0, 1) == 0 and s.position(1) == pos and s.position(0) == pos
    assert s.fork_full(0, 1) == -1 and s.fork_full(0, 0) == -1 and s.fork_full(3, 1) == -1      # dst open, src == dst, a bad index
    after = advance(s, cfg, {0: t0, 1: t0, 2: t2}, pos, AFTER)
    s.free()
    ref0, ref2 = reference(cfg, 4, 0, n), reference(cfg, 6, 2, n)
    tu.assert_column_equals_single(ru.column(before + after, 0), 0, ref0, "the source is unchanged")
    tu.assert_column_equals_single(ru.column(before + after, 2), 2, ref2, "the neighbour is untouched")
    tu.assert_column_equals_single(ru.column(after, 1), 1, ref0[pos:], "the copy runs the source's conversation, with the source's conditions")
    assert any(f[1][1] == 1 for f in after)


def saved(cfg, B, b, cond, text_b, pos):
    """-> (blob of slot b of a B-slot model after pos live frames of conversation (cond, text_b), the blob's size at every position)"""
    s = ru.Slots("oracle", cfg, B, seed=SEED)
    assert s.set_conditions(b, cond) == 0 and s.open(b) == 0
    sizes = [s.save_full_size(b)]
    texts = tu.text_stream(cfg, text_b, pos)
    for i in range(pos):
        advance(s, cfg, {b: texts}, i, 1)
        sizes.append(s.save_full_size(b))
    assert s.save_size(b) == -1 and s.save(b) is None          # the plain call still refuses the shape
    blob = s.save_full(b)
    assert L.moshi_hot_slot_save_full(s.m, b, blob.ctypes.data, blob.nbytes - 1) == -1
    s.free()
    return blob, sizes


@pytest.mark.parametrize("pos,context", [(5, 24), (11, 8)], ids=["at-5", "past-the-ring"])
def test_save_full_into_load_full(pos, context):
    cfg = cfg_of(context)
    n = pos + AFTER
    blob, sizes = saved(cfg, 2, 1, 4, 0, pos)
    assert blob.nbytes == sizes[-1]
    # the size grows with the position until the ring is full: by the K / V rows alone
    for p in range(pos):
        assert sizes[p + 1] - sizes[p] == ss.ring_bytes(cfg, p + 1) - ss.ring_bytes(cfg, p), p
    conds = cfg.dim * 4 + cfg.dim * cfg.cross_len * 4
    host = sizes[0]
    assert host % 16 == 0 and host >= 88 + conds + cfg.dim * 4
    magic, version = struct.unpack_from("<II", blob.tobytes(), 0)
    assert version == 2
    ref0, ref2 = reference(cfg, 4, 0, n), reference(cfg, 6, 2, n)
    t0, t2 = tu.text_stream(cfg, 0, n), tu.text_stream(cfg, 2, n)
    for B, dst in ((2, 0), (4, 3)):          # another column of a model like the saving one, and a model of another B
        s = ru.Slots("oracle", cfg, B, seed=SEED)
        other = 1 if dst != 1 else 0
        assert s.set_conditions(dst, 9) == 0 and s.set_conditions(other, 6) == 0 and s.open(other) == 0
        before = advance(s, cfg, {other: t2}, 0, pos)
        assert s.load(dst, blob) == -1 and s.position(dst) == -1                   # the plain call still refuses the shape
        assert s.load_full(other, blob) == -1                                      # an open slot
        assert s.load_full(dst, blob) == 0 and s.position(dst) == pos
        after = advance(s, cfg, {dst: t0, other: t2}, pos, AFTER)
        s.free()
        tu.assert_column_equals_single(ru.column(after, dst), dst, ref0[pos:], f"loaded into slot {dst} of {B}")
        tu.assert_column_equals_single(ru.column(before + after, other), other, ref2, "the neighbour is untouched")


def moshika_cfg():
    return su.lm_only(hu.hot.tiny(L, layers=1))


def test_bad_blobs_are_refused_and_change_nothing():
    cfg = cfg_of()
    pos, n = 4, 4 + AFTER
    blob, _ = saved(cfg, 2, 0, 4, 0, pos)
    v1 = blob.copy()
    v1[4:8] = np.frombuffer(struct.pack("<I", 1), np.uint8)
    wrong_len, _ = saved(cfg_of(cross_len=6), 2, 0, 4, 0, pos)
    mk = ss.Slots("oracle", moshika_cfg(), 2)
    assert mk.open(0) == 0
    mk.step([[1, 2, 3], [0, 0, 0]])
    moshika = mk.save(0)
    # the _full calls on a model without the tts shape are the plain calls: the same bytes
    n_full = L.moshi_hot_slot_save_full(mk.m, 0, None, 0)
    full = np.full(n_full, 0x5A, np.uint8)
    assert n_full == moshika.nbytes and L.moshi_hot_slot_save_full(mk.m, 0, full.ctypes.data, n_full) == n_full
    assert np.array_equal(full, moshika) and struct.unpack_from("<II", full.tobytes(), 0)[1] == 1
    assert L.moshi_hot_slot_load_full(mk.m, 1, blob.ctypes.data, blob.nbytes) == -1 and mk.position(1) == -1      # a tts blob into a moshika model
    assert L.moshi_hot_slot_load_full(mk.m, 1, full.ctypes.data, n_full) == 0 and mk.position(1) == 1
    assert mk.close(1) == 0 and L.moshi_hot_slot_fork_full(mk.m, 0, 1) == 0 and mk.position(1) == 1
    mk.free()

    s = ru.Slots("oracle", cfg, 2, seed=SEED)
    t1 = tu.text_stream(cfg, 1, n)
    assert s.set_conditions(0, 9) == 0 and s.set_conditions(1, 6) == 0 and s.open(1) == 0
    before = advance(s, cfg, {1: t1}, 0, pos)
    big = np.concatenate([blob, np.zeros(16, np.uint8)])
    assert s.load_full(0, blob[:-16]) == -1 and s.load_full(0, blob, blob.nbytes - 1) == -1       # truncated
    assert s.load_full(0, blob[:40]) == -1
    assert s.load_full(0, big) == -1                                                              # oversized
    assert s.load_full(0, v1) == -1 and s.load_full(0, moshika) == -1 and s.load_full(0, wrong_len) == -1
    assert s.position(0) == -1
    # nothing changed: slot 0 still holds the conditions it was given (a fresh conversation there is that conversation), its neighbour runs on
    assert s.open(0) == 0
    t0 = tu.text_stream(cfg, 0, AFTER)
    after = []
    for k in range(AFTER):
        after.append(ru.step(s, [t0[k], t1[pos + k]], True))
    s.free()
    ref1 = reference(cfg, 6, 1, n)
    tu.assert_column_equals_single(ru.column(before + after, 1), 1, ref1, "the neighbour of refused loads")
    ref0 = reference(cfg, 9, 0, AFTER)
    tu.assert_column_equals_single(ru.column(after, 0), 0, ref0, "the slot the loads were refused on")
