"""CPU: codec slot snapshots (moshi_hot_codec_slot_fork / _save / _load) on the host device with the oracle attached, at Mimi's own size, for the
decoder and for the encoder. Everything is compared bit for bit (PCM, or codes and both projected latents) against a fresh single-stream codec-only
model fed the whole history. The destination column is always dirty: another conversation ran through it for two frames before the fork or load."""
import ctypes as C
import functools

import numpy as np
import pytest

import codec_slot_state_util as cs
import hot_util as hu

L = hu.L
SEED = 3
N = 8                            # every input sequence is cut from the same N frames of its seed
A, X = 900, 902                  # seeds of the conversation and of the input a branch is fed instead
halves = pytest.mark.parametrize("half", cs.HALVES, ids=repr)


@functools.lru_cache(maxsize=None)
def reference(name, parts, fill=0):
    """parts: ((seed, first, n), ...) - the concatenated frames through a fresh single-stream model. Computed once per key and never changed"""
    half = next(h for h in cs.HALVES if h.name == name)
    frames = np.concatenate([half.frames(seed, N)[first:first + n] for seed, first, n in parts])
    return half.reference("oracle", frames, seed=SEED, fill=fill)


@halves
@pytest.mark.parametrize("pos", [1, 3])
def test_fork_continues_like_the_source_and_branches_on_other_input(half, pos):
    s = half.make("oracle", 3, seed=SEED)
    cs.dirty(half, s, 2)
    a, x = half.frames(A, N), half.frames(X, N)
    assert s.open(0) == 0
    cs.run(half, s, 0, a[:pos])
    assert cs.fork(s, 0, 2) == 0 and s.position(2) == pos == s.position(0)
    ref_a, ref_x = reference(half.name, ((A, 0, 7),)), reference(half.name, ((A, 0, pos + 2), (X, 0, 2)))
    for k in range(2):                                               # the same input: the same output, the reference's
        got = half.step(s, {0: a[pos + k], 2: a[pos + k]})
        assert cs.same(got[0], got[2]) and cs.same(got[0], ref_a[pos + k]), k
    for k in range(2):                                               # different input: each its own reference
        got = half.step(s, {0: a[pos + 2 + k], 2: x[k]})
        assert cs.same(got[0], ref_a[pos + 2 + k]) and cs.same(got[2], ref_x[pos + 2 + k]), k
        assert not cs.same(got[0], got[2])
    s.free()


@halves
@pytest.mark.parametrize("pos,fill", [(1, 0), (3, 0), (3, 123)], ids=["pos1", "pos3", "wrapped"])
def test_saved_slot_continues_in_another_column_of_another_model(half, pos, fill):
    s = half.make("oracle", 2, seed=SEED)
    a = half.frames(A, N)
    assert s.open(1) == 0
    if fill:
        s.set_fill(1, fill)                                          # rows 246 .. 251: the ring wraps at frame 125
    cs.run(half, s, 1, a[:pos])
    blob = cs.save(s, 1)
    assert s.position(1) == fill + pos
    s.free()
    h = cs.header(blob)
    assert h["pos"] == fill + pos and h["n"] == min(cs.ROWS_PER_FRAME * (fill + pos), cs.CAPACITY) and h["kind"] == half.kind_id
    t = half.make("oracle", 3, seed=SEED)
    cs.dirty(half, t, 2)
    assert cs.load(t, 2, blob) == 0 and t.position(2) == fill + pos
    got = cs.run(half, t, 2, a[pos:pos + 2])
    t.free()
    ref = reference(half.name, ((A, 0, 7),), fill) if not fill else reference(half.name, ((A, 0, 5),), fill)
    for k in range(2):
        assert cs.same(got[k], ref[pos + k]), k


@halves
def test_blob_sizes(half):
    s = half.make("oracle", 2, seed=SEED)
    assert s.open(0) == 0
    sizes = []
    for f in half.frames(A, N)[:2]:
        half.step(s, {0: f})
        need = cs.save_size(s, 0)
        one, two = cs.save(s, 0), cs.save(s, 0)
        assert one.nbytes == need and np.array_equal(one, two)       # save(NULL) = the bytes written; the same state gives the same bytes
        big = np.full(need + 5, 0x5A, np.uint8)                      # a larger buffer: only the blob's bytes are written
        assert L.moshi_hot_codec_slot_save(s.m, 0, big.ctypes.data, big.nbytes) == need
        assert np.array_equal(big[:need], one) and np.all(big[need:] == 0x5A)
        assert L.moshi_hot_codec_slot_save(s.m, 0, big.ctypes.data, need - 1) == -1
        sizes.append(need)
    assert sizes[1] - sizes[0] == cs.FRAME_BYTES
    for frames in (3, 124, 125, 126, 400):                           # the position alone decides the size: it grows until the ring is full, then stays
        s.set_fill(0, frames)
        assert cs.save_size(s, 0) == sizes[0] + (min(cs.ROWS_PER_FRAME * frames, cs.CAPACITY) - cs.ROWS_PER_FRAME) * (cs.FRAME_BYTES // cs.ROWS_PER_FRAME), frames
    states = sizes[0] - cs.HEADER - cs.FRAME_BYTES
    assert states % 16 == 0 and states > 0
    s.free()


@halves
def test_live_neighbour_is_untouched_by_snapshots_of_other_columns(half):
    s = half.make("oracle", 3, seed=SEED)
    cs.dirty(half, s, 2)
    a, x = half.frames(A, N), half.frames(X, N)
    assert s.open(0) == 0 and s.open(1) == 0
    got = [half.step(s, {0: a[0], 1: x[0]})[0]]
    assert cs.fork(s, 1, 2) == 0
    got.append(half.step(s, {0: a[1], 1: x[1], 2: x[1]})[0])
    blob = cs.save(s, 1)
    assert s.close(2) == 0 and s.close(1) == 0
    got.append(half.step(s, {0: a[2]})[0])
    assert cs.load(s, 1, blob) == 0
    got.append(half.step(s, {0: a[3], 1: x[0]})[0])
    s.free()
    ref = reference(half.name, ((A, 0, 7),))
    for k in range(4):
        assert cs.same(got[k], ref[k]), k


@halves
def test_every_refusal_changes_nothing(half):
    other = next(h for h in cs.HALVES if h is not half)
    o = other.make("oracle", 2, seed=SEED)
    assert o.open(0) == 0
    cs.run(other, o, 0, other.frames(A, N)[:1])
    other_blob = cs.save(o, 0)
    s = half.make("oracle", 3, seed=SEED)
    a = half.frames(A, N)
    assert s.open(0) == 0 and s.open(1) == 0
    first = half.step(s, {0: a[0], 1: a[0]})
    blob = cs.save(s, 0)
    n = blob.nbytes
    # fork
    assert cs.fork(s, 0, 0) == -1 and cs.fork(s, 0, 1) == -1 and cs.fork(s, 2, 1) == -1 and cs.fork(s, 2, 0) == -1   # src == dst, dst open, src closed
    assert cs.fork(s, -1, 2) == -1 and cs.fork(s, 0, 3) == -1 and cs.fork(s, 3, 2) == -1
    # save
    assert cs.save_size(s, 2) == -1 and cs.save_size(s, -1) == -1 and cs.save_size(s, 3) == -1
    buf = np.full(n, 0x5A, np.uint8)
    assert L.moshi_hot_codec_slot_save(s.m, 0, buf.ctypes.data, n - 1) == -1 and np.all(buf == 0x5A)
    # load
    assert cs.load(s, 0, blob) == -1 and cs.load(s, -1, blob) == -1 and cs.load(s, 3, blob) == -1      # open, bad index
    assert L.moshi_hot_codec_slot_load(s.m, 2, None, n) == -1
    assert cs.load(s, 2, blob[:cs.HEADER - 1]) == -1 and cs.load(s, 2, blob[:n - 1]) == -1             # short header, one byte short
    assert cs.load(s, 2, np.concatenate([blob, np.zeros(1, np.uint8)])) == -1                        # one byte long
    assert L.moshi_hot_codec_slot_load(s.m, 2, blob.ctypes.data, n + 1) == -1

    def patched(offset, fmt, value):
        b = blob.copy()
        b[offset:offset + np.dtype(fmt).itemsize] = np.array([value], fmt).view(np.uint8)
        return b

    h = cs.header(blob)
    flipped = blob.copy()
    flipped[16] ^= 1                                                 # one fingerprint byte
    bad = [flipped, patched(0, "<u4", 0x544C534D), patched(0, "<u4", h["magic"] ^ 0x100), patched(4, "<u4", 2), patched(8, "<u4", other.kind_id),
           patched(12, "<u4", 1), patched(24, "<i8", n + 16), patched(32, "<i8", 2), patched(32, "<i8", -1), patched(40, "<i8", 4), patched(40, "<i8", 0),
           other_blob]
    for i, b in enumerate(bad):
        assert cs.load(s, 2, b) == -1, i
    assert cs.load(o, 1, blob) == -1                                 # and this half's blob into the other half's model
    assert [s.position(b) for b in range(3)] == [1, 1, -1]
    # the LM snapshot calls keep refusing on a codec model, and the codec calls refuse on other kinds of model
    assert L.moshi_hot_slot_fork(s.m, 0, 2) == -1 and L.moshi_hot_slot_save(s.m, 0, None, 0) == -1 and L.moshi_hot_slot_load(s.m, 2, blob.ctypes.data, n) == -1
    one = hu.Model("oracle", half.cfg(), seed=SEED)
    assert L.moshi_hot_codec_slot_fork(one.m, 0, 1) == -1 and L.moshi_hot_codec_slot_save(one.m, 0, None, 0) == -1
    assert L.moshi_hot_codec_slot_load(one.m, 0, blob.ctypes.data, n) == -1
    one.free()
    cfg = hu.hot.tiny(L)
    cfg.enable_mimi_encoder = cfg.enable_mimi_decoder = 0
    be = hu.make_backend("oracle")
    lm = L.moshi_hot_create_slots(be, C.byref(cfg), SEED, 2)
    assert lm and L.moshi_hot_slot_open(lm, 0) == 0
    assert L.moshi_hot_codec_slot_fork(lm, 0, 1) == -1 and L.moshi_hot_codec_slot_save(lm, 0, None, 0) == -1
    assert L.moshi_hot_codec_slot_load(lm, 1, blob.ctypes.data, n) == -1
    L.moshi_hot_free(lm)
    L.ggml_backend_free(be)
    # nothing has changed: the blob is what it was, and both live slots' next frames are the reference's
    assert np.array_equal(cs.save(s, 0), blob)
    ref = reference(half.name, ((A, 0, 7),))
    assert cs.same(first[0], ref[0]) and cs.same(first[1], ref[0])
    for k in (1, 2):
        got = half.step(s, {0: a[k], 1: a[k]})
        assert cs.same(got[0], ref[k]) and cs.same(got[1], ref[k]), k
    # the column the refused loads aimed at still opens as a fresh conversation
    assert s.close(0) == 0 and s.close(1) == 0 and s.open(2) == 0
    assert cs.same(cs.run(half, s, 2, a[:1])[0], ref[0])
    s.free()
    o.free()


@halves
def test_reopening_a_loaded_slot_starts_a_fresh_conversation(half):
    s = half.make("oracle", 2, seed=SEED)
    assert s.open(0) == 0
    cs.run(half, s, 0, half.frames(X, N)[:2])
    blob = cs.save(s, 0)
    assert s.close(0) == 0
    cs.dirty(half, s, 1)
    assert cs.load(s, 1, blob) == 0 and s.position(1) == 2
    assert s.close(1) == 0 and s.open(1) == 0 and s.position(1) == 0
    got = cs.run(half, s, 1, half.frames(A, N)[:2])
    s.free()
    ref = reference(half.name, ((A, 0, 7),))
    assert cs.same(got[0], ref[0]) and cs.same(got[1], ref[1])
