"""CPU: slot snapshots (moshi_hot_slot_fork / _save / _load) on the host device with the oracle attached. Tiny LM, ring of 24, B = 3, everything
greedy and once more sampled with seeded columns. A forked or restored slot continues as the conversation it was copied from: tokens, status and text
logits bit for bit against a fresh single-stream model stepped through the whole history - at any position, past the ring's end included."""
import functools

import numpy as np
import pytest

import hot_util as hu
import sampling_util as sp
import slot_state_util as ss
import streams_util as su

N_BEFORE, N_AFTER = 7, 8
POSITIONS = (1, 13, 30)                      # 30 is past the wrap of the 24-slot ring, where prefill refuses
N_ALL = max(POSITIONS) + N_AFTER
SAMPLING = (1234, 0.9, 0.6, 12, 17)          # seed, temp, temp_text, top_k, top_k_text of the conversation under test
MODES = pytest.mark.parametrize("sampled", [False, True], ids=["greedy", "sampled"])


def base_cfg(sampled=False, context=24):
    cfg = su.lm_only(hu.hot.tiny(hu.L, context=context))
    return sp.sampled(cfg) if sampled else cfg


def codes(which):
    """A: the conversation itself (38 frames); B: what a fork is fed after it diverges"""
    return ss.live_codes(base_cfg(), N_ALL if which == "A" else N_AFTER, seed=71 if which == "A" else 72)


@functools.lru_cache(maxsize=None)
def reference(sampled, diverged=False):
    """the uninterrupted single-stream model: all of A, or 7 frames of A then B. Shared by the tests and never changed"""
    fr = codes("A")[:N_BEFORE] + codes("B") if diverged else codes("A")
    return ss.single_reference("oracle", base_cfg(sampled), [], fr, sampling=SAMPLING if sampled else None, seed=5)


def new_slots(sampled, B=3, seeded=(0,)):
    s = ss.Slots("oracle", base_cfg(sampled), B, seed=5)
    for b in seeded if sampled else ():
        assert s.set_sampling(b, *SAMPLING) == 0
    return s


@MODES
@pytest.mark.parametrize("same_codes", [True, False], ids=["same", "diverging"])
def test_forked_slot_and_its_source_continue_as_single_stream_models(sampled, same_codes):
    A, tail = codes("A"), codes("A")[N_BEFORE:] if same_codes else codes("B")
    s = new_slots(sampled)
    assert s.open(0) == 0
    before = ss.run(s, {0: A}, N_BEFORE)
    assert s.fork(0, 2) == 0
    assert [s.position(b) for b in range(3)] == [N_BEFORE, -1, N_BEFORE]
    if sampled:
        assert s.get_sampling(2) == s.get_sampling(0) and s.get_sampling(2)[5] and not s.get_sampling(1)[5]
    after = [ss.step_all(s, {0: A[N_BEFORE + k], 2: tail[k]}) for k in range(N_AFTER)]
    s.free()
    n = N_BEFORE + N_AFTER
    ss.assert_slot_equals_single(before + after, 0, reference(sampled, False)[:n], "source")
    ss.assert_slot_equals_single(after, 2, reference(sampled, not same_codes)[N_BEFORE:n], "fork")
    if same_codes:
        for k, r in enumerate(after):
            assert r[1][0] == r[1][2] and r[2][0] == r[2][2] and r[3][0] == r[3][2] and np.array_equal(r[4][0], r[4][2]), k
    assert all(r[1][1] == -1 for r in before + after)
    assert any(r[1][2] == 1 for r in after)


@functools.lru_cache(maxsize=None)
def saved(sampled):
    """slot 1 of a B = 3 model runs conversation A; -> ({position: blob}, [size asked with NULL at position 0, 1, ..])"""
    s = new_slots(sampled, seeded=(1,))
    assert s.open(1) == 0
    blobs, sizes = {}, []
    for k in range(max(POSITIONS) + 1):
        sizes.append(s.save_size(1))
        if k in POSITIONS:
            blobs[k] = s.save(1)
            assert blobs[k].nbytes == sizes[k] and s.position(1) == k
        if k < max(POSITIONS):
            ss.step_all(s, {1: codes("A")[k]})
    s.free()
    return blobs, sizes


@MODES
def test_blob_sizes_grow_with_the_position_until_the_ring_is_full(sampled):
    cfg = base_cfg(sampled)
    _, sizes = saved(sampled)
    header = sizes[0]                                   # position 0: no live ring row
    assert 0 < header < 4096
    for pos, n in enumerate(sizes):
        assert n == header + ss.ring_bytes(cfg, pos), pos
    assert sizes[cfg.context - 1] < sizes[cfg.context] == sizes[cfg.context + 1] == sizes[-1]


@MODES
@pytest.mark.parametrize("pos", POSITIONS)
def test_saved_slot_loaded_into_another_model_continues_the_conversation(sampled, pos):
    blob = saved(sampled)[0][pos]
    t = new_slots(sampled, B=2, seeded=())              # the blob brings the sampling setting with it
    assert t.load(0, blob) == 0
    assert t.position(0) == pos and t.position(1) == -1
    if sampled:
        assert np.allclose(t.get_sampling(0), SAMPLING + (True,), rtol=1e-6) and not t.get_sampling(1)[5]
    got = ss.run(t, {0: codes("A")[pos:]}, N_AFTER)
    again = t.save(0)                                   # and a blob of the restored slot loads as well
    t.free()
    ss.assert_slot_equals_single(got, 0, reference(sampled, False)[pos:pos + N_AFTER], f"loaded at {pos}")
    assert again.nbytes == saved(sampled)[1][min(pos + N_AFTER, len(saved(sampled)[1]) - 1)]


@MODES
def test_fork_of_a_slot_that_still_fills_its_delay_ring_and_of_a_held_slot(sampled):
    A = codes("A")
    s = new_slots(sampled)
    assert s.open(0) == 0
    first = ss.run(s, {0: A}, 1)
    assert first[0][1][0] == 0                          # the delay ring is still filling
    assert s.fork(0, 1) == 0
    got = [ss.step_all(s, {0: A[1 + k], 1: A[1 + k]}) for k in range(N_BEFORE - 1)]
    ss.assert_slot_equals_single(first + got, 0, reference(sampled, False)[:N_BEFORE], "source")
    ss.assert_slot_equals_single(got, 1, reference(sampled, False)[1:N_BEFORE], "fork of a filling slot")
    # a held slot counts as open; its fork is open and not held
    assert s.close(1) == 0 and s.hold(0, 1) == 0
    assert s.fork(0, 2) == 0
    got = [ss.step_all(s, {2: A[N_BEFORE + k]}) for k in range(N_AFTER)]
    assert all(r[1][0] == -2 and r[1][1] == -1 for r in got) and s.position(0) == N_BEFORE
    ss.assert_slot_equals_single(got, 2, reference(sampled, False)[N_BEFORE:N_BEFORE + N_AFTER], "fork of a held slot")
    assert s.hold(0, 0) == 0
    got = ss.run(s, {0: A[N_BEFORE:]}, N_AFTER)
    s.free()
    ss.assert_slot_equals_single(got, 0, reference(sampled, False)[N_BEFORE:N_BEFORE + N_AFTER], "the held source, released")


@MODES
def test_live_neighbour_is_untouched_by_snapshots_between_its_frames(sampled):
    A, Bc = codes("A"), codes("B")
    blob = saved(sampled)[0][30]
    runs = []
    for busy in (False, True):
        s = new_slots(sampled, seeded=(1,))
        assert s.open(1) == 0
        got = []
        for k in range(N_BEFORE + N_AFTER):
            per = {1: A[k]}
            if busy:
                if k == 0:
                    assert s.open(0) == 0
                if k == 3:
                    assert s.fork(0, 2) == 0
                if k == 5:
                    assert s.save(0) is not None and s.close(2) == 0
                if k == 6:
                    assert s.load(2, blob) == 0
                per[0] = Bc[k % N_AFTER]
                if 3 <= k < 5 or k >= 6:
                    per[2] = Bc[(k + 1) % N_AFTER]
            got.append(ss.step_all(s, per))
        s.free()
        runs.append(got)
    for got in runs:
        ss.assert_slot_equals_single(got, 1, reference(sampled, False)[:N_BEFORE + N_AFTER], "neighbour")
    assert any(r[1] == [1, 1, 1] for r in runs[1])


def corrupt(blob, offset, value=None):
    b = blob.copy()
    b[offset] = b[offset] ^ 0xFF if value is None else value
    return b


@MODES
def test_refused_calls_change_nothing(sampled):
    A = codes("A")
    blob = saved(sampled)[0][13]
    other_ring = ss.Slots("oracle", base_cfg(sampled, context=16), 2, seed=5)      # another fingerprint: a ring of 16
    assert other_ring.open(0) == 0
    foreign = other_ring.save(0)
    other_ring.free()
    other_mode = new_slots(not sampled, B=2, seeded=())                            # greedy against sampled
    assert other_mode.load(0, blob) == -1 and other_mode.position(0) == -1
    other_mode.free()

    s = new_slots(sampled)
    assert s.open(0) == 0
    got = ss.run(s, {0: A}, N_BEFORE)
    assert s.open(1) == 0
    # fork: bad indices, a closed source, an open destination, src == dst
    assert s.fork(-1, 2) == -1 and s.fork(0, 3) == -1 and s.fork(3, 2) == -1 and s.fork(0, -1) == -1
    assert s.fork(2, 0) == -1 and s.fork(2, 2) == -1 and s.fork(0, 1) == -1 and s.fork(0, 0) == -1
    # save: bad indices, a closed slot, a buffer one byte short
    assert s.save_size(-1) == -1 and s.save_size(3) == -1 and s.save_size(2) == -1 and s.save(2) is None
    n = s.save_size(0)
    short = np.full(n, 0x5A, np.uint8)
    assert hu.L.moshi_hot_slot_save(s.m, 0, short.ctypes.data, n - 1) == -1 and np.all(short == 0x5A)
    # load: bad indices, an open slot, truncated, oversized, a wrong magic / version / fingerprint, no buffer
    assert s.load(-1, blob) == -1 and s.load(3, blob) == -1 and s.load(0, blob) == -1 and s.load(1, blob) == -1
    assert s.load(2, blob, blob.nbytes - 1) == -1 and s.load(2, blob[:64]) == -1 and s.load(2, blob[:16]) == -1
    assert s.load(2, np.concatenate([blob, np.zeros(1, np.uint8)])) == -1
    assert s.load(2, corrupt(blob, 0)) == -1 and s.load(2, corrupt(blob, 4, 2)) == -1 and s.load(2, corrupt(blob, 8)) == -1
    assert s.load(2, foreign) == -1
    assert hu.L.moshi_hot_slot_load(s.m, 2, None, blob.nbytes) == -1
    assert [s.position(b) for b in range(3)] == [N_BEFORE, 0, -1]
    assert s.close(1) == 0
    got += ss.run(s, {0: A[N_BEFORE:]}, N_AFTER)
    assert s.load(2, blob) == 0 and s.position(2) == 13                              # the very blob loads once nothing is wrong with the call
    s.free()
    ss.assert_slot_equals_single(got, 0, reference(sampled, False)[:N_BEFORE + N_AFTER], "after refusals")


def test_other_model_kinds_refuse_and_go_on_as_if_never_asked():
    cfg = base_cfg()
    blob = saved(False)[0][13]
    buf = np.zeros(blob.nbytes, np.uint8)

    def refused(m):
        assert hu.L.moshi_hot_slot_fork(m, 0, 1) == -1
        assert hu.L.moshi_hot_slot_save(m, 0, None, 0) == -1 and hu.L.moshi_hot_slot_save(m, 0, buf.ctypes.data, buf.nbytes) == -1
        assert hu.L.moshi_hot_slot_load(m, 0, blob.ctypes.data, blob.nbytes) == -1 and hu.L.moshi_hot_slot_load(m, 1, blob.ctypes.data, blob.nbytes) == -1

    stream_codes = su.stream_codes(cfg, 2, 6, seed=3)
    ref = su.run_streams("oracle", cfg, stream_codes, seed=5, logits=True)
    st = su.Streams("oracle", cfg, 2, seed=5)
    for k, fr in enumerate(stream_codes):
        if k == 3:
            refused(st.m)
        r = st.step(fr)
        assert r == ref[k][:3] and np.array_equal(st.read("text_logits", cfg.text_card), ref[k][3]), k
    st.free()
    m = hu.Model("oracle", cfg, seed=5)
    for k, fr in enumerate(codes("A")[:6]):
        if k == 3:
            refused(m.m)
        r = m.lm_step(fr)
        assert r == reference(False, False)[k][:3] and np.array_equal(m.read("text_logits", cfg.text_card), reference(False, False)[k][3]), k
    m.free()


@MODES
def test_loaded_slot_closed_and_reopened_starts_fresh(sampled):
    s = new_slots(sampled, B=2, seeded=())
    assert s.load(1, saved(sampled)[0][30]) == 0 and s.position(1) == 30
    ss.step_all(s, {1: codes("A")[30]})
    assert s.position(1) == 31
    assert s.close(1) == 0 and s.open(1) == 0 and s.position(1) == 0
    got = ss.run(s, {1: codes("A")}, N_AFTER)                                        # (the column keeps the loaded sampling setting: the same seed replays)
    s.free()
    ss.assert_slot_equals_single(got, 1, reference(sampled, False)[:N_AFTER], "reopened")
