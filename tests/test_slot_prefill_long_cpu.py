"""CPU: slot prefill past the ring's end (moshi_hot_slots_prefill_long) on the host device with the oracle attached. A slot whose history crosses the
end of the Temporal ring, starts at or past it or goes round it more than once is afterwards indistinguishable from a fresh single-stream model that
ran moshi_hot_prefill over the same frames (which steps single provided frames at and after the wrap): status, tokens and text logits of the 8 live
frames that follow are equal bit for bit - greedy and with seeded sampling, on F32 and Q4_K weights, for every chunking, with a live neighbour, held
between calls, and through a snapshot. The refusing calls still refuse."""
import functools

import numpy as np
import pytest

import hot_util as hu
import sampling_util as sp
import slot_prefill_long_util as lu
import streams_util as su
import tts_slots_util as tu
from ggml_util import F32, Q4_0, Q4_K

C_RING, N_LIVE = 24, 8
SAMPLING = (1234, 0.9, 0.6, 12, 17)          # seed, temp, temp_text, top_k, top_k_text of the prefilled slot
WEIGHTS = {"f32": (F32, F32), "q4_k": (Q4_K, Q4_0)}
# name -> the calls that build the history: lengths of consecutive moshi_hot_slot_prefill_long calls on slot 1
CASES = {
    "a_crosses_the_wrap_37": [37],             # at chunk 10: passes 10 | 10 | 4 (to the ring's end) | 10 | 3 ring-ordered
    "b_twice_round_53": [53],                  # > 2 C
    "c_exactly_the_ring_24": [24],             # ends at the ring's end: all block form
    "c_starts_at_the_ring_end_24_7": [24, 7],  # the second call starts exactly at C
    "e_one_row_past_the_end_25": [25],         # a ring-ordered piece of one row
}


def base_cfg(sampled=False, weights="q4_k"):
    lt, et = WEIGHTS[weights]
    cfg = su.lm_only(hu.hot.tiny(hu.L, linear_type=lt, embed_type=et))      # ring of 24, D = 128, H = 4, 2 layers
    assert cfg.context == C_RING
    return sp.sampled(cfg) if sampled else cfg


def hist(cfg, n, seed=40):
    return lu.history(cfg, n, seed=seed)


def live(cfg, seed=50, n=N_LIVE):
    return lu.live_codes(cfg, n, seed=seed)


@functools.lru_cache(maxsize=None)
def reference(n_hist, sampled=False, weights="q4_k", seed=40, live_seed=50):
    """the single-stream model after moshi_hot_prefill over n_hist frames, then N_LIVE live frames; shared by the tests and never changed"""
    cfg = base_cfg(sampled, weights)
    return lu.single_reference("oracle", cfg, [("hist", hist(cfg, n_hist, seed))], live(cfg, live_seed), sampling=SAMPLING if sampled else None, seed=5)


def new_slots(sampled=False, weights="q4_k", B=3):
    s = lu.Slots("oracle", base_cfg(sampled, weights), B, seed=5)
    if sampled:
        assert s.set_sampling(1, *SAMPLING) == 0
    return s


def run_live(s, seed_of_slot, n=N_LIVE):
    return [lu.step_all(s, {b: live(s.cfg, sd)[k] for b, sd in seed_of_slot.items()}) for k in range(n)]


def prefill_calls(s, b, h, calls, chunk):
    at = 0
    for n in calls:
        assert s.prefill_long_one(b, h[at:at + n], chunk) == n
        at += n
        assert s.position(b) == at


# (a) (b) (c) (e), and (g): every chunking leaves the same state - the reference's
@pytest.mark.parametrize("chunk", [0, 1, 5, 10, 64])
@pytest.mark.parametrize("case", list(CASES))
def test_slot_prefilled_past_the_ring_end_equals_single_stream_prefill(case, chunk):
    calls = CASES[case]
    s = new_slots()
    assert s.open(1) == 0
    prefill_calls(s, 1, hist(s.cfg, sum(calls)), calls, chunk)
    got = run_live(s, {1: 50})
    s.free()
    lu.assert_slot_equals_single(got, 1, reference(sum(calls)), f"{case} chunk {chunk}")
    assert all(g[1][0] == -1 and g[1][2] == -1 for g in got)
    assert len({g[2][1] for g in got}) > 1


# (i) greedy and seeded-sampled, on F32 and Q4_K weights
@pytest.mark.parametrize("chunk", [0, 1, 5, 64])
@pytest.mark.parametrize("weights", ["f32", "q4_k"])
@pytest.mark.parametrize("sampled", [False, True], ids=["greedy", "sampled"])
@pytest.mark.parametrize("case", ["a_crosses_the_wrap_37", "b_twice_round_53"])
def test_greedy_and_seeded_on_f32_and_q4k(case, sampled, weights, chunk):
    calls = CASES[case]
    s = new_slots(sampled, weights)
    assert s.open(1) == 0
    prefill_calls(s, 1, hist(s.cfg, sum(calls)), calls, chunk)
    got = run_live(s, {1: 50})
    s.free()
    lu.assert_slot_equals_single(got, 1, reference(sum(calls), sampled, weights), f"{case} {weights} chunk {chunk}")


# (d) a slot stepped live past the wrap, then prefilled: the reference is a single-stream model over the same live frames and the same history
@pytest.mark.parametrize("chunk", [0, 1, 5, 64])
def test_slot_stepped_live_past_the_wrap_then_prefilled(chunk):
    cfg = base_cfg()
    before, h = live(cfg, 51, 30), hist(cfg, 9, seed=41)
    ref = lu.single_reference("oracle", cfg, [("live", before), ("hist", h)], live(cfg), seed=5)
    s = new_slots()
    assert s.open(1) == 0
    for fr in before:
        lu.step_all(s, {1: fr})
    assert s.position(1) == 30
    assert s.prefill_one(1, h, chunk) == -1 and s.position(1) == 30          # the refusing call refuses a slot past the ring's end
    assert s.prefill_long_one(1, h, chunk) == 9 and s.position(1) == 39
    got = run_live(s, {1: 50})
    s.free()
    lu.assert_slot_equals_single(got, 1, ref, f"live 30 + 9, chunk {chunk}")


# (f) two jobs in one call, one wholly before the wrap and one past it, beside a live slot 0
@pytest.mark.parametrize("chunk", [0, 1, 5, 64])
def test_two_jobs_one_before_and_one_past_the_wrap_beside_a_live_slot(chunk):
    cfg = base_cfg()
    h1, h2 = hist(cfg, 11, seed=42), hist(cfg, 37)
    runs = []
    for prefill in (False, True):
        s = new_slots()
        assert s.open(0) == 0
        got = []
        for k in range(3 + N_LIVE):
            if prefill and k == 3:
                assert s.open(1) == 0 and s.open(2) == 0
                assert s.prefill_long([(1, h1), (2, h2)], chunk) == 48
                assert [s.position(b) for b in range(3)] == [3, 11, 37]
            per = {0: live(cfg, 52, 3 + N_LIVE)[k]}
            if prefill and k >= 3:
                per[1], per[2] = live(cfg, 53)[k - 3], live(cfg)[k - 3]
            got.append(lu.step_all(s, per))
        s.free()
        runs.append(got)
    ref0 = lu.single_reference("oracle", cfg, [], live(cfg, 52, 3 + N_LIVE), seed=5)
    lu.assert_slot_equals_single(runs[0], 0, ref0)
    lu.assert_slot_equals_single(runs[1], 0, ref0, "slot 0 beside the call")      # bit-identical to the run without the call
    for a, b in zip(*runs):
        assert a[1][0] == b[1][0] and a[2][0] == b[2][0] and a[3][0] == b[3][0] and np.array_equal(a[4][0], b[4][0])
    lu.assert_slot_equals_single(runs[1][3:], 2, reference(37), "the job past the wrap")
    lu.assert_slot_equals_single(runs[1][3:], 1, reference(11, seed=42, live_seed=53), "the job before the wrap")


# (h) held between three calls, a live neighbour stepping in between
@pytest.mark.parametrize("chunk", [0, 1, 5, 7, 64])
def test_held_slot_prefilled_in_three_calls_between_live_frames(chunk):
    cfg = base_cfg()
    h = hist(cfg, 53)
    s = new_slots()
    assert s.open(0) == 0 and s.open(1) == 0 and s.hold(1, 1) == 0
    slot0, at = [], 0
    for k, n in enumerate((20, 17, 16)):       # ends at 20 (before the wrap), 37 (crosses it), 53 (wholly past it)
        assert s.prefill_long_one(1, h[at:at + n], chunk) == n
        at += n
        r = lu.step_all(s, {0: live(cfg, 52, 3 + N_LIVE)[k]})
        slot0.append(r)
        assert r[1][1] == -2 and r[2][1] == -1 and s.position(1) == at
    assert s.hold(1, 0) == 0
    got = []
    for k in range(N_LIVE):
        r = lu.step_all(s, {0: live(cfg, 52, 3 + N_LIVE)[3 + k], 1: live(cfg)[k]})
        got.append(r)
        slot0.append(r)
    s.free()
    lu.assert_slot_equals_single(got, 1, reference(53), "held, three calls")
    lu.assert_slot_equals_single(slot0, 0, lu.single_reference("oracle", cfg, [], live(cfg, 52, 3 + N_LIVE), seed=5), "the live neighbour")


# (j) a snapshot taken after a long prefill loads into another slot and continues bit for bit
@pytest.mark.parametrize("chunk", [0, 1, 5, 64])
@pytest.mark.parametrize("sampled", [False, True], ids=["greedy", "sampled"])
def test_snapshot_after_a_long_prefill_continues_in_another_slot(sampled, chunk):
    s = new_slots(sampled)
    assert s.open(1) == 0
    assert s.prefill_long_one(1, hist(s.cfg, 37), chunk) == 37
    blob = s.save(1)
    assert blob is not None and s.load(2, blob) == 0 and s.position(2) == 37
    got = run_live(s, {1: 50, 2: 50})
    s.free()
    lu.assert_slot_equals_single(got, 1, reference(37, sampled), "the prefilled slot")
    lu.assert_slot_equals_single(got, 2, reference(37, sampled), "the slot loaded from its snapshot")


# (k) refusals - and the refusing calls still refuse past the ring's end
@pytest.mark.parametrize("chunk", [0, 1, 5, 64])
def test_refusals_change_nothing_and_the_old_calls_still_refuse(chunk):
    cfg = base_cfg()
    h = hist(cfg, 37)
    s = new_slots()
    assert s.open(1) == 0
    assert s.prefill_long_one(1, h[:4], chunk) == 4
    assert s.prefill_one(1, h[4:], 0) == -1 and s.prefill([(1, h[4:])], 8) == -1          # 4 + 33 > 24: the old calls refuse
    assert s.prefill_long([(1, h[4:]), (2, h)], 8) == -1                                   # slot 2 is closed
    assert s.prefill_long([(1, h[4:20]), (1, h[20:])], 8) == -1                            # named twice
    assert s.prefill_long([(1, h[4:]), (3, h)], 8) == -1 and s.prefill_long_one(-1, h, 0) == -1   # bad indices
    assert s.prefill_long([(1, h[4:]), (0, h), (2, h), (1, h)], 8) == -1                   # more jobs than slots
    assert s.prefill_long([], 8) == 0 and s.prefill_long_one(1, [], 8) == 0 and s.prefill_long([(1, [])], 0) == 0
    assert s.position(1) == 4
    assert s.prefill_long_one(1, h[4:], chunk) == 33
    assert s.prefill_one(1, h[:1], 0) == -1 and s.position(1) == 37                        # ... and a slot that stands past it
    got = run_live(s, {1: 50})
    s.free()
    lu.assert_slot_equals_single(got, 1, reference(37), "after refusals")

    buf = lu.flat(h)
    st = su.Streams("oracle", cfg, 2, seed=5)                                              # a lockstep model
    assert hu.L.moshi_hot_slot_prefill_long(st.m, 0, buf.ctypes.data, 37, 0) == -1
    st.free()
    m = hu.Model("oracle", cfg, seed=5)                                                    # a single-stream model
    assert hu.L.moshi_hot_slot_prefill_long(m.m, 0, buf.ctypes.data, 37, 0) == -1
    m.free()
    tcfg = tu.tts_cfg(layers=2, cross_len=5)                                               # the tts shape
    t = tu.Slots("oracle", tcfg, 2)
    assert t.set_conditions(0, 4) == 0 and t.open(0) == 0
    tb = lu.flat(lu.history(tcfg, 3, seed=1))
    assert hu.L.moshi_hot_slot_prefill_long(t.m, 0, tb.ctypes.data, 3, 0) == -1
    t.free()


# (l) a job that does not pass the ring's end: the new call is the old one
@pytest.mark.parametrize("chunk", [0, 1, 5, 64])
def test_before_the_ring_end_the_new_call_is_the_old_one(chunk):
    cfg = base_cfg()
    h1, h2 = hist(cfg, 13), hist(cfg, 6, seed=43)
    runs = []
    for long in (False, True):
        s = new_slots()
        assert s.open(1) == 0 and s.open(2) == 0
        jobs = [(1, h1), (2, h2)]
        assert (s.prefill_long(jobs, chunk) if long else s.prefill(jobs, chunk)) == 19
        runs.append(run_live(s, {1: 50, 2: 53}))
        s.free()
    for a, b in zip(*runs):
        assert a[:4] == b[:4] and np.array_equal(a[4], b[4])
    lu.assert_slot_equals_single(runs[1], 1, reference(13))
