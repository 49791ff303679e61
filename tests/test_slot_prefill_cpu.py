"""CPU: slot prefill (moshi_hot_slots_prefill) on the host device with the oracle attached. A slot that takes a history in batched [dim, T] passes is
afterwards indistinguishable from a fresh single-stream model that ran moshi_hot_prefill over the same frames - tokens and text logits bit for bit,
greedy and with seeded sampling, for every chunking, several jobs in one pass, with the neighbours live and with the slot held between passes."""
import ctypes as C
import functools

import numpy as np
import pytest

import hot_util as hu
import sampling_util as sp
import slot_prefill_util as pu
import streams_util as su

N_HIST, N_HIST2, N_LIVE = 13, 6, 10
SAMPLING = (1234, 0.9, 0.6, 12, 17)          # seed, temp, temp_text, top_k, top_k_text of the prefilled slot
SAMPLING2 = (77, 0.7, 0.8, 20, 9)


def base_cfg(sampled=False):
    cfg = su.lm_only(hu.hot.tiny(hu.L))      # ring of 24 >= 13 history + 10 live frames
    return sp.sampled(cfg) if sampled else cfg


def hist(cfg, which):
    return pu.history(cfg, N_HIST if which == 1 else N_HIST2, seed=40 + which)


def live(cfg, which):
    return pu.live_codes(cfg, N_LIVE, seed=50 + which)


@functools.lru_cache(maxsize=None)
def reference(sampled, which):
    """the single-stream model of conversation `which` (1: 13 frames of history, 2: 6, 0: none), shared by the tests and never changed"""
    cfg = base_cfg(sampled)
    samp = None if not sampled else SAMPLING if which == 1 else SAMPLING2
    return pu.single_reference("oracle", cfg, hist(cfg, which) if which else [], live(cfg, which), sampling=samp, seed=5)


def new_slots(sampled, B=3):
    s = pu.Slots("oracle", base_cfg(sampled), B, seed=5)
    if sampled:
        assert s.set_sampling(1, *SAMPLING) == 0 and s.set_sampling(2, *SAMPLING2) == 0
    return s


def run_live(s, which_of_slot, n=N_LIVE):
    return [pu.step_all(s, {b: live(s.cfg, w)[k] for b, w in which_of_slot.items()}) for k in range(n)]


@pytest.mark.parametrize("chunk", [0, 1, 5, 64])
@pytest.mark.parametrize("sampled", [False, True], ids=["greedy", "sampled"])
def test_prefilled_slot_equals_single_stream_prefill(sampled, chunk):
    s = new_slots(sampled)
    assert s.open(1) == 0
    assert s.prefill_one(1, hist(s.cfg, 1), chunk) == N_HIST
    assert s.position(1) == N_HIST and s.position(0) == -1
    got = run_live(s, {1: 1})
    s.free()
    pu.assert_slot_equals_single(got, 1, reference(sampled, 1), f"chunk {chunk}")
    assert all(g[1][0] == -1 and g[1][2] == -1 for g in got)
    assert len({g[2][1] for g in got}) > 1


@pytest.mark.parametrize("sampled", [False, True], ids=["greedy", "sampled"])
def test_two_jobs_sharing_passes_equal_one_call_per_job_and_the_single_stream_models(sampled):
    # chunk 8 over 13 + 6 rows: passes 8 | 5 + 3 | 3 - a job that spans passes, a ragged 5 = 4 + 1 group and jobs of at most 4 rows
    runs = []
    for together in (True, False):
        s = new_slots(sampled)
        assert s.open(1) == 0 and s.open(2) == 0
        if together:
            assert s.prefill([(1, hist(s.cfg, 1)), (2, hist(s.cfg, 2))], 8) == N_HIST + N_HIST2
        else:
            assert s.prefill([(1, hist(s.cfg, 1))], 8) == N_HIST and s.prefill([(2, hist(s.cfg, 2))], 8) == N_HIST2
        assert [s.position(b) for b in range(3)] == [-1, N_HIST, N_HIST2]
        runs.append(run_live(s, {1: 1, 2: 2}))
        s.free()
    for got in runs:
        pu.assert_slot_equals_single(got, 1, reference(sampled, 1))
        pu.assert_slot_equals_single(got, 2, reference(sampled, 2))
    for a, b in zip(*runs):
        assert a[:4] == b[:4] and np.array_equal(a[4][1:], b[4][1:])


def test_live_neighbour_is_untouched_by_prefills_between_its_frames():
    cfg = base_cfg()
    runs = []
    for prefill in (False, True):
        s = new_slots(False)
        assert s.open(0) == 0
        got = []
        for k in range(N_LIVE):
            if prefill and k == 3:
                assert s.open(1) == 0 and s.open(2) == 0
                assert s.prefill([(1, hist(cfg, 1)), (2, hist(cfg, 2))], 8) == N_HIST + N_HIST2
                assert s.close(1) == 0 and s.close(2) == 0
            if prefill and k == 6:
                assert s.open(2) == 0 and s.prefill_one(2, hist(cfg, 2), 4) == N_HIST2   # the slot stays open: it steps along from here
            per = {0: live(cfg, 0)[k]}
            if prefill and k >= 6:
                per[2] = live(cfg, 2)[k - 6]
            got.append(pu.step_all(s, per))
        s.free()
        runs.append(got)
    pu.assert_slot_equals_single(runs[0], 0, reference(False, 0))
    pu.assert_slot_equals_single(runs[1], 0, reference(False, 0))
    pu.assert_slot_equals_single(runs[1][6:], 2, reference(False, 2)[:N_LIVE - 6])


def test_held_slot_prefilled_between_live_frames_equals_one_call():
    cfg = base_cfg()
    h = hist(cfg, 1)
    s = new_slots(False)
    assert s.open(0) == 0 and s.open(1) == 0
    assert s.hold(1, 1) == 0 and s.hold(2, 1) == -1 and s.hold(7, 1) == -1      # closed / bad slots cannot be held
    slot0 = []
    for k, part in enumerate((h[:5], h[5:10], h[10:])):
        assert s.prefill_one(1, part, 4) == len(part)
        r = pu.step_all(s, {0: live(cfg, 0)[k]})
        slot0.append(r)
        # held: status -2, outputs -1, nothing of the column advances; the slot that was never held and the closed one report as ever
        assert r[1][1] == -2 and r[2][1] == -1 and r[3][1] == [-1] * cfg.dep_q
        assert r[1][0] in (0, 1) and r[1][2] == -1 and r[0] == (r[1][0] == 1)
        assert s.position(1) == min(5 * (k + 1), N_HIST)
    assert s.hold(1, 0) == 0
    got = []
    for k in range(N_LIVE):
        r = pu.step_all(s, {0: live(cfg, 0)[(3 + k) % N_LIVE], 1: live(cfg, 1)[k]})
        got.append(r)
        if k < N_LIVE - 3:
            slot0.append(r)
    s.free()
    pu.assert_slot_equals_single(got, 1, reference(False, 1))            # = the slot prefilled in one call (the test above), bit for bit
    pu.assert_slot_equals_single(slot0, 0, reference(False, 0))
    # open and close clear the hold
    s = new_slots(False)
    assert s.open(1) == 0 and s.hold(1, 1) == 0 and s.open(1) == 0
    assert pu.step_all(s, {1: live(cfg, 1)[0]})[1][1] in (0, 1)
    assert s.hold(1, 1) == 0 and s.close(1) == 0 and s.open(1) == 0
    assert pu.step_all(s, {1: live(cfg, 1)[0]})[1][1] in (0, 1)
    s.free()


def test_refused_calls_change_nothing():
    cfg = base_cfg()
    h1, h2 = hist(cfg, 1), hist(cfg, 2)
    s = new_slots(False)
    assert s.open(1) == 0
    assert s.prefill_one(1, h1[:4], 0) == 4
    too_long = pu.history(cfg, cfg.context - 3, seed=1)                        # 4 + 21 > 24: would pass the ring's end
    assert s.prefill_one(1, too_long, 0) == -1
    assert s.prefill([(1, h1[4:]), (2, h2)], 8) == -1                          # slot 2 is closed
    assert s.prefill([(1, h1[4:8]), (1, h1[8:])], 8) == -1                     # named twice
    assert s.prefill([(1, h1[4:]), (3, h2)], 8) == -1 and s.prefill_one(-1, h2, 0) == -1   # bad indices
    assert s.prefill([(1, h1[4:]), (0, h2), (2, h2), (1, h2)], 8) == -1        # more jobs than slots
    assert s.prefill([], 8) == 0 and s.prefill_one(1, [], 8) == 0 and s.prefill([(1, [])], 0) == 0   # no frames: no work
    assert s.position(1) == 4
    assert s.prefill_one(1, h1[4:], 0) == N_HIST - 4
    got = run_live(s, {1: 1})
    s.free()
    pu.assert_slot_equals_single(got, 1, reference(False, 1), "after refusals")

    # a lockstep model and a single-stream model refuse, and go on as if never asked
    buf = pu.flat(h2)
    codes = su.stream_codes(cfg, 2, 6, seed=3)
    ref = su.run_streams("oracle", cfg, codes, seed=5, logits=True)
    st = su.Streams("oracle", cfg, 2, seed=5)
    for k, fr in enumerate(codes):
        if k == 3:
            assert hu.L.moshi_hot_slot_prefill(st.m, 0, buf.ctypes.data, N_HIST2, 0) == -1 and hu.L.moshi_hot_slot_hold(st.m, 0, 1) == -1
        r = st.step(fr)
        assert r == ref[k][:3] and np.array_equal(st.read("text_logits", cfg.text_card), ref[k][3]), k
    st.free()
    m = hu.Model("oracle", cfg, seed=5)
    for k, fr in enumerate(live(cfg, 0)[:6]):
        if k == 3:
            assert hu.L.moshi_hot_slot_prefill(m.m, 0, buf.ctypes.data, N_HIST2, 0) == -1 and hu.L.moshi_hot_slot_hold(m.m, 0, 1) == -1
        r = m.lm_step(fr)
        assert r == reference(False, 0)[k][:3] and np.array_equal(m.read("text_logits", cfg.text_card), reference(False, 0)[k][3]), k
    m.free()


def test_prefilled_slot_closed_and_reopened_starts_fresh():
    cfg = base_cfg()
    s = new_slots(False)
    assert s.open(1) == 0 and s.prefill_one(1, hist(cfg, 1), 0) == N_HIST
    pu.step_all(s, {1: live(cfg, 1)[0]})
    assert s.position(1) == N_HIST + 1
    assert s.close(1) == 0 and s.open(1) == 0 and s.position(1) == 0
    got = [pu.step_all(s, {1: live(cfg, 0)[k]}) for k in range(N_LIVE)]
    s.free()
    pu.assert_slot_equals_single(got, 1, reference(False, 0), "reopened")
