"""CPU (oracle backend): histories over Q8_0 K / V rings, moshi_hot_config::kv_q8 = 3 (include/moshi_hot.h), tiny slots models, ring of 8.
Two histories admitted in one pass beside a stepping neighbour continue bit for bit as the same histories admitted one row per pass, job by job (a
one-row pass is the attention of a live step); a fork and a blob in a second model continue bit for bit as the conversation that was never copied, from
an odd row count - that conversation stepped on a kv_q8 = 1 model; what stays refused returns -1, the values of the field that mean nothing NULL."""
import ctypes as C

import numpy as np
import pytest

import hot_util as hu
import slot_prefill_util as pu
import slot_state_util as ss
import streams_util as su
import stt_slots_util as st
import tts_replay_util as tr

L = hu.L
RING, B = 8, 3
SHAPES = {"moshika": (lambda: su.lm_only(hu.hot.tiny(L, context=RING)), ss.Slots), "stt": (lambda: hu.hot.tiny_stt(L, context=RING), st.Slots),
          "tts": (lambda: su.lm_only(hu.hot.tiny_tts(L)), tr.Slots)}


def new_slots(shape, kv_q8=3):
    cfg = SHAPES[shape][0]()
    cfg.kv_q8 = kv_q8
    return SHAPES[shape][1]("oracle", cfg, B, seed=5)


def same(a, b, slot_a, slot_b):   # two step_all results: status, tokens and text logits of a slot of each, bit for bit
    return all(a[i][slot_a] == b[i][slot_b] for i in (1, 2, 3)) and np.array_equal(a[4][slot_a], b[4][slot_b])


@pytest.mark.parametrize("shape", ["moshika", "stt"])
def test_two_jobs_in_one_pass_continue_as_one_row_per_pass(shape):
    runs = []
    for together in (True, False):
        s = new_slots(shape)
        hx, hy = pu.history(s.cfg, 5, seed=1), pu.history(s.cfg, 3, seed=2)
        codes = {b: pu.live_codes(s.cfg, 7, seed=10 + b) for b in range(B)}
        assert s.open(0) == 0
        ss.step_all(s, {0: codes[0][0]})
        assert s.open(1) == 0 and s.open(2) == 0
        if together:
            assert s.prefill([(1, hx), (2, hy)]) == 8
        else:
            assert s.prefill_one(1, hx, 1) == 5 and s.prefill_one(2, hy, 1) == 3
        assert [s.position(b) for b in range(B)] == [1, 5, 3]
        runs.append(ss.run(s, {b: c[1:] for b, c in codes.items()}, 6))      # live frames across the ring's wrap
        s.free()
    for k, (a, b) in enumerate(zip(*runs)):
        assert all(same(a, b, i, i) for i in range(B)) and a[1] == [1, 1, 1], f"live frame {k}"
    assert len({r[2][1] for r in runs[0]}) > 1


def test_fork_and_a_blob_in_another_model_continue_from_an_odd_row_count():
    a, b, bf, ref = new_slots("moshika"), new_slots("moshika"), new_slots("moshika", kv_q8=0), new_slots("moshika", kv_q8=1)
    codes = pu.live_codes(a.cfg, 9, seed=3)
    assert ref.open(1) == 0 and a.open(1) == 0
    want = ss.run(ref, {1: codes}, 9)
    assert all(same(x, y, 1, 1) for x, y in zip(ss.run(a, {1: codes}, 5), want))      # 5 live rows: the copies take whole row groups, one row more at least
    assert a.fork(1, 2) == 0
    blob = a.save(1)
    assert bf.load(0, blob) == -1 and b.load(0, blob) == 0 and b.position(0) == 5      # the fingerprint holds the ring type
    for k in range(5, 9):
        ga, gb = ss.step_all(a, {1: codes[k], 2: codes[k]}), ss.step_all(b, {0: codes[k]})
        assert same(ga, want[k], 1, 1) and same(ga, want[k], 2, 1) and same(gb, want[k], 0, 1), f"frame {k}"
    for s in (a, b, bf, ref):
        s.free()


def test_what_stays_refused_and_the_values_that_mean_nothing():
    s, t = new_slots("moshika"), new_slots("tts")
    assert s.open(0) == 0 and t.open(0) == 0
    frames = pu.flat(pu.history(s.cfg, 2, seed=1))
    assert L.moshi_hot_slot_prefill_long(s.m, 0, frames.ctypes.data, 2, 0) == -1 and s.position(0) == 0
    assert t.replay_one(0, tr.history(t.cfg, 2, seed=1)) == -1 and t.fork_full(0, 1) == -1 and t.save_full_size(0) == -1 and t.position(0) == 0
    be = hu.make_backend("oracle")
    for v in (2, 4):
        s.cfg.kv_q8 = v
        assert not L.moshi_hot_create_slots(be, C.byref(s.cfg), 0, B) and not L.moshi_hot_create_streams(be, C.byref(s.cfg), 0, B)
    L.ggml_backend_free(be)
    s.free()
    t.free()
