"""CPU (oracle backend): histories past the ring's end over Q8_0 K / V rings, kv_q8 = 7 (include/moshi_hot.h), tiny slots models, ring of
16. A 37-frame history (block rows to the ring's end, then ring-ordered rows across the wrap inside a pass, twice round) admitted through _prefill_long
at chunk 64 beside a stepping neighbour continues bit for bit as the same history admitted one row per pass, and so does a blob of it; the refusals."""
import ctypes as C

import pytest

import hot_util as hu
import slot_prefill_long_util as lu
import slot_prefill_util as pu
import slot_state_util as ss
import streams_util as su
import stt_slots_util as st
import tts_replay_util as tr
from test_kv_q8_histories_cpu import same

L = hu.L
RING, B, N_HIST, N_LIVE = 16, 3, 37, 6
SHAPES = {"moshika": (lambda: su.lm_only(hu.hot.tiny(L, context=RING)), ss.Slots), "stt": (lambda: hu.hot.tiny_stt(L, context=RING), st.Slots),
          "tts": (lambda: su.lm_only(hu.hot.tiny_tts(L)), tr.Slots)}


def new_slots(shape, kv_q8=7):
    cfg = SHAPES[shape][0]()
    cfg.kv_q8 = kv_q8
    return SHAPES[shape][1]("oracle", cfg, B, seed=5)


prefill_long = lu.Slots.prefill_long_one   # (the call needs the model handle alone: any Slots class will do)


@pytest.mark.parametrize("shape", ["moshika", "stt"])
def test_a_history_past_the_rings_end_continues_as_one_row_per_pass_and_from_a_blob(shape):
    runs, copy = [], None
    for chunk in (64, 1):
        s = new_slots(shape)
        hist = pu.history(s.cfg, N_HIST, seed=1)
        codes = {b: pu.live_codes(s.cfg, N_LIVE + 1, seed=10 + b) for b in (0, 1)}
        assert s.open(0) == 0
        ss.step_all(s, {0: codes[0][0]})
        assert s.open(1) == 0 and prefill_long(s, 1, hist, chunk) == N_HIST and [s.position(b) for b in (0, 1)] == [1, N_HIST]
        if chunk == 64:
            t = new_slots(shape)
            assert t.load(0, s.save(1)) == 0 and t.position(0) == N_HIST
            copy = ss.run(t, {0: codes[1]}, N_LIVE)
            t.free()
        runs.append(ss.run(s, {0: codes[0][1:], 1: codes[1]}, N_LIVE))
        s.free()
    for k, (a, b, c) in enumerate(zip(runs[0], runs[1], copy)):
        assert same(a, b, 0, 0) and same(a, b, 1, 1) and same(a, c, 1, 0) and a[1][:2] == [1, 1], f"live frame {k}"
    assert len({r[2][1] for r in runs[0]}) > 1


def test_what_stays_refused_and_the_values_that_mean_nothing():
    s, t = new_slots("moshika"), new_slots("tts")
    assert s.open(0) == 0 and t.open(0) == 0
    persona = hu.hot.Persona()
    assert L.moshi_hot_slot_persona(s.m, 0, C.byref(persona), 0) == -1 and s.position(0) == 0
    assert prefill_long(t, 0, tr.history(t.cfg, 2, seed=1), 0) == -1
    assert t.replay_one(0, tr.history(t.cfg, 2, seed=1)) == -1 and t.fork_full(0, 1) == -1 and t.save_full_size(0) == -1 and t.position(0) == 0
    be = hu.make_backend("oracle")
    for v in (5, 6, 8):
        s.cfg.kv_q8 = v
        assert not L.moshi_hot_create_slots(be, C.byref(s.cfg), 0, B) and not L.moshi_hot_create_streams(be, C.byref(s.cfg), 0, B)
    L.ggml_backend_free(be)
    s.free()
    t.free()
