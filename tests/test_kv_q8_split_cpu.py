"""CPU (oracle backend): bit 3 of moshi_hot_config::kv_q8 (include/moshi_hot.h) only asks the MI355X handle for the split step attention -
the model is that of the value without the bit: 9 computes what 1 computes, 11 what 3 computes, and the bit beside anything else is NULL."""
import ctypes as C

import numpy as np

import hot_util as hu
import slot_prefill_util as pu
import slot_state_util as ss
import streams_util as su

L = hu.L
RING = 8


def tiny(kv_q8):
    cfg = su.lm_only(hu.hot.tiny(L, context=RING))
    cfg.kv_q8 = kv_q8
    return cfg


def test_streams_with_the_bit_give_the_tokens_and_logits_without_it():
    codes = su.stream_codes(tiny(1), 2, 5, seed=5)
    a, b = (su.run_streams("oracle", tiny(v), codes, logits=True) for v in (9, 1))
    for k, (x, y) in enumerate(zip(a, b)):
        assert x[:3] == y[:3] and np.array_equal(x[3], y[3]), f"frame {k}"


def slots_run(kv_q8):
    cfg = tiny(kv_q8)
    s = ss.Slots("oracle", cfg, 2, seed=5)
    assert s.open(0) == 0 and s.open(1) == 0
    assert s.prefill([(1, pu.history(cfg, 3, seed=41))]) == 3
    out = pu.step_all(s, {0: pu.live_codes(cfg, 1, seed=52)[0], 1: pu.live_codes(cfg, 1, seed=51)[0]})
    s.free()
    return out


def test_slots_with_the_bit_give_the_step_without_it_after_a_prefill():
    a, b = slots_run(11), slots_run(3)
    assert a[:4] == b[:4] and np.array_equal(a[4], b[4])


def test_the_bit_beside_anything_else_is_refused():
    be = hu.make_backend("oracle")
    for v in (8, 10, 12, 16):
        cfg = tiny(v)
        assert not L.moshi_hot_create_streams(be, C.byref(cfg), 0, 2) and not L.moshi_hot_create_slots(be, C.byref(cfg), 0, 2), v
    L.ggml_backend_free(be)
