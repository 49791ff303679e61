"""Helpers for slot prefill past the ring's end (moshi_hot_slots_prefill_long / moshi_hot_slot_prefill_long): a Slots model that takes such histories
(it also forks, saves and loads), and the single-stream reference of a conversation made of live and provided stretches."""
import ctypes as C

import numpy as np

import hot_util as hu
import sampling_util as sp
import slot_prefill_util as pu
import slot_state_util as ss

L = hu.L
flat = pu.flat
history = pu.history
live_codes = pu.live_codes
step_all = pu.step_all
assert_slot_equals_single = pu.assert_slot_equals_single


class Slots(ss.Slots):
    def prefill_long(self, jobs, chunk=0):
        """jobs: [(slot, [frames of n_q + 1 tokens])] in one call -> the call's return value"""
        n = len(jobs)
        bufs = [flat(fr) if len(fr) else np.zeros(1, np.int32) for _, fr in jobs]
        slots = (C.c_int32 * max(n, 1))(*[b for b, _ in jobs])
        ptrs = (C.c_void_p * max(n, 1))(*[a.ctypes.data for a in bufs])
        counts = (C.c_int32 * max(n, 1))(*[len(fr) for _, fr in jobs])
        return L.moshi_hot_slots_prefill_long(self.m, n, slots, ptrs, counts, chunk)

    def prefill_long_one(self, b, frames, chunk=0):
        buf = flat(frames) if len(frames) else np.zeros(1, np.int32)
        return L.moshi_hot_slot_prefill_long(self.m, b, buf.ctypes.data, len(frames), chunk)


def single_reference(kind, cfg, stretches, codes, sampling=None, seed=0):
    """a fresh single-stream model taken through `stretches` - ("live", [codes per frame]) steps frames whose results are dropped, ("hist", [frames])
    is one moshi_hot_prefill (which steps single provided frames at and after the ring's wrap) - then one live frame per entry of `codes`
    -> per live frame (ok, text, audio, text_logits)"""
    if sampling:
        m = sp.Model(kind, sp.sampled(cfg, *sampling[1:]), seed=seed)
        assert m.set_sampling(0, *sampling) == 0
    else:
        m = sp.Model(kind, cfg, seed=seed)
    for what, frames in stretches:
        if what == "live":
            for fr in frames:
                m.lm_step(fr)
        elif len(frames):
            m.prefill(frames, 0)
    out = []
    for fr in codes:
        out.append(m.lm_step(fr) + (m.read("text_logits", cfg.text_card),))
    m.free()
    return out
