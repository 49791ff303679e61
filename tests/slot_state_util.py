"""Helpers for slot snapshots (moshi_hot_slot_fork / moshi_hot_slot_save / moshi_hot_slot_load): a Slots model that forks, saves and loads, and the
sizes a blob must have."""
import numpy as np

import hot_util as hu
import slot_prefill_util as pu

L = hu.L
step_all = pu.step_all
assert_slot_equals_single = pu.assert_slot_equals_single
single_reference = pu.single_reference
live_codes = pu.live_codes


class Slots(pu.Slots):
    def __init__(self, kind, cfg, n_slots, seed=0, flags=0):
        super().__init__(kind, cfg, n_slots, seed)
        if kind == "hip" and flags:
            L.ggml_backend_mi355x_set_flags(self.be, flags)

    def fork(self, src, dst):
        return L.moshi_hot_slot_fork(self.m, src, dst)

    def save_size(self, b):
        return L.moshi_hot_slot_save(self.m, b, None, 0)

    def save(self, b):
        """the blob of slot b as bytes (uint8 array), or None when the model refuses"""
        n = self.save_size(b)
        if n < 0:
            return None
        buf = np.full(n, 0xA5, np.uint8)
        assert L.moshi_hot_slot_save(self.m, b, buf.ctypes.data, n) == n
        return buf

    def load(self, b, blob, nbytes=None):
        blob = np.ascontiguousarray(blob, np.uint8)
        return L.moshi_hot_slot_load(self.m, b, blob.ctypes.data, blob.nbytes if nbytes is None else nbytes)


def ring_bytes(cfg, pos):
    """the K / V part of a blob at stream position pos: 2 x layers x H x min(pos, C) x D x 2"""
    return 2 * cfg.num_layers * cfg.dim * min(pos, cfg.context) * 2


def run(slots, per_slot_codes, n):
    """n frames; per_slot_codes = {slot: [codes of frame 0, 1, ..]} -> step_all results"""
    return [step_all(slots, {b: c[k] for b, c in per_slot_codes.items()}) for k in range(n)]
