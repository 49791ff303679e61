"""Helpers for slot prefill (moshi_hot_slots_prefill / moshi_hot_slot_prefill / moshi_hot_slot_hold): a Slots model that takes histories, and the
single-stream reference of one conversation (moshi_hot_prefill over its history, then its live frames)."""
import ctypes as C

import numpy as np

import hot_util as hu
import sampling_util as sp

L = hu.L


def flat(frames):
    return np.ascontiguousarray(np.array(frames, np.int32).reshape(-1))


class Slots(sp.Slots):
    def prefill(self, jobs, chunk=0):
        """jobs: [(slot, [frames of n_q + 1 tokens])] in one call -> the call's return value"""
        n = len(jobs)
        bufs = [flat(fr) if len(fr) else np.zeros(1, np.int32) for _, fr in jobs]
        slots = (C.c_int32 * max(n, 1))(*[b for b, _ in jobs])
        ptrs = (C.c_void_p * max(n, 1))(*[a.ctypes.data for a in bufs])
        counts = (C.c_int32 * max(n, 1))(*[len(fr) for _, fr in jobs])
        return L.moshi_hot_slots_prefill(self.m, n, slots, ptrs, counts, chunk)

    def prefill_one(self, b, frames, chunk=0):
        buf = flat(frames) if len(frames) else np.zeros(1, np.int32)
        return L.moshi_hot_slot_prefill(self.m, b, buf.ctypes.data, len(frames), chunk)

    def hold(self, b, on):
        return L.moshi_hot_slot_hold(self.m, b, 1 if on else 0)


def history(cfg, n, seed):
    """n provided frames: a text token and n_q audio tokens each"""
    rng = np.random.default_rng(seed)
    return [[int(rng.integers(0, cfg.text_card))] + rng.integers(0, cfg.card, cfg.n_q).tolist() for _ in range(n)]


def live_codes(cfg, n, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, cfg.card, (n, cfg.n_q - cfg.dep_q)).tolist()


def single_reference(kind, cfg, frames, codes, sampling=None, seed=0, chunk=0, extra=()):
    """a fresh single-stream model: moshi_hot_prefill over `frames` (none: no call), then one live frame per entry of `codes`
    -> per live frame (ok, text, audio, text_logits, *[read(name, n) for name, n in extra])"""
    if sampling:
        m = sp.Model(kind, sp.sampled(cfg, *sampling[1:]), seed=seed)
        assert m.set_sampling(0, *sampling) == 0
    else:
        m = sp.Model(kind, cfg, seed=seed)
    if len(frames):
        m.prefill(frames, chunk)
    out = []
    for fr in codes:
        r = m.lm_step(fr)
        out.append(r + (m.read("text_logits", cfg.text_card),) + tuple(m.read(n, k) for n, k in extra))
    m.free()
    return out


def step_all(slots, per_slot):
    """one frame: per_slot = {slot: codes}; the other slots get zeros (closed or held slots ignore theirs)
    -> (n_valid, status, texts, audios, text_logits [B, text_card])"""
    n_in = slots.cfg.n_q - slots.cfg.dep_q
    codes = [per_slot.get(b, [0] * n_in) for b in range(slots.B)]
    return slots.step(codes) + (slots.read("text_logits", slots.cfg.text_card),)


def assert_slot_equals_single(got, b, ref, what=""):
    """got: step_all results of the frames in which slot b ran the conversation `ref` (single_reference) describes: bit for bit"""
    assert len(got) == len(ref)
    for k, (g, r) in enumerate(zip(got, ref)):
        assert g[1][b] == r[0], (what, b, k, g[1], r[0])
        if r[0]:
            assert g[2][b] == r[1] and g[3][b] == r[2], (what, b, k)
        assert np.array_equal(g[4][b], r[3]), (what, b, k)
