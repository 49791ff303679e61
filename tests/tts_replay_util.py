"""Helpers for replay and full snapshots of tts-shaped slots (moshi_hot_slots_replay / moshi_hot_slot_replay / moshi_hot_slot_last_raw,
moshi_hot_slot_fork_full / _save_full / _load_full): a Slots model that takes histories and snapshots with conditions, and the single-stream
reference of one conversation - stepped with a text hook, its raw tokens logged, any of its frames forced with moshi_hot_force_last."""
import ctypes as C

import numpy as np

import hot_util as hu
import slot_prefill_util as pu
import tts_slots_util as tu

L = hu.L
KEEP = tu.KEEP


class Slots(tu.Slots):
    def replay(self, jobs, chunk=0):
        """jobs: [(slot, [frames of n_q + 1 tokens])] in one call -> the call's return value"""
        n = len(jobs)
        bufs = [pu.flat(fr) if len(fr) else np.zeros(1, np.int32) for _, fr in jobs]
        slots = (C.c_int32 * max(n, 1))(*[b for b, _ in jobs])
        ptrs = (C.c_void_p * max(n, 1))(*[a.ctypes.data for a in bufs])
        counts = (C.c_int32 * max(n, 1))(*[len(fr) for _, fr in jobs])
        return L.moshi_hot_slots_replay(self.m, n, slots, ptrs, counts, chunk)

    def replay_one(self, b, frames, chunk=0):
        buf = pu.flat(frames) if len(frames) else np.zeros(1, np.int32)
        return L.moshi_hot_slot_replay(self.m, b, buf.ctypes.data, len(frames), chunk)

    def last_raw(self, b):
        """the n_q + 1 tokens slot b committed last, or None when the call refuses"""
        out = np.full(self.cfg.n_q + 1, -7, np.int32)
        return out.tolist() if L.moshi_hot_slot_last_raw(self.m, b, out.ctypes.data) == 0 else None

    def fork_full(self, src, dst):
        return L.moshi_hot_slot_fork_full(self.m, src, dst)

    def save_full_size(self, b):
        return L.moshi_hot_slot_save_full(self.m, b, None, 0)

    def save_full(self, b):
        n = self.save_full_size(b)
        if n < 0:
            return None
        buf = np.full(n, 0xA5, np.uint8)
        assert L.moshi_hot_slot_save_full(self.m, b, buf.ctypes.data, n) == n
        return buf

    def load_full(self, b, blob, nbytes=None):
        blob = np.ascontiguousarray(blob, np.uint8)
        return L.moshi_hot_slot_load_full(self.m, b, blob.ctypes.data, blob.nbytes if nbytes is None else nbytes)


def history(cfg, n, seed):
    """n arbitrary history frames: a demuxed text value and dep_q audio tokens each - none of them -1, inside the delay_steps frames either"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        text = tu.demux_token(cfg, int(rng.integers(0, cfg.text_card)), int(rng.integers(-1, cfg.text_card))) if cfg.demux_second_stream \
            else int(rng.integers(0, cfg.text_card))
        out.append([text] + rng.integers(0, cfg.card, cfg.dep_q).tolist())
    return out


def single_reference(kind, cfg, cond_seed, texts, forced=None, seed=0, sampling=None):
    """a fresh single-stream model with the conditions of `cond_seed` and a text hook returning texts[offset]; forced = {frame: n_q + 1 tokens}: after
    that frame moshi_hot_force_last(text, audio) replaces what it committed -> (per frame (ok, text, audio, reads), per frame the raw tokens committed)"""
    m = hu.Model(kind, cfg, seed=seed)
    if sampling:
        assert hu.hot.set_sampling(L, m.m, 0, *sampling) == 0
    if cond_seed is not None:
        hu.set_conditions(m, cfg, seed=cond_seed)
    hu.set_text_hook(m, lambda offset, sampled: texts[offset] if texts[offset] != KEEP else sampled)
    out, raw = [], []
    for i in range(len(texts)):
        r = m.lm_step_n([])
        out.append(r + (tu.reads(m, cfg, i >= cfg.delay_steps),))
        if forced and i in forced:
            m.force_last(forced[i][0], forced[i][1:])
            raw.append(list(forced[i]))
        else:
            t, a = m.last_raw()
            raw.append([t] + a)
    m.free()
    return out, raw


def step(s, text_in, depth=True):
    """one live frame -> (n_valid, status, texts, audios, reads)"""
    return s.step(text_in) + (tu.reads(s, s.cfg, depth),)


def column(frames, b):
    """step() results -> what tts_slots_util.assert_column_equals_single takes for column b"""
    return [(f[1][b], f[2], f[3], f[4]) for f in frames]


def same_frames(a, b, cols, what=""):
    """two lists of step() results agree bit for bit in the given columns"""
    assert len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b)):
        for c in cols:
            assert x[1][c] == y[1][c] and x[2][c] == y[2][c] and x[3][c] == y[3][c], (what, k, c)
            for name in x[4]:
                assert np.array_equal(x[4][name][c], y[4][name][c]), (what, k, c, name)
