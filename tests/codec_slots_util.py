"""Helpers for the decoder-slots tests (moshi_hot_create_codec_slots, include/moshi_hot.h): a model wrapper, the staggered schedule the CPU and GPU tests
share and its single-stream references."""
import ctypes as C

import numpy as np

import hot_util as hu

L = hu.L
FRAME = 1920
N_FRAMES = 6


def cfg_of(wide=False):
    """the Mimi decoder alone at Mimi's own size (its widths are fixed by the checkpoint): 8 RVQ levels of 2048 codes"""
    cfg = hu.hot.moshika(L)
    cfg.enable_lm, cfg.enable_mimi_encoder, cfg.enable_mimi_decoder = 0, 0, 1
    cfg.mimi_n_q, cfg.mimi_codebook_size = 8, 2048
    cfg.wide_streams = 1 if wide else 0
    return cfg


def codes(seed, n=N_FRAMES, n_q=8, card=2048):
    """n frames of seeded random codes, int32 [n, n_q]"""
    return np.random.default_rng(seed).integers(0, card, (n, n_q)).astype(np.int32)


class CodecSlots:
    def __init__(self, kind, cfg, B, seed=0, flags=0):
        self.cfg, self.B = cfg, B
        self.be = hu.make_backend(kind)
        if kind == "hip" and flags:
            L.ggml_backend_mi355x_set_flags(self.be, flags)
        self.m = L.moshi_hot_create_codec_slots(self.be, C.byref(cfg), seed, B)
        assert self.m

    def open(self, b):
        return L.moshi_hot_codec_slot_open(self.m, b)

    def close(self, b):
        return L.moshi_hot_codec_slot_close(self.m, b)

    def position(self, b):
        return L.moshi_hot_codec_slot_position(self.m, b)

    def set_fill(self, b, frames):
        L.moshi_hot_codec_slot_set_fill(self.m, b, frames)

    def decode(self, rows):
        """rows: per slot a list of mimi_n_q codes, or None for a slot whose codes do not matter -> (return value, pcm [B, 1920], status [B])"""
        cd = np.full((self.B, self.cfg.mimi_n_q), 7, np.int32)
        for b, r in enumerate(rows):
            if r is not None:
                cd[b] = r
        pcm = np.full((self.B, FRAME), np.nan, np.float32)
        status = np.full(self.B, -7, np.int32)
        r = L.moshi_hot_mimi_decode_slots(self.m, cd.ctypes.data, pcm.ctypes.data, status.ctypes.data)
        return r, pcm, status

    def stats(self):
        s = hu.pkg.Stats()
        L.ggml_backend_mi355x_get_stats(self.be, C.byref(s))
        return s

    def free(self):
        L.moshi_hot_free(self.m)
        L.ggml_backend_free(self.be)


def single_reference(kind, cfg, frames, seed=0, flags=0):
    """a fresh single-stream codec-only model fed `frames` one by one -> pcm [n, 1920]"""
    m = hu.Model(kind, cfg, seed=seed, flags=flags)
    out = np.stack([m.mimi_decode(f.tolist()) for f in frames])
    m.free()
    return out


# The staggered schedule: spans of (slot, first frame, code sequence). Slot 0 opens at frame 0, closes after frame 3 and reopens at frame 4 with a new
# sequence; `late` (slot 2 of a B = 3 model) opens at frame 2; every other slot stays closed.
def schedule(late):
    return [(0, 0, codes(900)[:4]), (late, 2, codes(902)[:4]), (0, 4, codes(904)[:2])]


def run_schedule(s, spans, n=N_FRAMES, fills=None):
    """drive model s through the spans -> per frame (return value, pcm, status, the slots open in that frame)"""
    out = []
    for k in range(n):
        for b, first, seq in spans:
            if first == k:
                if s.position(b) >= 0:
                    assert s.close(b) == 0
                assert s.open(b) == 0
                if fills and (b, first) in fills:
                    s.set_fill(b, fills[(b, first)])
            elif first + len(seq) == k and not any(b2 == b and f2 == k for b2, f2, _ in spans):
                assert s.close(b) == 0
        rows = [None] * s.B
        for b, first, seq in spans:
            if first <= k < first + len(seq):
                rows[b] = seq[k - first]
        r, pcm, status = s.decode(rows)
        out.append((r, pcm, status, [b for b in range(s.B) if rows[b] is not None]))
    return out
