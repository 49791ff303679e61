"""Helpers for the encoder-slots tests (moshi_hot_create_encoder_slots, include/moshi_hot.h): a model wrapper, seeded PCM, the staggered schedule the
CPU and GPU tests share, its single-stream references, and the code comparison that holds between two executors whose latents differ in the last bits."""
import ctypes as C

import numpy as np

import hot_util as hu

L = hu.L
FRAME = 1920
N_FRAMES = 6
N_Q = 8
CARD = 2048


def cfg_of(wide=False):
    """the Mimi encoder alone at Mimi's own size (its widths are fixed by the checkpoint): 8 RVQ levels of 2048 codes"""
    cfg = hu.hot.moshika(L)
    cfg.enable_lm, cfg.enable_mimi_encoder, cfg.enable_mimi_decoder = 0, 1, 0
    cfg.mimi_n_q, cfg.mimi_codebook_size = N_Q, CARD
    cfg.wide_streams = 1 if wide else 0
    return cfg


def pcm(seed, n=N_FRAMES):
    """n frames of a seeded tone under a slow envelope plus noise, amplitude ~0.3 (the codes vary from frame to frame), float32 [n, 1920]"""
    rng = np.random.default_rng(seed)
    t = np.arange(n * FRAME) / 24000.0
    f = 110.0 * (1 + seed % 7)
    wave = 0.3 * np.sin(2 * np.pi * f * t + seed) * (0.5 + 0.5 * np.sin(2 * np.pi * 0.7 * t + 0.1 * seed)) + 0.05 * rng.standard_normal(t.size)
    return wave.astype(np.float32).reshape(n, FRAME)


class EncoderSlots:
    def __init__(self, kind, cfg, B, seed=0, flags=0):
        self.cfg, self.B = cfg, B
        self.be = hu.make_backend(kind)
        if kind == "hip" and flags:
            L.ggml_backend_mi355x_set_flags(self.be, flags)
        self.m = L.moshi_hot_create_encoder_slots(self.be, C.byref(cfg), seed, B)
        assert self.m

    def open(self, b):
        return L.moshi_hot_codec_slot_open(self.m, b)

    def close(self, b):
        return L.moshi_hot_codec_slot_close(self.m, b)

    def position(self, b):
        return L.moshi_hot_codec_slot_position(self.m, b)

    def set_fill(self, b, frames):
        L.moshi_hot_codec_slot_set_fill(self.m, b, frames)

    def encode(self, rows):
        """rows: per slot a frame of 1920 samples, or None for a slot whose audio does not matter -> (return value, codes [B, n_q], status [B])"""
        x = np.full((self.B, FRAME), 0.25, np.float32)
        for b, r in enumerate(rows):
            if r is not None:
                x[b] = r
        codes = np.full((self.B, self.cfg.mimi_n_q), -7, np.int32)
        status = np.full(self.B, -7, np.int32)
        r = L.moshi_hot_mimi_encode_slots(self.m, x.ctypes.data, codes.ctypes.data, status.ctypes.data)
        return r, codes, status

    def latents(self):
        """the projected latents the two RVQ stacks quantised in the last call -> (first [B, 256], rest [B, 256])"""
        out = []
        for name in (b"enc_latent_first", b"enc_latent_rest"):
            a = np.zeros((self.B, 256), np.float32)
            assert L.moshi_hot_read_last(self.m, name, a.ctypes.data, a.size) == 0
            out.append(a)
        return out

    def stats(self):
        s = hu.pkg.Stats()
        L.ggml_backend_mi355x_get_stats(self.be, C.byref(s))
        return s

    def free(self):
        L.moshi_hot_free(self.m)
        L.ggml_backend_free(self.be)


def single_reference(kind, cfg, frames, seed=0, flags=0, fill=0):
    """a fresh single-stream codec-only model fed `frames` one by one, from transformer position `fill` (frames) on
    -> (codes [n, n_q], first latents [n, 256], rest latents [n, 256])"""
    m = hu.Model(kind, cfg, seed=seed, flags=flags)
    if fill:
        L.moshi_hot_set_context_fill(m.m, fill)
    codes, first, rest = [], [], []
    for f in frames:
        codes.append(m.mimi_encode(f))
        first.append(m.read("enc_latent_first", 256))
        rest.append(m.read("enc_latent_rest", 256))
    m.free()
    return np.array(codes, np.int32), np.stack(first), np.stack(rest)


# The staggered schedule: spans of (slot, first frame, audio). Slot 0 opens at frame 0, closes after frame 3 and reopens at frame 4 with new audio;
# `late` (the last slot) opens at frame 2; every other slot stays closed.
def schedule(late):
    return [(0, 0, pcm(900)[:4]), (late, 2, pcm(902)[:4]), (0, 4, pcm(904)[:2])]


def run_schedule(s, spans, n=N_FRAMES, fills=None):
    """drive model s through the spans -> per frame (return value, codes, status, the slots open in that frame, (first, rest) latents)"""
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
        r, codes, status = s.encode(rows)
        out.append((r, codes, status, [b for b in range(s.B) if rows[b] is not None], s.latents()))
    return out


def codebook(m, stack, level, card=CARD):
    """a codebook of model handle m as float64 [card, 256]"""
    t = C.cast(L.moshi_hot_weight(m, f"mimi.quantizer.rvq_{stack}.vq.layers.{level}._codebook.embedding".encode()), hu.pkg.TP)
    assert t
    e = np.zeros((card, 256), np.float32)
    L.ggml_backend_tensor_get(t, e.ctypes.data, 0, e.nbytes)
    return e.astype(np.float64)


class CodeCheck:
    """Codes of a device encode against an oracle encode of the same frame, when the latents the two quantise differ in their last bits. Per stack the
    codes must be equal level by level up to the first parting; there the device's code must be the arg-min for the device's own residual (recomputed
    in float64 from the device's latent, within 1 + 1e-6) and the oracle's two distances must lie within the gap the latent difference explains,
    2 |e . (c_b - c_a)|. Levels below a parting follow another residual and are skipped. Counts what was exact."""

    def __init__(self, book, n_q=N_Q):
        self.book, self.n_q = book, n_q          # book(stack, level) -> float64 [card, 256]
        self.pairs = self.pairs_exact = self.levels = self.levels_exact = 0
        self.partings = []

    def add(self, tag, codes_ref, codes_dev, lat_ref, lat_dev):
        """lat_*: (first [256], rest [256])"""
        ca, cb = [int(v) for v in codes_ref], [int(v) for v in codes_dev]
        self.pairs += 1
        self.pairs_exact += ca == cb
        self.levels += self.n_q
        for stack, sl, la, lb in (("first", slice(0, 1), lat_ref[0], lat_dev[0]), ("rest", slice(1, self.n_q), lat_ref[1], lat_dev[1])):
            xa, xb = ca[sl], cb[sl]
            if xa == xb:
                self.levels_exact += len(xa)
                continue
            lvl = next(j for j, (u, v) in enumerate(zip(xa, xb)) if u != v)
            self.levels_exact += lvl
            ra, rb = la.astype(np.float32), lb.astype(np.float32)
            for j in range(lvl):                 # residuals at the level where the codes part (float32 subtractions, as the graph does)
                q = self.book(stack, j)[xa[j]].astype(np.float32)
                ra, rb = ra - q, rb - q
            E = self.book(stack, lvl)
            dist_dev = ((E - rb.astype(np.float64)) ** 2).sum(1)
            assert dist_dev[xb[lvl]] <= dist_dev.min() * (1 + 1e-6), f"{tag} {stack} level {lvl}: device code {xb[lvl]} is not the nearest centroid of the device's own residual"
            da, db = float(((E[xa[lvl]] - ra.astype(np.float64)) ** 2).sum()), float(((E[xb[lvl]] - ra.astype(np.float64)) ** 2).sum())
            explained = 2 * abs(float((rb.astype(np.float64) - ra.astype(np.float64)) @ (E[xb[lvl]] - E[xa[lvl]])))
            assert db - da <= explained * (1 + 1e-3) + 1e-6 * da, f"{tag} {stack} level {lvl}: oracle distances {da:.9g} / {db:.9g}, latent difference explains only {explained:.3g}"
            self.partings.append((tag, stack, lvl))

    def assert_caps(self, what):
        """partings cannot hide a failure: at least half of the (slot, frame) pairs fully exact, at least 0.8 of all level codes counted exact"""
        print(f"{what}: {self.pairs_exact} of {self.pairs} (slot, frame) pairs fully exact, {self.levels_exact} of {self.levels} level codes exact, partings {self.partings}")
        assert self.pairs_exact >= 0.5 * self.pairs and self.levels_exact >= 0.8 * self.levels, (what, self.pairs_exact, self.pairs, self.levels_exact, self.levels)
