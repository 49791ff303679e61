"""Helpers for lockstep-stream models (moshi_hot_create_streams / moshi_hot_lm_step_streams)."""
import ctypes as C

import numpy as np

import hot_util as hu

L = hu.L


def lm_only(cfg):
    cfg.enable_mimi_encoder = cfg.enable_mimi_decoder = 0
    return cfg


class Streams:
    """B lockstep streams over one set of weights on a backend ("oracle" or "hip")."""

    create = "moshi_hot_create_streams"

    def __init__(self, kind, cfg, n_streams, seed=0):
        self.cfg, self.B = cfg, n_streams
        self.be = hu.make_backend(kind)
        self.m = getattr(L, self.create)(self.be, C.byref(cfg), seed, n_streams)
        assert self.m, f"{self.create} refused the configuration"

    def step(self, codes):
        """codes: B lists of (n_q - dep_q) codes -> (ok, [B text tokens], [B lists of dep_q audio tokens])"""
        B, n_in, dq = self.B, self.cfg.n_q - self.cfg.dep_q, self.cfg.dep_q
        ia = np.ascontiguousarray(np.array(codes, np.int32).reshape(B * n_in))
        txt = np.full(B, -7, np.int32)
        aud = np.zeros(B * dq, np.int32)
        r = L.moshi_hot_lm_step_streams(self.m, ia.ctypes.data, txt.ctypes.data, aud.ctypes.data)
        return r, txt.tolist(), aud.reshape(B, dq).tolist()

    def read(self, what, n_per_stream):
        out = np.zeros(self.B * n_per_stream, np.float32)
        assert L.moshi_hot_read_last(self.m, what.encode(), out.ctypes.data, out.size) == 0
        return out.reshape(self.B, n_per_stream)

    def stats(self):
        s = hu.pkg.Stats()
        L.ggml_backend_mi355x_get_stats(self.be, C.byref(s))
        return s

    def free(self):
        L.moshi_hot_free(self.m)
        L.ggml_backend_free(self.be)


def stream_codes(cfg, n_streams, n_frames, seed=0):
    """[frame][stream] -> (n_q - dep_q) codes, different for every stream"""
    rng = np.random.default_rng(seed)
    return rng.integers(0, cfg.card, (n_frames, n_streams, cfg.n_q - cfg.dep_q)).tolist()


def run_streams(kind, cfg, codes, seed=0, logits=False):
    """every frame of `codes` ([frame][stream]) through one B-stream model -> per frame (ok, texts, audios[, text_logits [B, text_card]])"""
    s = Streams(kind, cfg, len(codes[0]), seed)
    out = []
    for fr in codes:
        r = s.step(fr)
        out.append(r + (s.read("text_logits", cfg.text_card),) if logits else r)
    s.free()
    return out


def run_single(kind, cfg, codes_of_stream, seed=0, logits=False):
    """one stream's codes through a single-stream model (moshi_hot_create) -> per frame (ok, text, audio[, text_logits])"""
    m = hu.Model(kind, cfg, seed=seed)
    out = []
    for fr in codes_of_stream:
        r = m.lm_step(fr)
        out.append(r + (m.read("text_logits", cfg.text_card),) if logits else r)
    m.free()
    return out
