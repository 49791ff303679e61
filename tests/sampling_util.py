"""Helpers for per-conversation sampling (moshi_hot_set_sampling): seeded slots / streams / single-stream models and the numpy restatement of the
noise formula of include/moshi_hot.h."""
import ctypes as C

import numpy as np

import hot_util as hu
import slots_util as sl
import streams_util as su

L = hu.L
hot = hu.hot
M64 = (1 << 64) - 1


def copy_cfg(cfg):
    return type(cfg).from_buffer_copy(cfg)


def sampled(cfg, temp=0.8, temp_text=0.7, top_k=20, top_k_text=25):
    cfg = copy_cfg(cfg)
    cfg.temp, cfg.temp_text, cfg.top_k, cfg.top_k_text = temp, temp_text, top_k, top_k_text
    return cfg


class _Sampling:
    def set_sampling(self, b, seed, temp, temp_text, top_k, top_k_text):
        return hot.set_sampling(L, self.m, b, seed, temp, temp_text, top_k, top_k_text)

    def get_sampling(self, b):
        return hot.get_sampling(L, self.m, b)


class Slots(_Sampling, sl.Slots):
    pass


class Streams(_Sampling, su.Streams):
    pass


class Model(_Sampling, hu.Model):
    pass


def run_single(kind, cfg, sampling, codes_of_stream, seed=0, logits=False):
    """one conversation through a fresh single-stream model whose CONFIGURATION carries sampling = (seed, temp, temp_text, top_k, top_k_text)'s
    temperatures and top-k values and which is seeded with its seed -> per frame (ok, text, audio[, text_logits])"""
    cfg = sampled(cfg, *sampling[1:])
    m = Model(kind, cfg, seed=seed)
    assert m.set_sampling(0, *sampling) == 0
    out = []
    for fr in codes_of_stream:
        r = m.lm_step(fr)
        out.append(r + (m.read("text_logits", cfg.text_card),) if logits else r)
    m.free()
    return out


# ---- include/moshi_hot.h's formula, restated ---------------------------------------------------------------------------------------------------
def _mix(x):
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def noise_u(seed, frame, site, rank):
    h = _mix((seed + 0x9E3779B97F4A7C15) & M64)
    z = _mix(h ^ (((frame * 0xD1342543DE82EF95) + ((site << 32) | rank)) & M64))
    return np.float32(2 * (z >> 41) + 1) * np.float32(2.0 ** -24)


def lib_noise(seed, frame, site, n):
    out = np.zeros(n, np.float32)
    L.moshi_hot_sampling_noise(seed, frame, site, n, out.ctypes.data)
    return out
