"""Helpers for stt-shaped B-column models (no Depth transformer, extra heads on transformer_out): lockstep streams and slots that read
moshi_hot_last_heads, and the single-stream reference of one conversation stepped with the VAD value requested."""
import ctypes as C

import numpy as np

import ggml_util as gu
import hot_util as hu
import sampling_util as sp
import slot_state_util as ss

L = hu.L
hot = hu.hot


class _Heads:
    def heads(self):
        """moshi_hot_last_heads -> [B, extra_heads, extra_heads_dim] (rows of columns whose status was not 1: -1)"""
        nh, hd = self.cfg.extra_heads, self.cfg.extra_heads_dim
        out = np.full(self.B * nh * hd, -7, np.float32)
        assert L.moshi_hot_last_heads(self.m, out.ctypes.data, out.size) == out.size
        return out.reshape(self.B, nh, hd)


class Streams(_Heads, sp.Streams):
    pass


class Slots(_Heads, ss.Slots):
    pass


def codes(cfg, n_frames, seed):
    """one conversation: n_frames x n_q codes"""
    return np.random.default_rng(seed).integers(0, cfg.card, (n_frames, cfg.n_q)).tolist()


def head_weights(model, cfg):
    """[extra_heads, extra_heads_dim, dim] float64: the heads' weights, dequantised with the oracle's row routine"""
    out = []
    for k in range(cfg.extra_heads):
        t = C.cast(L.moshi_hot_weight(model, f"lm.extra_heads.{k}.weight".encode()), hu.pkg.TP)
        assert t
        n = L.ggml_nbytes(t)
        raw = np.zeros(n, np.uint8)
        L.ggml_backend_tensor_get(t, raw.ctypes.data, 0, n)
        gtype = t.contents.type
        if gtype == gu.F32:
            w = raw.view(np.float32).reshape(cfg.extra_heads_dim, cfg.dim)
        else:
            w = gu.dequantize(raw.reshape(cfg.extra_heads_dim, -1), gtype, cfg.dim)
        out.append(w.astype(np.float64))
    return np.stack(out)


def numpy_heads(w, tout):
    """soft_max(w[k] @ tout) for every head, in float64: [extra_heads, extra_heads_dim]"""
    z = w @ tout.astype(np.float64)
    p = np.exp(z - z.max(axis=1, keepdims=True))
    return p / p.sum(axis=1, keepdims=True)


def single_reference(kind, cfg, frames, live, sampling=None, seed=0, chunk=0):
    """a fresh single-stream stt model: moshi_hot_prefill over `frames` (none: no call), then one live frame per entry of `live` with the VAD
    value requested -> per live frame (ok, text, [], text_logits, vad, transformer_out)"""
    if sampling:
        m = sp.Model(kind, sp.sampled(cfg, *sampling[1:]), seed=seed)
        assert m.set_sampling(0, *sampling) == 0
    else:
        m = sp.Model(kind, cfg, seed=seed)
    if len(frames):
        m.prefill(frames, chunk)
    out = []
    for fr in live:
        r = m.lm_step_n(fr, vad=True)
        out.append(r[:3] + (m.read("text_logits", cfg.text_card), r[3], m.read("transformer_out", cfg.dim)))
    m.free()
    return out


def step_all(model, per_col):
    """one frame of a Slots model: per_col = {slot: codes}; the others get zeros -> (n_valid, status, texts, audios, text_logits, heads)"""
    cds = [per_col.get(b, [0] * model.cfg.n_q) for b in range(model.B)]
    return model.step(cds) + (model.read("text_logits", model.cfg.text_card), model.heads())


def assert_column_equals_single(got, b, ref, what=""):
    """got: step_all results of the frames in which column b ran the conversation `ref` (single_reference) describes: status, token and text logits
    bit for bit; the VAD value (head 2, element 0 - all the single-stream step computes) bit for bit where the frame is valid, -1 rows elsewhere"""
    assert len(got) == len(ref)
    for k, (g, r) in enumerate(zip(got, ref)):
        assert g[1][b] == r[0], (what, b, k, g[1], r[0])
        assert np.array_equal(g[4][b], r[3]), (what, b, k)
        if r[0]:
            assert g[2][b] == r[1], (what, b, k)
            assert g[5][b, 2, 0] == np.float32(r[4]), (what, b, k, g[5][b, 2, 0], r[4])
            assert np.all(g[5][b] >= 0) and np.allclose(g[5][b].sum(axis=1), 1.0, atol=1e-6), (what, b, k)
        else:
            assert np.all(g[5][b] == -1), (what, b, k)
