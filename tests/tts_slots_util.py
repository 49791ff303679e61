"""Helpers for tts-shaped B-column models (n_q == dep_q: no input codebook; per-column conditions and a text stream from above the boundary):
lockstep streams and slots stepped through moshi_hot_lm_step_*_text, the single-stream reference of one conversation (moshi_hot_set_conditions + a
text hook), and the ggml op wrappers the cross-attention node sequence needs."""
import ctypes as C

import numpy as np

import ggml_util as gu
import hot_util as hu
import sampling_util as sp
import slot_state_util as ss

L = hu.L
hot = hu.hot
KEEP = hot.TEXT_KEEP
F32 = gu.F32


def demux_token(cfg, first, second):
    """the text token that carries two ids (lm.h:176-191); second = -1: the right half is scaled by 0"""
    return (second + 1) * (cfg.text_card + 1) + first


def text_stream(cfg, b, n_frames):
    """column b's forced text stream: a different one per column"""
    return [demux_token(cfg, 7 + i + b, i - 1) for i in range(n_frames)]


def conditions(cfg, seed):
    """what hot_util.set_conditions(seed) uploads: (sum [dim] or None, cross [cross_len, dim] or None)"""
    rng = np.random.default_rng(seed)
    s = (rng.standard_normal(cfg.dim) * 0.1).astype(np.float32) if cfg.condition_sum else None
    x = rng.standard_normal((cfg.cross_len, cfg.dim)).astype(np.float32) if cfg.cross_attention else None
    return s, x


def tts_cfg(linear_type=F32, embed_type=F32, layers=1, **kw):
    cfg = hot.tiny_tts(L, linear_type=linear_type, embed_type=embed_type, layers=layers, **kw)
    cfg.enable_mimi_encoder = cfg.enable_mimi_decoder = 0
    return cfg


class _Tts:
    def set_conditions(self, b, seed):
        s, x = conditions(self.cfg, seed)
        return hot.set_conditions_column(L, self.m, b, s, x)

    def _text_in(self, text_in):
        if text_in is None:
            return None, None
        t = np.ascontiguousarray(np.array(text_in, np.int64).astype(np.int32))
        return t, t.ctypes.data


class Streams(_Tts, sp.Streams):
    def step(self, text_in, codes=None):
        """text_in: B text tokens (KEEP: the sampled one stays) or None -> (ok, [B text tokens], [B lists of dep_q audio tokens])"""
        B, dq = self.B, self.cfg.dep_q
        ia = None if codes is None else np.ascontiguousarray(np.array(codes, np.int32).reshape(-1))
        keep, tp = self._text_in(text_in)
        txt = np.full(B, -7, np.int32)
        aud = np.full(B * dq, -7, np.int32)
        r = L.moshi_hot_lm_step_streams_text(self.m, None if ia is None else ia.ctypes.data, tp, txt.ctypes.data, aud.ctypes.data)
        return r, txt.tolist(), aud.reshape(B, dq).tolist()


class Slots(_Tts, ss.Slots):
    def step(self, text_in, codes=None):
        """-> (n_valid, [B status], [B text tokens], [B lists of dep_q audio tokens])"""
        B, dq = self.B, self.cfg.dep_q
        ia = None if codes is None else np.ascontiguousarray(np.array(codes, np.int32).reshape(-1))
        keep, tp = self._text_in(text_in)
        txt = np.full(B, -7, np.int32)
        aud = np.full(B * dq, -7, np.int32)
        st = np.full(B, -7, np.int32)
        r = L.moshi_hot_lm_step_slots_text(self.m, None if ia is None else ia.ctypes.data, tp, txt.ctypes.data, aud.ctypes.data, st.ctypes.data)
        return r, st.tolist(), txt.tolist(), aud.reshape(B, dq).tolist()


def reads(model, cfg, depth):
    """text_logits, transformer_out and (when the Depth graph ran in that frame) every dep_logits<k>, as the model returns them"""
    out = {"text_logits": model.read("text_logits", cfg.text_card), "transformer_out": model.read("transformer_out", cfg.dim)}
    if depth:
        for k in range(cfg.dep_q):
            out[f"dep_logits{k}"] = model.read(f"dep_logits{k}", cfg.card)
    return {k: np.array(v, copy=True) for k, v in out.items()}


def single_reference(kind, cfg, cond_seed, texts, seed=0):
    """a fresh single-stream model with the conditions of `cond_seed` (None: never set) and a text hook that returns texts[offset]
    -> per frame (ok, text, audio, reads)"""
    m = hu.Model(kind, cfg, seed=seed)
    if cond_seed is not None:
        hu.set_conditions(m, cfg, seed=cond_seed)
    hu.set_text_hook(m, lambda offset, sampled: texts[offset] if texts[offset] != KEEP else sampled)
    out = []
    for i in range(len(texts)):
        r = m.lm_step_n([])
        out.append(r + (reads(m, cfg, i >= cfg.delay_steps),))
    m.free()
    return out


def assert_column_equals_single(got, b, ref, what=""):
    """got: per frame (status of column b's step or ok, texts, audios, reads) of the frames in which column b ran the conversation `ref` describes:
    status, tokens, text logits, transformer_out and the Depth logits of frames whose Depth graph ran for the column, bit for bit"""
    assert len(got) == len(ref)
    for k, (g, r) in enumerate(zip(got, ref)):
        assert g[0] == r[0], (what, b, k, g[0], r[0])
        if r[0]:
            assert g[1][b] == r[1] and g[2][b] == r[2], (what, b, k, g[1][b], r[1], g[2][b], r[2])
        for name, v in r[3].items():
            assert np.array_equal(g[3][name][b], v), (what, b, k, name)


# ---- op wrappers for the cross-attention node sequence (ggml_util.Graph) -----------------------------------------------------------------
def cross_attention_nodes(g, K, V, q, H, scale):
    """K / V: uploaded [D, Tc, H, B] tensors, q: [D * H, 1, B] -> the node sequence of cross_attention() up to x = [D * H, 1, B]"""
    ctx = g.ctx
    D = K.contents.ne[0]
    B = q.contents.ne[2]
    q4 = L.ggml_permute(ctx, L.ggml_reshape_4d(ctx, q, D, H, 1, B), 0, 2, 1, 3)
    w = L.ggml_soft_max_ext(ctx, L.ggml_mul_mat(ctx, K, q4), None, scale, 0.0)
    v = L.ggml_cont(ctx, L.ggml_transpose(ctx, V))
    o = L.ggml_mul_mat(ctx, v, w)
    o2 = L.ggml_cont(ctx, L.ggml_permute(ctx, o, 0, 2, 1, 3))
    return L.ggml_reshape_3d(ctx, o2, D * H, 1, B)
