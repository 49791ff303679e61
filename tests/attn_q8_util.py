"""Self-attention over Q8_0 K / V rings at the op level (moshi_hot_config::kv_q8): the graph of attention() for such a layer and a float64
restatement of its contract. Cases, RoPE, projections and the comparison are attn_ref_util's.

THE REFERENCE follows ggml's arithmetic for the graph's nodes. Every discontinuous step is made as ggml makes it: RoPE in float32, a ring row = the Q8_0
image of the float32 row (block_arith.quant_q80: d = amax / 127 kept as F16, q = roundf(x / d)), the query quantised the same way, a score = per block
the exact integer dot times float32(d_k * d_q), rounded to float32, the D / 32 block terms added in float32 in block order, score * scale rounded to
float32 before the mask is added. The soft_max and P x V are float64 over v = d_v * q_v; p is not rounded.

SLACK. p carries no BF16 rounding here, so there are no near ties; what the device may differ by is the float32 evaluation of p. attn_ref_util derives the
relative error of p as tau = 2 * (4 + 2 * max|x|) * 2^-24 (score and scaled score half an ulp each in the exponent, expf within 2 ulp, the reciprocal,
its rounding and the product 2 ulp, doubled) - with p unrounded that error reaches the output: slack[j] = tau * sum over slots of p_c * |V[c, j]|. The
float32 roundings of v * p and of the output are inside BAR. The ring bytes must be equal."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import attn_ref_util as ar  # noqa: E402
import block_arith as ba  # noqa: E402
import ggml_util as gu  # noqa: E402
from ggml_util import F32, I32, Q8_0  # noqa: E402


def geometry(D, H, C):
    return ar._geometry(f"q8 d{D} h{H} c{C}", D, H, C, [])


def q8_rows(x):
    """float32 [..., D] -> the rows' Q8_0 bytes [..., D / 32 * 34] (uint8)"""
    x = np.ascontiguousarray(x, np.float32)
    q, d = ba.quant_q80(x.reshape(-1))
    out = np.zeros((q.shape[0], 34), np.uint8)
    out[:, 0:2] = d.astype(np.float16).view(np.uint8).reshape(-1, 2)
    out[:, 2:] = q.astype(np.int8).view(np.uint8)
    return out.reshape(x.shape[:-1] + (x.shape[-1] // 32 * 34,))


def q8_fields(rows):
    """Q8_0 bytes [..., nb * 34] -> (q [..., nb, 32] int64, d [..., nb] float32)"""
    r = rows.reshape(rows.shape[:-1] + (-1, 34))
    return r[..., 2:].view(np.int8).astype(np.int64), np.ascontiguousarray(r[..., :2]).view(np.float16)[..., 0].astype(np.float32)


def rings_of(case):
    """the case's BF16 ring values as Q8_0 rings [B, H, C, ROWB]"""
    return q8_rows(gu.bf16_bits_to_f32(case.kbits)), q8_rows(gu.bf16_bits_to_f32(case.vbits))


def reference(case):
    """-> ar.Ref over the case's columns; kbits / vbits are the ring bytes viewed as uint16"""
    kr, vr = rings_of(case)
    outs, slacks = [], []
    for s in ar.streams_sequences(case):
        H, T, D = s.q.shape
        q, k = (ar.rope_rows(s.q, s.rot), ar.rope_rows(s.k, s.rot)) if s.rot is not None else (s.q, s.k)
        kr[s.b][:, s.idx[0], :] = q8_rows(k[:, 0, :])
        vr[s.b][:, s.idx[0], :] = q8_rows(s.v[:, 0, :])
        kq, kd = q8_fields(kr[s.b])                       # [H, C, nb, 32], [H, C, nb]
        vq, vd = q8_fields(vr[s.b])
        qq, qd = q8_fields(q8_rows(q[:, 0, :]))           # [H, nb, 32], [H, nb]
        sumi = np.einsum("hcbk,hbk->hcb", kq, qq).astype(np.float32)
        terms = sumi * (kd * qd[:, None, :]).astype(np.float32)
        score = np.zeros(terms.shape[:2], np.float32)
        for b in range(terms.shape[2]):
            score = (score + terms[:, :, b]).astype(np.float32)
        x = (score * np.float32(ar.attn_scale(D))).astype(np.float32) + s.mask[0][None].astype(np.float32)
        live = np.isfinite(x)
        x64 = np.where(live, x, -np.inf).astype(np.float64)
        e = np.where(live, np.exp(x64 - x64.max(axis=-1, keepdims=True)), 0.0)
        p = e / e.sum(axis=-1, keepdims=True)
        V = (vd[..., None] * vq.astype(np.float32)).astype(np.float32).reshape(H, -1, D).astype(np.float64)
        tau = 2.0 * (4.0 + 2.0 * np.where(live, np.abs(x64), 0.0).max(axis=-1)) * 2.0 ** -24
        outs.append(np.einsum("hc,hcd->hd", p, V)[:, None, :])
        slacks.append((tau[:, None] * np.einsum("hc,hcd->hd", p, np.abs(V)))[:, None, :])
    return ar.Ref(outs, slacks, kr.view(np.uint16), vr.view(np.uint16), 0, 0, 0, 0.0)


class Q8Graph:
    """attention() of a kv_q8 layer between the projections: ar.StreamsGraph's inputs with GGML_TYPE_Q8_0 rings [D, C, H, B], the dequantising
    get_rows(v, iota) in front of the transpose, iota a [C] index viewed as [C, H, B] with zero strides"""

    def __init__(self, kind, geo, B, rope, per_stream, flags=0):
        D, H, C = geo.D, geo.H, geo.C
        self.geo, self.B, self.rope, self.per_stream = geo, B, rope, per_stream
        g = self.g = gu.Graph(kind, mem_mb=64)
        if kind == "hip" and flags:
            g.set_flags(flags)
        self.proj = g.new(F32, 3 * H * D, 1, B)
        self.kc, self.vc = g.new(Q8_0, D, C, H, B), g.new(Q8_0, D, C, H, B)
        self.iota = g.input(np.arange(C), I32)
        if per_stream:
            self.mask, self.idx = g.new(F32, C, 1, 1, B), g.new(I32, 1, 1, B)
        else:
            self.mask, self.idx = g.new(F32, C, 1), g.new(I32, 1)
        rotr = roti = None
        if rope:
            self.rot = g.new(F32, D, B if per_stream else 1)
            nb1 = self.rot.contents.nb[1]
            if per_stream:
                rotr, roti = g.view_4d(self.rot, D // 2, 1, 1, B, nb1, nb1, nb1, 0), g.view_4d(self.rot, D // 2, 1, 1, B, nb1, nb1, nb1, 4 * (D // 2))
            else:
                rotr, roti = g.view_2d(self.rot, D // 2, 1, nb1, 0), g.view_2d(self.rot, D // 2, 1, nb1, 4 * (D // 2))
        p = self.proj.contents

        def third(i):
            t = g.cont(g.view_3d(self.proj, p.ne[0] // 3, p.ne[1], p.ne[2], p.nb[1], p.nb[2], i * (p.nb[1] // 3)))
            return g.permute(g.reshape_4d(t, D, H, t.contents.ne[1], t.contents.ne[2]), 0, 2, 1, 3)

        q, k, v = third(0), third(1), third(2)
        if rope:
            q, k = ar._apply_rope(g, q, k, rotr, roti)
        k = g.set_rows(self.kc, k, self.idx)
        v = g.set_rows(self.vc, v, self.idx)
        w = g.soft_max_ext(g.mul_mat(k, q), self.mask, ar.attn_scale(D), 0.0)
        vf = g.get_rows(v, g.view_3d(self.iota, C, H, B, 0, 0, 0))
        o = g.mul_mat(g.cont(g.transpose(vf)), w)
        self.out = g.cont(g.permute(o, 0, 2, 1, 3))   # [D, H, 1, B]
        g.build([self.out])
        g.alloc()

    def _ring(self, t):
        n = self.g.L.ggml_nbytes(t)
        buf = np.zeros(n, np.uint8)
        self.g.L.ggml_backend_tensor_get(t, buf.ctypes.data, 0, n)
        return buf.view(np.uint16).reshape(self.B, self.geo.H, self.geo.C, -1)

    def run(self, case):
        """-> ([per column [H, 1, D]], (K ring, V ring as uint16 [B, H, C, ROWB / 2]))"""
        g, geo, B = self.g, self.geo, self.B
        n = B if self.per_stream else 1
        pick = (lambda a: [a[0]] * n) if case.shared else (lambda a: list(a))
        kr, vr = rings_of(case)
        for t, arr in ((self.proj, case.proj.astype(np.float32)), (self.kc, kr), (self.vc, vr), (self.mask, np.stack(pick(case.masks)).astype(np.float32)),
                       (self.idx, np.array(pick(case.slots), np.int32))):
            ar._set_raw(g, t, arr)
        if self.rope:
            ar._set_raw(g, self.rot, np.stack([ar.rope_row(p, geo.D) for p in pick(case.positions)]))
        g.compute()
        out = g.get(self.out).reshape(B, geo.H, 1, geo.D)
        return [out[b] for b in range(B)], (self._ring(self.kc), self._ring(self.vc))

    def stats(self):
        return self.g.stats()

    def free(self):
        self.g.free()
