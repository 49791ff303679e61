"""Selector weights that make the activation quantiser's hidden blocks observable ("The activation-rounding probe").

Every quantised linear rounds its activation row first (Q8_K blocks for Q4_K weights, Q8_0 blocks for Q8_0 / Q4_0 weights, BF16 / F16 for float
weights); the rounded blocks live in LDS or in a workspace and no graph output shows them. A weight row that is zero but for ONE unit entry turns
the product into a read-out of one hidden number:
  Q4_K   d = 1, dmin = 0, one sub-block scale 1, one nibble 1            y = fl(d_x q_x[m])           (every other term is an exact zero)
         d = 0, dmin = 1, one sub-block min 1                            y = -fl(d_x bsum_j)          (the 32-wide block sum)
  Q8_0   d = 1, qs one-hot 1 / all ones in one block                     y = d_x q_x[m] / d_x bsum    (d_x an F16 value: both products exact)
  Q4_0   d = 1, nibble 9 at m (8 elsewhere) / all nibbles 9              the same through (nib - 8)
  BF16 / F16 one-hot 1.0                                                 y = round_to_type(x[m])
With d_w = 1 there is one float operation per output, so a correct kernel has no freedom of association: the outputs equal the reference below as
values (the sign of a zero aside). Q4_K sets end with a "heavy" row (every nibble 15, every scale and min 63, d = dmin = 1): it saturates the folded
scales and the split block sums of the batched mat-mul; its sum over super-blocks is order-dependent and is held to a bar of roundings instead.

The reference is tests/golden/block_arith.py (quant_q8k, quant_q80: float32 restatements of the published quantisers) and round-to-nearest-even on
the bit pattern for BF16 / F16. Nothing here calls the oracle or the device. `mutate` names deliberately wrong quantisers for the CPU tests."""
import os
import sys
from fractions import Fraction

import numpy as np

import ggml_util as gu
from ggml_util import BF16, F16, Q4_0, Q4_K, Q8_0

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import block_arith as ba  # noqa: E402

QUANT = (Q4_K, Q8_0, Q4_0)
FLOAT = (BF16, F16)
NAMES = {Q4_K: "q4_K", Q8_0: "q8_0", Q4_0: "q4_0", BF16: "bf16", F16: "f16"}
f32 = np.float32


def _f16_bytes(a):
    return np.ascontiguousarray(a, dtype=np.float16).view(np.uint8).reshape(a.shape + (2,))


# ---- selector matrices ----------------------------------------------------------------------------------------------------------------------
def pack_q4k(d, dmin, sc, mn, nib):
    """d, dmin [M, nb]; sc, mn [M, nb, 8] six-bit; nib [M, nb, 256] in element order -> raw rows [M, nb * 144] (layout: block_arith.py)"""
    M, nb = d.shape
    out = np.zeros((M, nb, 144), np.uint8)
    out[:, :, 0:2] = _f16_bytes(d)
    out[:, :, 2:4] = _f16_bytes(dmin)
    sc, mn = sc.astype(np.uint8), mn.astype(np.uint8)
    for j in range(4):
        out[:, :, 4 + j] = (sc[:, :, j] & 63) | ((sc[:, :, j + 4] >> 4) << 6)
        out[:, :, 8 + j] = (mn[:, :, j] & 63) | ((mn[:, :, j + 4] >> 4) << 6)
        out[:, :, 12 + j] = (sc[:, :, j + 4] & 0xF) | ((mn[:, :, j + 4] & 0xF) << 4)
    n = nib.astype(np.uint8).reshape(M, nb, 4, 2, 32)      # group j: sub-block 2j in the low nibbles, 2j + 1 in the high nibbles
    out[:, :, 16:144] = (n[:, :, :, 0] | (n[:, :, :, 1] << 4)).reshape(M, nb, 128)
    return out.reshape(M, nb * 144)


class Selectors:
    """raw: the selector rows of one (weight type, K); n_val value rows, then n_sum block-sum rows, then n_heavy heavy rows"""

    def __init__(self, wt, K):
        self.wt, self.K = wt, K
        self.n_heavy = 0
        if wt == Q4_K:
            nb = K // 256
            self.n_val, self.n_sum, self.n_heavy = K, 8 * nb, 1
            M = self.M0 = K + 8 * nb + 1
            d, dmin = np.zeros((M, nb), f32), np.zeros((M, nb), f32)
            sc, mn, nib = np.zeros((M, nb, 8), np.uint8), np.zeros((M, nb, 8), np.uint8), np.zeros((M, nb, 256), np.uint8)
            m = np.arange(K)
            d[m, m // 256] = 1
            sc[m, m // 256, (m % 256) // 32] = 1
            nib[m, m // 256, m % 256] = 1
            s = np.arange(8 * nb)
            dmin[K + s, s // 8] = 1
            mn[K + s, s // 8, s % 8] = 1
            d[M - 1], dmin[M - 1], sc[M - 1], mn[M - 1], nib[M - 1] = 1, 1, 63, 63, 15
            self.raw = pack_q4k(d, dmin, sc, mn, nib)
        elif wt in (Q8_0, Q4_0):
            nb = K // 32
            self.n_val, self.n_sum = K, nb
            M = self.M0 = K + nb
            d = np.zeros((M, nb), f32)
            m, s = np.arange(K), np.arange(nb)
            d[m, m // 32] = 1
            d[K + s, s] = 1
            if wt == Q8_0:
                out = np.zeros((M, nb, 34), np.uint8)
                out[m, m // 32, 2 + m % 32] = 1
                out[K + s, s, 2:34] = 1
            else:
                out = np.full((M, nb, 18), 0x88, np.uint8)             # nibble 8 is the value 0
                e = m % 32
                out[m, m // 32, 2 + e % 16] = np.where(e < 16, 0x89, 0x98)   # low nibbles hold elements 0-15, high nibbles 16-31
                out[K + s, s, 2:18] = 0x99
            out[:, :, 0:2] = _f16_bytes(d)
            self.raw = out.reshape(M, -1)
        else:
            self.n_val, self.n_sum, self.M0 = K, 0, K
            self.raw = None                                             # the identity, encoded by Graph.input

    def weights(self, g, M=None):
        """the weight tensor of M rows: the selector rows repeated cyclically where a launch form needs more rows than there are selectors"""
        M = M or self.M0
        if self.raw is None:
            return g.input(np.eye(self.K, dtype=f32)[np.arange(M) % self.M0], self.wt)
        return g.input_raw(self.raw[np.arange(M) % self.M0], self.wt, self.K, M)


# ---- the reference quantisers, and deliberately wrong ones ---------------------------------------------------------------------------------
Q8K_MUTATIONS = ("half_away", "recip", "no_clamp", "trunc", "neighbour_amax", "bsum16", "bs_hi_div", "zero_nan", "last_tie")
Q80_MUTATIONS = ("half_even", "trunc", "d_unrounded", "d_toward_zero", "neighbour_amax", "bsum16", "zero_nan")
FLOAT_MUTATIONS = ("bf16_trunc",)


def _half_away(p):
    return (np.sign(p) * np.floor(np.abs(p).astype(np.float64) + 0.5)).astype(np.int32)


def q8k_blocks(v, mutate=None):
    """v [T, K] -> q [T, nb, 256] int32, d [T, nb] float32, bsum [T, nb, 8] int32 (32-wide sums). mutate None: block_arith.quant_q8k itself"""
    T, K = v.shape
    nb = K // 256
    if mutate is None:
        q, d = ba.quant_q8k(np.ascontiguousarray(v, f32).reshape(-1))
        q, d = q.reshape(T, nb, 256), d.reshape(T, nb)
    else:
        xb = np.ascontiguousarray(v, f32).reshape(T, nb, 256)
        q, d = np.zeros((T, nb, 256), np.int32), np.zeros((T, nb), f32)
        for t in range(T):
            for b in range(nb):
                x = xb[t, b]
                src = xb[t, (b + 1) % nb] if mutate == "neighbour_amax" else x
                a = np.abs(src)
                j = int(np.argmax(a)) if mutate != "last_tie" else 255 - int(np.argmax(a[::-1]))
                if src[j] == 0:
                    if mutate == "zero_nan":
                        d[t, b] = np.nan
                    continue
                with np.errstate(over="ignore", invalid="ignore"):
                    iscale = f32(127.0) * (f32(1.0) / src[j]) if mutate == "recip" else f32(-127.0) / src[j]
                    p = (iscale * x).astype(f32)
                r = _half_away(p) if mutate == "half_away" else np.trunc(p).astype(np.int32) if mutate == "trunc" else np.rint(p).astype(np.int32)
                q[t, b] = ((r + 128) % 256 - 128) if mutate == "no_clamp" else np.clip(np.minimum(127, r), -128, 127)   # (int8 storage)
                d[t, b] = f32(1.0) / iscale
    qs = q.reshape(T, nb, 8, 32)
    bsum = qs[..., :16].sum(-1) if mutate == "bsum16" else qs.sum(-1)
    if mutate == "bs_hi_div":       # the batched record keeps 64 hi + lo: hi by a division that truncates toward zero, not the arithmetic shift
        bsum = 64 * np.trunc(bsum / 64.0).astype(np.int32) + (bsum & 63)
    return q, d, bsum


def q80_blocks(v, mutate=None):
    """v [T, K] -> q [T, nb, 32] int32, d [T, nb] float32 (the F16 value), bsum [T, nb] int32. mutate None: block_arith.quant_q80 itself"""
    T, K = v.shape
    nb = K // 32
    if mutate is None:
        q, d = ba.quant_q80(np.ascontiguousarray(v, f32).reshape(-1))
        q, d = q.reshape(T, nb, 32), d.reshape(T, nb)
    else:
        xb = np.ascontiguousarray(v, f32).reshape(T, nb, 32)
        src = np.roll(xb, -1, axis=1) if mutate == "neighbour_amax" else xb
        d = (np.abs(src).max(-1) / f32(127.0)).astype(f32)
        with np.errstate(over="ignore", invalid="ignore"):
            idv = np.where(d != 0, f32(1.0) / np.where(d != 0, d, 1), 0).astype(f32)
            p = (xb * idv[..., None]).astype(f32)
        q = np.rint(p).astype(np.int32) if mutate == "half_even" else np.trunc(p).astype(np.int32) if mutate == "trunc" else _half_away(p)
        q = (q + 128) % 256 - 128                                      # int8 storage (a neighbour's amax overflows it)
        if mutate == "d_toward_zero":
            h = d.astype(np.float16)
            over = np.abs(h.astype(f32)) > np.abs(d)
            d = np.where(over, (h.view(np.uint16) - 1).view(np.float16), h).astype(f32)
        elif mutate != "d_unrounded":
            d = d.astype(np.float16).astype(f32)
        if mutate == "zero_nan":
            d = np.where(np.abs(xb).max(-1) == 0, np.nan, d).astype(f32)
    bsum = q[..., :16].sum(-1) if mutate == "bsum16" else q.sum(-1)
    return q, d, bsum


def round_to_type(v, wt, mutate=None):
    v = np.ascontiguousarray(v, f32)
    if wt == BF16:
        u = v.view(np.uint32)
        if mutate == "bf16_trunc":
            return (u & np.uint32(0xFFFF0000)).view(f32)
        return (((u + (0x7FFF + ((u >> 16) & 1))) >> 16).astype(np.uint32) << 16).view(f32)     # round to nearest even on the bit pattern
    return v.astype(np.float16).astype(f32)                              # IEEE round to nearest even, subnormals kept


class Reference:
    """sel [T, n_val + n_sum] float32: what the selector rows must return; heavy / bar [T, n_heavy]: the exact value of the heavy rows (as the
    nearest double of an exact rational) and its bar of roundings"""

    def __init__(self, sel, heavy=None, bar=None, bar_lanes=None):
        self.sel, self.heavy, self.bar, self.bar_lanes = sel, heavy, bar, bar_lanes


def reference(wt, v, mutate=None):
    """v [T, K]: the floats the quantiser sees (after any prologue) -> Reference"""
    v = np.ascontiguousarray(v, f32)
    T, K = v.shape
    with np.errstate(invalid="ignore", over="ignore"):
        if wt == Q4_K:
            q, d, bsum = q8k_blocks(v, mutate)
            val = (d[..., None] * q.astype(f32)).astype(f32).reshape(T, K)
            sums = (-(d[..., None] * bsum.astype(f32))).astype(f32).reshape(T, -1)
            nb = K // 256
            heavy, bar, bar_lanes = np.zeros((T, 1)), np.zeros((T, 1)), np.zeros((T, 1))
            for t in range(T):
                if not np.isfinite(d[t]).all():
                    heavy[t] = np.nan
                    continue
                exact, mag, mag_lanes = Fraction(0), Fraction(0), Fraction(0)
                for b in range(nb):
                    tot = int(bsum[t, b].sum())
                    isum, msum = 63 * 15 * tot, 63 * tot            # d_w = dmin_w = 1
                    dx = Fraction(float(d[t, b]))
                    exact += dx * (isum - msum)
                    mag += abs(dx * isum) + abs(dx * msum)
                    lanes = q[t, b].reshape(32, 8).sum(0)           # ggml's generic kernel keeps one float partial sum per element position mod 8
                    mag_lanes += sum(abs(dx * 63 * 15 * int(v)) for v in lanes) + abs(dx * msum)
                heavy[t, 0] = float(exact)
                bar[t, 0] = float((nb + 4) * Fraction(1, 2 ** 24) * mag)
                bar_lanes[t, 0] = float((nb + 12) * Fraction(1, 2 ** 24) * mag_lanes)
            return Reference(np.concatenate([val, sums], axis=1), heavy, bar, bar_lanes)
        if wt in (Q8_0, Q4_0):
            q, d, bsum = q80_blocks(v, mutate)
            val = (d[..., None] * q.astype(f32)).astype(f32).reshape(T, K)
            return Reference(np.concatenate([val, (d * bsum.astype(f32)).astype(f32)], axis=1))
        return Reference(round_to_type(v, wt, mutate))


def as_output(ref, M=None):
    """what a device that computed `ref` exactly would return: [T, M] float32 (the CPU tests feed mutated references through this)"""
    full = ref.sel if ref.heavy is None else np.concatenate([ref.sel, ref.heavy.astype(f32)], axis=1)
    M = M or full.shape[1]
    return full[:, np.arange(M) % full.shape[1]]


def assert_probe(got, ref, what="", who="device", lanes=False, residual=None):
    """got [T, M], M >= the selector count (cyclic repeats). Selector rows: equal as values (+0 == -0) and the same finite pattern. Heavy rows:
    within (nb + 4) 2^-24 sum_b (|d_w d_x isum_b| + |dmin d_x msum_b|) of the exact value - one rounding per factor and per super-block add, for a
    kernel that forms isum_b in integers. lanes=True is the bar of ggml's generic kernel (the oracle), which adds eight float partial sums per
    super-block (element positions mod 8): (nb + 12) 2^-24 sum_b (sum_l |d_x isum_b,l| + |d_x msum_b|) - two roundings for the factors of each
    side, nb adds per partial sum and for the mins, eight final adds; where the lanes cancel, |isum_b| says nothing about their roundings. The
    fraction of the first bar is printed either way. residual [T, M]: what the graph added to the product (one more correctly rounded operation on
    the selector rows; it must be zero on the heavy rows).
    -> the worst heavy-row error as a fraction of the first bar (0 without heavy rows)"""
    got = np.asarray(got)
    T, M = got.shape
    n_sel = ref.sel.shape[1]
    M0 = n_sel + (0 if ref.heavy is None else ref.heavy.shape[1])
    assert T == ref.sel.shape[0] and M >= M0, (got.shape, ref.sel.shape)
    src = np.arange(M) % M0
    issel = src < n_sel
    g, r = got[:, issel], ref.sel[:, src[issel]]
    if residual is not None:
        assert (residual[:, ~issel] == 0).all()
        with np.errstate(invalid="ignore"):
            r = (residual[:, issel] + r).astype(f32)
    assert np.array_equal(np.isfinite(g), np.isfinite(r)), f"{what}: finite pattern differs at {np.argwhere(np.isfinite(g) != np.isfinite(r))[:4].tolist()}"
    fin = np.isfinite(r)
    bad = fin & (g != r)
    if bad.any():
        t, i = np.argwhere(bad)[0]
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} selector outputs differ; first at column {t}, row {np.flatnonzero(issel)[i]} "
                             f"(selector {src[issel][i]}): got {g[t, i]!r}, want {r[t, i]!r}")
    worst = 0.0
    if ref.heavy is not None:
        gh = got[:, ~issel].astype(np.float64)
        rh, bar = ref.heavy[:, src[~issel] - n_sel], ref.bar[:, src[~issel] - n_sel]
        assert np.array_equal(np.isfinite(gh), np.isfinite(rh)), f"{what}: finite pattern of the heavy rows differs"
        err = np.where(np.isfinite(rh), np.abs(gh - rh), 0.0)
        frac = err / np.where(bar > 0, bar, 1.0)
        worst = float(frac.max())
        print(f"{what}: {who} heavy rows at most {worst:.4f} of the bar")
        if lanes:
            bar = ref.bar_lanes[:, src[~issel] - n_sel]
        assert (err <= bar).all(), f"{what}: heavy row off by {float((err / np.where(bar > 0, bar, 1.0)).max()):.3f} of its bar at {np.argwhere(err > bar)[:4].tolist()}"
    return worst


# ---- input families: each a function of (K, T, seed) -> [T, K] float32, T >= 3 ----------------------------------------------------------------
def _base(K, T, seed, scale=1.0):
    r = np.random.default_rng(seed)
    return r, (r.standard_normal((T, K)) * r.uniform(0.2, 3.0, (T, 1)) * scale).astype(f32)


def fam_random(K, T, seed):
    return _base(K, T, seed)[1]


def fam_zero(K, T, seed):
    """a zero 256-block (between live ones where K allows), a zero 32-block inside a live block, one all-zero row"""
    r, x = _base(K, T, seed)
    nb = K // 256
    for t in range(T):
        if nb >= 3:
            b = 1 + t % (nb - 2)
            x[t, 256 * b:256 * b + 256] = 0
        elif nb == 2:
            x[t, 256 * (t % 2):256 * (t % 2) + 256] = 0
        sb = (3 + 5 * t) % (K // 32)
        x[t, 32 * sb:32 * sb + 32] = 0
    x[T - 1] = 0
    return x


def fam_sign(K, T, seed):
    """per 256-block: row 3n the extreme element negative; row 3n + 1 a tie +a before -a; row 3n + 2 the tie -a before +a (even blocks: both inside one
    32-wide sub-block; odd blocks: in different sub-blocks)"""
    r, x = _base(K, T, seed)
    for t in range(T):
        for b in range(K // 256):
            blk = x[t, 256 * b:256 * b + 256]
            a = f32(1.5) * np.abs(blk).max()
            i = int(r.integers(0, 16)) + 32 * int(r.integers(0, 4))
            j = i + (int(r.integers(1, 16)) if b % 2 == 0 else 32 * int(r.integers(1, 4)) + int(r.integers(0, 16)))
            if t % 3 == 0:
                blk[i] = -a
            else:
                blk[i], blk[j] = (a, -a) if t % 3 == 1 else (-a, a)
    return x


def fam_halves(K, T, seed):
    """every 32-wide block holds +-127 * 2^k (so iscale and the Q8_0 scale are powers of two); every other value is an exact (n + 0.5) * 2^k, among them
    +-126.5 (127 away from zero, 126 to even), 0.5, 1.5, 2.5 and a second +-127 of the other sign"""
    r = np.random.default_rng(seed)
    x = np.zeros((T, K), f32)
    for t in range(T):
        for b in range(K // 256):
            k = (t + b) % 7 - 3
            n = r.integers(-127, 127, 256).astype(f32) + f32(0.5)
            for j in range(8):
                s = 1.0 if (t + b + j) % 2 == 0 else -1.0
                p = 32 * j + r.permutation(32)[:8]
                n[p] = np.array([127 * s, 126.5, -126.5, -127 * s, 0.5 * s, -1.5 * s, 2.5, -2.5], f32)
                first = np.sort(p[[0, 3]])
                n[first] = np.array([127 * s, -127 * s], f32)          # the first of the pair decides the sign of iscale
            x[t, 256 * b:256 * b + 256] = n * f32(2.0 ** k)
    return x


def fam_const(K, T, seed):
    """two 32-wide sub-blocks of one 256-block hold +amax and -amax throughout (the first in index order rounds to -127, the second to 127: block
    sums of -4064 and 4064, the two ends of the 64 hi + lo split); every third row also a whole 256-block of +amax where K has a second block"""
    r, x = _base(K, T, seed)
    nb = K // 256
    for t in range(T):
        a = f32(4.0) * np.abs(x[t]).max()
        if t % 3 == 2 and nb >= 2:
            b = (t + 1) % nb
            x[t, 256 * b:256 * b + 256] = a
        base = 256 * (t % nb)
        x[t, base + 32 * (t % 8):base + 32 * (t % 8) + 32] = a if t % 2 == 0 else -a
        x[t, base + 32 * ((t + 3) % 8):base + 32 * ((t + 3) % 8) + 32] = -a if t % 2 == 0 else a
    return x


def f16_tie_amax(m, e):
    """amax with amax / 127 exactly halfway between two F16 values: (1 + (2 m + 1) 2^-11) 2^e, times 127 (19 significant bits: exact in float32)"""
    return f32(127.0 * (1.0 + (2 * m + 1) * 2.0 ** -11) * 2.0 ** e)


def fam_f16scale(K, T, seed):
    """Q8_0 blocks whose scale amax / 127 is an F16 subnormal (amax = 1e-3), rounds to an F16 zero (amax = 1e-6), or sits on an F16 rounding tie
    (one with an even, one with an odd lower neighbour)"""
    r, x = _base(K, T, seed)
    nb = K // 32
    for t in range(T):
        bl = r.permutation(nb)[:4]
        for which, b in enumerate(bl):
            blk = x[t, 32 * b:32 * b + 32]
            if which < 2:
                blk *= f32((1e-3, 1e-6)[which]) / np.abs(blk).max()
            else:
                a = f16_tie_amax(int(r.integers(0, 500)) * 2 + (which - 2), int(r.integers(-6, 4)))
                blk *= f32(0.9) * a / np.abs(blk).max()
                blk[int(r.integers(0, 32))] = a if r.integers(0, 2) else -a
    return x


def fam_range_q8k(K, T, seed):
    """magnitudes of 1e-30 and 1e30 in different 256-blocks of one row (K = 256: in alternate rows); single denormal elements inside normal blocks"""
    r, x = _base(K, T, seed)
    nb = K // 256
    for t in range(T):
        if nb >= 2:
            x[t, 0:256] *= f32(1e-30)
            x[t, 256:512] *= f32(1e30)
        else:
            x[t] *= f32(1e-30 if t % 2 == 0 else 1e30)
        base = 256 * (nb - 1)
        x[t, base + 7], x[t, base + 200] = f32(1e-40), f32(-1e-42)
    return x


def fam_range_q80(K, T, seed):
    """the same for 32-wide blocks with an F16 scale: 1e-30 (the scale rounds to zero) and 1e6 (amax / 127 < 65504: no F16 overflow)"""
    r, x = _base(K, T, seed)
    nb = K // 32
    for t in range(T):
        bl = r.permutation(nb)[:3]
        x[t, 32 * bl[0]:32 * bl[0] + 32] *= f32(1e-30)
        x[t, 32 * bl[1]:32 * bl[1] + 32] *= f32(1e6)
        x[t, 32 * bl[2] + 5], x[t, 32 * bl[2] + 20] = f32(1e-40), f32(-1e-42)
    return x


def fam_float_edges(K, T, seed, wt):
    """BF16 / F16: mantissa ties with an even and an odd kept part, one bit either side of a tie, all-ones mantissas that round up into the next
    binade, results that are F16 subnormals, and -0"""
    r = np.random.default_rng(seed)
    drop = 16 if wt == BF16 else 13
    exp = r.integers(100, 141, (T, K)) if wt == BF16 else r.integers(113, 141, (T, K))       # F16: inside its normal range, below 2^14
    if wt == F16:
        exp[:, 5::16] = r.integers(96, 113, exp[:, 5::16].shape)                             # results in the F16 subnormal range (and below it)
    kept = r.integers(0, 1 << (23 - drop), (T, K))
    kept[:, 3::8] = (1 << (23 - drop)) - 1                                                   # all ones: a round-up carries into the exponent
    low = np.array([1 << (drop - 1), (1 << (drop - 1)) - 1, (1 << (drop - 1)) + 1, 0, (1 << drop) - 1], np.int64)[r.integers(0, 5, (T, K))]
    low[:, ::2] = 1 << (drop - 1)                                                            # half of all values are exact ties
    u = (r.integers(0, 2, (T, K)) << 31) | (exp << 23) | (kept << drop) | low
    x = u.astype(np.uint32).view(f32)
    x[:, 1] = f32(-0.0)
    return x


FAMILIES_Q8K = {"random": fam_random, "zero": fam_zero, "sign": fam_sign, "halves": fam_halves, "const": fam_const, "range": fam_range_q8k}
FAMILIES_Q80 = {"random": fam_random, "zero": fam_zero, "sign": fam_sign, "halves": fam_halves, "const": fam_const, "f16scale": fam_f16scale,
                "range": fam_range_q80}
FAMILIES_FLOAT = {"random": fam_random, "zero": fam_zero, "edges": fam_float_edges}


def families(wt):
    return FAMILIES_Q8K if wt == Q4_K else FAMILIES_Q80 if wt in (Q8_0, Q4_0) else FAMILIES_FLOAT


def family(wt, name, K, T, seed=0):
    fn = families(wt)[name]
    s = 100000 * seed + 10 * K + T + 7919 * ("random", "zero", "sign", "halves", "const", "f16scale", "range", "edges").index(name)
    return fn(K, T, s, wt) if fn is fam_float_edges else fn(K, T, s)


def stacked(wt, K, rows_each=3, seed=0):
    """every family of the weight type, rows_each rows apiece, as one [T, K] array (the GPU tests run them as one activation)"""
    return np.concatenate([family(wt, n, K, rows_each, seed) for n in families(wt)], axis=0)


# ---- prologues whose result is exact, so the quantiser sees bit-identical floats on every side ------------------------------------------------
EPS = 1e-8


def norm_inputs(K, T, seed):
    """integer-valued x (|x| <= 50, times a power of two per row) and a random float alpha: the double sum of squares is exact in any order,
    1 / sqrtf(mean + eps) and both products are correctly rounded operations (no contraction, no fast-math)"""
    r = np.random.default_rng(seed)
    x = (r.integers(-50, 51, (T, K)) * 2.0 ** r.integers(-6, 7, (T, 1))).astype(f32)
    alpha = (1.0 + 0.1 * r.standard_normal(K)).astype(f32)
    return x, alpha


def norm_values(x, alpha):
    """what alpha * rms_norm(x) hands to the quantiser: float squares summed in double, mean = float(sum / K), scale = 1 / sqrtf(mean + eps)"""
    K = x.shape[1]
    mean = ((x * x).astype(f32).astype(np.float64).sum(1) / K).astype(f32)
    scale = (f32(1.0) / np.sqrt((mean + f32(EPS)).astype(f32))).astype(f32)
    return ((x * scale[:, None]).astype(f32) * alpha[None]).astype(f32)


def gate_inputs(v, seed, random_l=False):
    """h = [l | r] with silu(l) * r == v exactly: l = 32 (1 + expf(-32) is 1, so silu(l) = l; r = v / 32 is exact unless it is denormal), or with
    random_l a random l in [20, 60] and r = v itself (the quantiser then sees fl(l v)). Every 37th element has l <= -90 instead, where
    l / (1 + expf(-l)) is -0 whatever r is. -> h [T, 2 K], and the floats the quantiser sees"""
    r = np.random.default_rng(seed)
    T, K = v.shape
    if random_l:
        l = r.uniform(20.0, 60.0, (T, K)).astype(f32)
        rr = v.copy()
    else:
        l = np.full((T, K), 32.0, f32)
        rr = (v / f32(32.0)).astype(f32)
    dead = np.zeros((T, K), bool)
    dead[:, 11::37] = True
    l[dead] = r.uniform(-200.0, -90.0, int(dead.sum())).astype(f32)
    seen = np.where(dead, f32(0.0), (l * rr).astype(f32)).astype(f32)
    return np.concatenate([l, rr], axis=1), seen


# ---- graphs ---------------------------------------------------------------------------------------------------------------------------------
def gate_views(g, hh):
    t = hh.contents
    left = g.view_4d(hh, t.ne[0] // 2, 1, t.ne[1], t.ne[2], t.nb[1] // 2, t.nb[1], t.nb[2], 0)
    right = g.view_4d(hh, t.ne[0] // 2, 1, t.ne[1], t.ne[2], t.nb[1] // 2, t.nb[1], t.nb[2], t.nb[1] // 2)
    return g.mul(g.silu(left), right)


def probe_graph(sel, a, prologue="plain", alpha=None, residual=None, M=None, per_row=False):
    """the selector product of the rows of `a` ([T, K]; gate: h [T, 2 K]). per_row: one mat-vec node per row (the T = 1 launch forms), else one
    mat-mul over all rows ([K, T] for block weights, [K, 1, T] for float weights - up to four plain columns would be the float mat-vec).
    residual [T, M] is added to the product. Outputs reshape to [T, M]."""
    T = a.shape[0]
    M = M or sel.M0
    isfloat = sel.wt in FLOAT

    def act(g, rows):
        n = rows.shape[0]
        if prologue == "gate":
            return gate_views(g, g.input(rows))
        x = g.input(rows.reshape(n, 1, -1) if (isfloat and n > 1) else rows)
        return g.mul(g.rms_norm(x, EPS), g.input(alpha)) if prologue == "norm" else x

    def build(g):
        w = sel.weights(g, M)
        outs = []
        for rows, res in ([(a[t:t + 1], None if residual is None else residual[t:t + 1]) for t in range(T)] if per_row else [(a, residual)]):
            y = g.mul_mat(w, act(g, rows))
            if res is not None:
                n = rows.shape[0]
                yt = y.contents
                shaped = res.reshape([int(yt.ne[i]) for i in (3, 2, 1, 0)])
                y = g.add(g.input(shaped), y)
                assert n == res.shape[0]
            outs.append(y)
        return outs
    return build


def collect(outs, T, M):
    return np.concatenate([o.reshape(-1, M) for o in outs], axis=0).reshape(T, M)


def probe_residual(sel, T, M, seed):
    """a random residual for the selector rows, zero on the heavy rows"""
    res = np.random.default_rng(seed).standard_normal((T, M)).astype(f32)
    res[:, (np.arange(M) % sel.M0) >= sel.n_val + sel.n_sum] = 0
    return res


def paired_gate_case(sel_out, K=512, seed=0):
    """linear_in [K -> 2 F] -> silu(l) * r -> linear_out (the selectors of sel_out, F = sel_out.K) from one plain activation row, with every
    intermediate exact: linear_in's rows are selectors themselves (l rows read block 0, whose values lie in [21, 59], so silu(l) = l; r rows read
    block 1 through a sub-block scale of 1 .. 5 and a nibble of 1 .. 3 - an exact integer factor), so l, r and g = fl(l r) are known bit for bit.
    -> build, g [1, F] (what linear_out's quantiser sees)"""
    F = sel_out.K
    r = np.random.default_rng(seed)
    x = np.concatenate([r.uniform(21.0, 59.0, 256), r.standard_normal(K - 256) * 1.7]).astype(f32).reshape(1, K)
    q, d, _ = q8k_blocks(x)
    nb = K // 256
    i = np.arange(F)
    dw = np.zeros((2 * F, nb), f32)
    sc, nib = np.zeros((2 * F, nb, 8), np.uint8), np.zeros((2 * F, nb, 256), np.uint8)
    e = i % 256
    s, n = 1 + (i // 256) % 5, 1 + (i // 256) % 3
    dw[i, 0], sc[i, 0, e // 32], nib[i, 0, e] = 1, 1, 1
    dw[F + i, 1], sc[F + i, 1, e // 32], nib[F + i, 1, e] = 1, s, n
    w_in = pack_q4k(dw, np.zeros_like(dw), sc, np.zeros_like(sc), nib)
    left = (d[0, 0] * q[0, 0, e].astype(f32)).astype(f32)
    right = (d[0, 1] * (s * n * q[0, 1, e]).astype(f32)).astype(f32)
    assert (left >= 20).all() and (left <= 60).all()
    seen = (left * right).astype(f32).reshape(1, F)

    def build(g):
        h = g.mul_mat(g.input_raw(w_in, Q4_K, K, 2 * F), g.input(x))
        return [g.mul_mat(sel_out.weights(g), gate_views(g, h))]
    return build, seen


# ---- general gate values: the tolerant form --------------------------------------------------------------------------------------------------
NEAR = 2.0 ** -10


def gate_general(K, T, seed):
    """l in [-8, 8], where expf matters: h [T, 2 K] and the reference's silu(l) r with expf correctly rounded (exp in double, rounded once). An
    expf within an ulp of that moves the value by an ulp or two, which the tolerant form below absorbs; nothing else in the chain is inexact."""
    r = np.random.default_rng(seed)
    l = r.uniform(-8.0, 8.0, (T, K)).astype(f32)
    rr = (r.standard_normal((T, K)) * r.uniform(0.2, 3.0, (T, 1))).astype(f32)
    e = np.exp(-l.astype(np.float64)).astype(f32)
    return np.concatenate([l, rr], axis=1), ((l / (f32(1.0) + e)).astype(f32) * rr).astype(f32)


def near_boundary(wt, v):
    """[T, K] bool: the reference's |scale x| lies within 2^-10 of a rounding boundary n + 0.5 (values of up to 127 known to a few 2^-24: the
    window is some 60 times what an ulp or two can move them)"""
    T, K = v.shape
    if wt == Q4_K:
        xb = v.reshape(T, -1, 256)
        j = np.abs(xb).argmax(-1)
        mx = np.take_along_axis(xb, j[..., None], -1)
        p = ((f32(-127.0) / mx).astype(f32) * xb).astype(f32)
    else:
        xb = v.reshape(T, -1, 32)
        d = (np.abs(xb).max(-1, keepdims=True) / f32(127.0)).astype(f32)
        p = (xb * (f32(1.0) / d).astype(f32)).astype(f32)
    a = np.abs(p.astype(np.float64))
    return (np.abs(a - np.floor(a) - 0.5) <= NEAR).reshape(T, K)


def assert_probe_tolerant(got, wt, v, what=""):
    """the selector outputs for an activation known only to an ulp or two. Per block: with the reference's scale or one of its two neighbours (one
    ulp of float32 for Q8_K, of F16 for Q8_0), every element NOT near a rounding boundary equals fl(d q_ref) exactly, a near one is q_ref or
    q_ref +- 1, and a block sum is off by at most the number of near elements in it. The heavy row is not looked at.
    -> (share of near elements, blocks that needed a neighbouring scale)"""
    T, K = v.shape
    near = near_boundary(wt, v)
    if wt == Q4_K:
        q, d, bsum = q8k_blocks(v)
        B, nsub, sgn = 256, 8, f32(-1.0)
        cands = lambda x: [x, np.nextafter(x, f32(np.inf)), np.nextafter(x, f32(-np.inf))]                      # noqa: E731
    else:
        q, d, bsum = q80_blocks(v)
        B, nsub, sgn = 32, 1, f32(1.0)
        cands = lambda x: [x] + [f32(np.nextafter(np.float16(x), np.float16(s))) for s in (np.inf, -np.inf)]    # noqa: E731
    nbk = K // B
    val, sums = got[:, :K].reshape(T, nbk, B), got[:, K:K + nbk * nsub].reshape(T, nbk, nsub)
    bsum, nearb = bsum.reshape(T, nbk, nsub), near.reshape(T, nbk, B)
    moved = 0
    for t in range(T):
        for b in range(nbk):
            qb, nr = q[t, b].reshape(B).astype(f32), nearb[t, b]
            nn = nr.reshape(nsub, 32).sum(1)
            for k, dc in enumerate(cands(d[t, b])):
                ok = np.array_equal(val[t, b][~nr], (dc * qb)[~nr])
                ok = ok and all(val[t, b][i] in [dc * (qb[i] + f32(s)) for s in (-1, 0, 1)] for i in np.flatnonzero(nr))
                ok = ok and all(sums[t, b, j] in [sgn * dc * f32(bsum[t, b, j] + s) for s in range(-nn[j], nn[j] + 1)] for j in range(nsub))
                if ok:
                    moved += k > 0
                    break
            else:
                bad = np.flatnonzero(~nr & (val[t, b] != d[t, b] * qb))
                raise AssertionError(f"{what}: column {t} block {b}: no scale within an ulp of {d[t, b]!r} explains the outputs; with the reference's "
                                     f"scale {bad.size} elements away from any boundary differ, first {bad[:4].tolist()}")
    return float(near.mean()), moved
