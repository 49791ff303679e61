"""Self-attention at the op level: a float64 restatement of the block, the graphs of its launch forms, the comparison.

THE BLOCK is the node sequence of attention() / attention_jobs() (moshi.cpp_amd/csrc/moshi_hot.cpp): RoPE on q and k, k and v stored as BF16 at the
sequence's ring slots, soft_max(K q * scale + mask), P x V. On the device it is attn_decode_body (hip_attn_body.h), reached as k_attn_decode (one column),
k_attn_streams (lockstep streams and stream slots), k_attn_blocks (slot prefill: block pieces) and k_attn_rows (ring-ordered one-row sequences).

THE REFERENCE (attention_reference) is plain numpy. Every discontinuous step is made exactly as ggml makes it - RoPE as separate float32 mul / sub / add
on interleaved pairs with the output de-interleaved, bf16(q) and bf16(k) to nearest even (ggml_util.f32_to_bf16_bits), v rounded to BF16 when stored, all
T rows of a sequence written before any row attends (last writer wins on a repeated slot), the score rounded to float32, score * scale rounded to float32
before the mask is added, p rounded to BF16 - and every sum (q . K, the sum of exponentials, P x V) in float64.

NEAR TIES. The device and the oracle evaluate expf and e * (1 / sum) in float32, so a probability may round to the other BF16 neighbour than the float64
value does. A live slot is a near tie when its float64 p lies within relative tau of a BF16 rounding midpoint,
    tau = 2 * (4 + 2 * max|x|) * 2^-24,        x = the row's scaled, masked scores.
Derived, not measured: the score and the scaled score carry half a float32 ulp each (relative 2^-24 each in x, the second rounding half an ulp again),
together at most 2 * |x| * 2^-24 absolute in the exponent, which exp turns into the same relative error of e; expf itself is within 2 ulp
(2 * 2^-24 relative); the reciprocal of the sum, its rounding to float32 and the product are 1.5 ulp more (rounded up: 2 * 2^-24); that is
(4 + 2 max|x|) * 2^-24, doubled as margin. slack[j] = sum over the row's near-tie slots of ulp_bf16(p_c) * |V[c, j]|: what the output may move by if every
one of them goes the other way. test_attn_columns_cpu.py caps how many near ties the inputs may hold, so that the slack cannot hide a dropped slot.

THE COMPARISON (assert_matches): |got - ref| <= BAR * max|ref| + slack elementwise, the same finite pattern, and the K / V ring BYTES equal to the
reference's in every slot of every column - the ones the step must not touch included."""
import collections

import numpy as np

import ggml_util as gu
from ggml_util import BF16, F32, I32

# BAR = 4 x the worst |oracle - reference| / max|reference| over the whole case table, measured on the CPU oracle by tests/test_attn_columns_cpu.py
# over rows that hold no near tie (2026-10-20: 5.903e-8 over 321 cases, all forms between 4.4e-8 and 5.9e-8 - the final float32 rounding of the output
# alone is 2^-24 = 5.96e-8; near ties were 167 of 625 323 live probabilities, 0.027 %, at most 2 in one row). Why 4 x: device and oracle make the same
# float32 roundings and differ in the order of float64 partial sums and in expf by an ulp, which the BF16 rounding of p absorbs or turns into a flip the
# slack covers. It must stay below the project's own 2e-6 (tests/test_hip_ops.py); if it does not, the reference is wrong.
# The device's own worst per form, same figure, one MI355X run of tests/test_attn_columns_gpu.py (2026-10-20; a record, never a source for the bar) -
# fused launches and plain nodes (backend flag 1) gave the same figures: lockstep 5.903e-8, slots 5.480e-8, single column 5.874e-8, blocks 5.614e-8,
# rows 5.599e-8.
ORACLE_WORST = 5.91e-8
BAR = 4 * ORACLE_WORST

Seq = collections.namedtuple("Seq", "b q k v idx mask rot")   # column; q / k / v [H, T, D] f32; ring slots [T]; mask block [T, C]; RoPE rows [T, D] (cos | sin) or None
Ref = collections.namedtuple("Ref", "out slack kbits vbits n_live n_ties max_row_ties max_x")
Geometry = collections.namedtuple("Geometry", "name D H C waves spw n_ends")


def _geometry(name, D, H, C, n_ends):
    waves = 8 if D <= 64 and C >= 128 else 4          # (k_attn_streams / k_attn_blocks / k_attn_rows: wide = D <= 64 && C >= 128)
    return Geometry(name, D, H, C, waves, 64 // (D // 8), n_ends)


# the smallest shapes at which the body can still go wrong: LPS = D / 8 lanes per slot, SPW = 64 / LPS slots per wave per pass, ATTN_NPRE = 4 passes
# requested at entry, loops striding by the thread count. n_ends: 1, either side of a pass, of the entry prefetch, of the thread count, the full ring.
GEOMETRIES = {g.name: g for g in (
    _geometry("d128", 128, 2, 300, [1, 2, 16, 17, 64, 65, 128, 129, 256, 257, 300]),     # 4 waves: 16 slots per pass / 64 at entry / 256 threads
    _geometry("d64_wide", 64, 4, 600, [1, 64, 65, 128, 129, 256, 257, 512, 513, 600]),   # 8 waves: 64 / 256 / 512
    _geometry("d64", 64, 4, 100, [1, 32, 33, 100]),                                      # 4 waves: 32 / 128 / 256
    # D 256 (4 waves: 8 / 32 / 256): match_attention_chain takes D <= 256 with 64 % (D / 8) == 0; k_attn_streams, k_attn_rows and k_attn_decode at T = 1
    # assert D <= 512. k_attn_blocks asserts ATTN_MAX_T * D <= 512 and k_attn_decode T * D <= 512: D 256 has NO blocks case and no block of T > 2 rows.
    _geometry("d256", 256, 1, 40, [8, 9, 32, 33, 40]),
)}
LONG = _geometry("d128_long", 128, 2, 1200, [384, 385, 1024, 1025, 1200])   # single column only: straddles ATTN_SINGLE_MAX and ATTN_SPLIT_BIG_MIN


def entry_slots(geo):
    return 4 * geo.waves * geo.spw   # ATTN_NPRE passes


def attn_scale(D):
    return float(np.float32(1.0) / np.sqrt(np.float32(D)))   # 1.f / sqrtf((float) D)


# ---- the reference -------------------------------------------------------------------------------------------------------------------------------
def bf16_f32(x):
    return gu.bf16_bits_to_f32(gu.f32_to_bf16_bits(x))


def round_bf16_f64(p):
    """p >= 0 (float64, normal BF16 range) -> (nearest-even BF16 value, the BF16 ulp at p, distance of p to the nearest rounding midpoint)"""
    _, e = np.frexp(p)                      # p in [2^(e-1), 2^e): 8 significant bits -> ulp 2^(e-8)
    ulp = np.ldexp(1.0, e - 8)
    t = p / ulp
    return np.rint(t) * ulp, ulp, np.abs(t - np.floor(t) - 0.5) * ulp


def rope_rows(x, rot):
    """x [H, T, D] f32 interleaved (re, im) pairs, rot [T, D] = cos | sin -> [H, T, D]: the real halves, then the imaginary ones (apply_rope)"""
    half = x.shape[-1] // 2
    re, im = x[..., 0::2], x[..., 1::2]
    c, s = rot[None, :, :half].astype(np.float32), rot[None, :, half:].astype(np.float32)
    return np.concatenate([re * c - im * s, re * s + im * c], axis=-1).astype(np.float32)


def attention_reference(rings_k, rings_v, sequences, variant=None):
    """rings_k / rings_v: BF16 bits [B, H, C, D] (uint16); sequences: Seq tuples in graph order -> Ref. out / slack: one [H, T, D] float64 array per
    sequence. variant (the mutations test_attn_columns_cpu.py must see rejected): "p_unrounded", "q_unrounded", "stale_written" (the slots a sequence
    writes are attended to as they were before), "stale_rows" (a sequence does not see what the previous sequence of its column stored)."""
    kb, vb = np.array(rings_k, dtype=np.uint16), np.array(rings_v, dtype=np.uint16)
    outs, slacks = [], []
    n_live = n_ties = max_row_ties = 0
    max_x = 0.0
    before_prev = {}   # column -> (K, V) bits as they were before the column's previous sequence
    for s in sequences:
        H, T, D = s.q.shape
        q, k = (rope_rows(s.q, s.rot), rope_rows(s.k, s.rot)) if s.rot is not None else (s.q.astype(np.float32), s.k.astype(np.float32))
        old = (kb[s.b].copy(), vb[s.b].copy())
        for t in range(T):   # every row is stored before any row attends; the last writer of a slot wins
            kb[s.b][:, s.idx[t], :] = gu.f32_to_bf16_bits(k[:, t, :])
            vb[s.b][:, s.idx[t], :] = gu.f32_to_bf16_bits(s.v[:, t, :])
        seen_k, seen_v = kb[s.b], vb[s.b]
        if variant == "stale_written":
            seen_k, seen_v = seen_k.copy(), seen_v.copy()
            seen_k[:, s.idx, :], seen_v[:, s.idx, :] = old[0][:, s.idx, :], old[1][:, s.idx, :]
        if variant == "stale_rows" and s.b in before_prev:
            seen_k, seen_v = before_prev[s.b][0].copy(), before_prev[s.b][1].copy()
            seen_k[:, s.idx, :], seen_v[:, s.idx, :] = kb[s.b][:, s.idx, :], vb[s.b][:, s.idx, :]
        before_prev[s.b] = old
        K, V = gu.bf16_bits_to_f32(seen_k).astype(np.float64), gu.bf16_bits_to_f32(seen_v).astype(np.float64)
        qr = (q if variant == "q_unrounded" else bf16_f32(q)).astype(np.float64)
        score = np.einsum("hcd,htd->htc", K, qr).astype(np.float32)
        x = (score * np.float32(attn_scale(D))).astype(np.float32) + s.mask[None].astype(np.float32)
        live = np.isfinite(x)
        assert live.any(axis=-1).all(), "a row with no live slot has no soft_max"
        x64 = np.where(live, x, -np.inf).astype(np.float64)
        e = np.where(live, np.exp(x64 - x64.max(axis=-1, keepdims=True)), 0.0)
        p64 = e / e.sum(axis=-1, keepdims=True)
        p, ulp, dist = round_bf16_f64(p64)
        ax = np.where(live, np.abs(x64), 0.0).max(axis=-1, keepdims=True)
        tau = 2.0 * (4.0 + 2.0 * ax) * 2.0 ** -24
        tie = live & (dist <= tau * p64)
        if variant == "p_unrounded":
            p = p64
        outs.append(np.einsum("htc,hcd->htd", p, V))
        slacks.append(np.einsum("htc,hcd->htd", np.where(tie, ulp, 0.0), np.abs(V)))
        n_live += int(live.sum())
        n_ties += int(tie.sum())
        max_row_ties = max(max_row_ties, int(tie.sum(axis=-1).max()))
        max_x = max(max_x, float(ax.max()))
    return Ref(outs, slacks, kb, vb, n_live, n_ties, max_row_ties, max_x)


def assert_matches(got_out, got_rings, ref, what=""):
    """got_out: one [H, T, D] f32 array per sequence; got_rings: (K bits, V bits) [B, H, C, D] -> worst |got - ref| / max|ref| over the rows that hold no
    near tie (the figure BAR is derived from)"""
    assert len(got_out) == len(ref.out), (what, len(got_out), len(ref.out))
    worst = 0.0
    for i, (g, r, sl) in enumerate(zip(got_out, ref.out, ref.slack)):
        assert g.shape == r.shape, (what, i, g.shape, r.shape)
        assert np.array_equal(np.isfinite(g), np.isfinite(r)), f"{what} sequence {i}: the finite pattern differs"
        scale = float(np.abs(r).max())
        err = np.abs(g.astype(np.float64) - r)
        bad = err > BAR * scale + sl
        assert not bad.any(), (f"{what} sequence {i}: {int(bad.sum())} of {bad.size} elements beyond the bar, worst {float((err - sl).max() / scale):.3e} x max|ref| "
                               f"at (head, row, dim) {np.argwhere(bad)[:4].tolist()}")
        quiet = sl.max(axis=-1) == 0.0   # rows without a near tie
        if quiet.any():
            worst = max(worst, float(err[quiet].max() / scale))
    for name, g, r in (("K", got_rings[0], ref.kbits), ("V", got_rings[1], ref.vbits)):
        assert g.shape == r.shape and g.dtype == np.uint16, (what, name, g.shape, r.shape, g.dtype)
        assert np.array_equal(g, r), f"{what}: {name} ring bytes differ at (column, head, slot, dim) {np.argwhere(g != r)[:4].tolist()} ({int((g != r).sum())} values)"
    return worst


# ---- inputs --------------------------------------------------------------------------------------------------------------------------------------
def rope_row(position, D):
    ang = position * np.exp(-np.log(10000.0) * np.arange(D // 2) / (D // 2))
    return np.concatenate([np.cos(ang), np.sin(ang)]).astype(np.float32)


def live_row(C, n_end, hole=None):
    m = np.full(C, -np.inf, np.float32)
    m[:n_end] = 0.0
    if hole:
        m[hole[0]:hole[1]] = -np.inf
    return m


def causal_block(C, pos, n):
    """causal_mask_block (moshi_hot.cpp): row t is open up to slot pos + t"""
    return np.where(np.arange(C)[None, :] <= pos + np.arange(n)[:, None], 0.0, -np.inf).astype(np.float32)


def bias_pattern_block(C, n, offset):
    """create_bias_pattern + bias_pattern_index (moshi_hot.cpp): the [n, C] window of the lookup table at stream position `offset`"""
    start = 2 * C - n
    width = start + C
    pat = np.zeros((n, width), np.float32)
    for j in range(n):
        pat[j, start + 1 + j:] = -np.inf
        for i in range(n - j - 1):
            pat[j, C - 1 - i] = -np.inf
    col = start - offset if offset <= C else C - (offset % C)
    return pat[:, col:col + C].copy()


def ring_bits(rng, B, H, C, D, live):
    """live [B, C] bool -> BF16 bits [B, H, C, D]: standard normal rows in the live slots, finite rows 64 times larger in the masked ones (a leaked slot is
    gross; no NaN / Inf: ggml's 0 * NaN differs from the device's skip on purpose). Never zero."""
    x = rng.standard_normal((B, H, C, D)).astype(np.float32)
    x = np.where(np.asarray(live)[:, None, :, None], x, 64.0 * x)
    return gu.f32_to_bf16_bits(x)


def qkv_rows(rng, T, H, D):
    """T rows of the projection output [T, 3 * H * D]: q and k of standard deviation 0.4 (the soft-max is not peaked and the new row does not take it
    all), v standard normal"""
    r = rng.standard_normal((T, 3, H * D)).astype(np.float32)
    r[:, :2] *= 0.4
    return r.reshape(T, 3 * H * D)


def heads_of(proj_rows, H, D):
    """[T, 3 H D] -> q, k, v as [H, T, D]"""
    T = proj_rows.shape[0]
    r = proj_rows.reshape(T, 3, H, D).transpose(1, 2, 0, 3)
    return np.ascontiguousarray(r[0]), np.ascontiguousarray(r[1]), np.ascontiguousarray(r[2])


StreamsCase = collections.namedtuple("StreamsCase", "name geo B rope shared proj masks slots positions kbits vbits")


def streams_case(geo, B, n_ends, slots, rope, seed, shared, holes=None, positions=None, name=""):
    """One step of B columns. shared (lockstep): one mask row, ring slot and RoPE phase for all columns - n_ends / slots / positions hold one value.
    holes: per column None or (first, end) of a -inf run inside the live range."""
    rng = np.random.default_rng(seed)
    n = 1 if shared else B
    holes = holes or [None] * n
    masks = np.stack([live_row(geo.C, n_ends[i], holes[i]) for i in range(n)])
    positions = positions if positions is not None else [1000 + 37 * i + n_ends[i] for i in range(n)]   # distinct per column
    live = np.isfinite(masks)
    kbits = ring_bits(rng, B, geo.H, geo.C, geo.D, np.broadcast_to(live, (B, geo.C)))
    vbits = ring_bits(rng, B, geo.H, geo.C, geo.D, np.broadcast_to(live, (B, geo.C)))
    return StreamsCase(name, geo, B, rope, shared, qkv_rows(rng, B, geo.H, geo.D), masks, list(slots), list(positions), kbits, vbits)


def streams_sequences(case, mask_of=None, position_of=None):
    geo = case.geo
    seqs = []
    for b in range(case.B):
        i = 0 if case.shared else b
        q, k, v = heads_of(case.proj[b:b + 1], geo.H, geo.D)
        mi = mask_of(b) if mask_of else i
        pos = position_of(b) if position_of else case.positions[i]
        seqs.append(Seq(b, q, k, v, np.array([case.slots[i]]), case.masks[mi][None], rope_row(pos, geo.D)[None] if case.rope else None))
    return seqs


def column_case(case, b):
    """column b of a streams case as a single-column (B = 1) case"""
    i = 0 if case.shared else b
    return StreamsCase(f"{case.name} column {b}", case.geo, 1, case.rope, True, case.proj[b:b + 1], case.masks[i:i + 1], [case.slots[i]], [case.positions[i]],
                       case.kbits[b:b + 1], case.vbits[b:b + 1])


Job = collections.namedtuple("Job", "b row n pos ordered")
JobsCase = collections.namedtuple("JobsCase", "name geo B rope jobs proj kbits vbits")


def jobs_case(geo, B, jobs, rope, seed, name=""):
    """One pass. jobs: Job(column, first row, rows, stream position before the pass, ring-ordered). Slots below a column's position are its history
    (live); a column's other slots hold the large rows, where its position has not wrapped."""
    rng = np.random.default_rng(seed)
    T = sum(j.n for j in jobs)
    live = np.zeros((B, geo.C), bool)
    live[:, :3] = True
    for j in jobs:
        live[j.b, :min(j.pos, geo.C)] = True
    kbits, vbits = ring_bits(rng, B, geo.H, geo.C, geo.D, live), ring_bits(rng, B, geo.H, geo.C, geo.D, live)
    return JobsCase(name, geo, B, rope, list(jobs), qkv_rows(rng, T, geo.H, geo.D), kbits, vbits)


def job_sequences(job):
    """the attention sequences of a piece (slots_pass_stack): a block piece is one, a ring-ordered piece one per row"""
    if not job.ordered:
        return [job]
    return [Job(job.b, job.row + t, 1, job.pos + t, True) for t in range(job.n)]


def jobs_sequences(case):
    """-> (Seq list in graph order, the first pass row of each)"""
    geo = case.geo
    seqs, rows = [], []
    for job in case.jobs:
        for s in job_sequences(job):
            q, k, v = heads_of(case.proj[s.row:s.row + s.n], geo.H, geo.D)
            rot = np.stack([rope_row(s.pos + t, geo.D) for t in range(s.n)]) if case.rope else None
            seqs.append(Seq(s.b, q, k, v, (s.pos + np.arange(s.n)) % geo.C, causal_block(geo.C, s.pos, s.n), rot))
            rows.append(s.row)
    return seqs, rows


# ---- graphs --------------------------------------------------------------------------------------------------------------------------------------
def _set_raw(g, t, arr):
    raw = np.ascontiguousarray(arr).tobytes()
    assert len(raw) == g.L.ggml_nbytes(t), (len(raw), g.L.ggml_nbytes(t))
    g.L.ggml_backend_tensor_set(t, raw, 0, len(raw))


def _ring_bits_of(g, t, shape):
    return gu.f32_to_bf16_bits(g.get(t)).reshape(shape)   # (BF16 -> float32 -> BF16 is exact)


def _rope_split(g, q, half, Tn, H, B):
    """rope_split (moshi_hot.cpp)"""
    q = g.reshape_4d(g.cont(q), 2, half, Tn, B * H)
    q = g.cont(g.permute(q, 3, 0, 1, 2))
    qc = q.contents
    qr = g.view_3d(q, half, Tn, B * H, qc.nb[1], qc.nb[2], 0)
    qi = g.view_3d(q, half, Tn, B * H, qc.nb[1], qc.nb[2], qc.nb[2] * B * H)
    return g.reshape_4d(qr, half, Tn, H, B), g.reshape_4d(qi, half, Tn, H, B)


def _apply_rope(g, q, k, rotr, roti):
    """apply_rope (moshi_hot.cpp)"""
    c = q.contents
    B, H, Tn, D = int(c.ne[3]), int(c.ne[2]), int(c.ne[1]), int(c.ne[0])
    qr, qi = _rope_split(g, q, D // 2, Tn, H, B)
    kr, ki = _rope_split(g, k, D // 2, Tn, H, B)
    qo = g.concat(g.sub(g.mul(qr, rotr), g.mul(qi, roti)), g.add(g.mul(qr, roti), g.mul(qi, rotr)), 0)
    ko = g.concat(g.sub(g.mul(kr, rotr), g.mul(ki, roti)), g.add(g.mul(kr, roti), g.mul(ki, rotr)), 0)
    return qo, ko


class StreamsGraph:
    """attention() between the projections, on one handle: q / k / v [D, 1, H, B] views of the projected rows [3 H D, 1, B], rings [D, C, H, B].
    per_stream False: the lockstep graph (one shared mask row [C, 1], index of one element, RoPE halves of D / 2) - with B = 1 the single-column graph;
    True: the slots graph (mask [C, 1, 1, B], index [1, 1, B], RoPE halves [D/2, 1, 1, B] of a [D, B] table). Inputs are rewritten between computes: the
    second and later computes replay the captured graph."""

    def __init__(self, kind, geo, B, rope, per_stream, flags=0):
        D, H, C = geo.D, geo.H, geo.C
        self.geo, self.B, self.rope, self.per_stream, self.kind = geo, B, rope, per_stream, kind
        g = self.g = gu.Graph(kind, mem_mb=64)
        if kind == "hip" and flags:
            g.set_flags(flags)
        self.proj = g.new(F32, 3 * H * D, 1, B)
        self.kc, self.vc = g.new(BF16, D, C, H, B), g.new(BF16, D, C, H, B)
        if per_stream:
            self.mask, self.idx = g.new(F32, C, 1, 1, B), g.new(I32, 1, 1, B)
        else:
            self.mask, self.idx = g.new(F32, C, 1), g.new(I32, 1)
        rotr = roti = None
        if rope:
            if per_stream:
                self.rot = g.new(F32, D, B)
                nb1 = self.rot.contents.nb[1]
                rotr = g.view_4d(self.rot, D // 2, 1, 1, B, nb1, nb1, nb1, 0)
                roti = g.view_4d(self.rot, D // 2, 1, 1, B, nb1, nb1, nb1, 4 * (D // 2))
            else:
                self.rot = g.new(F32, D, 1)
                nb1 = self.rot.contents.nb[1]
                rotr, roti = g.view_2d(self.rot, D // 2, 1, nb1, 0), g.view_2d(self.rot, D // 2, 1, nb1, 4 * (D // 2))
        p = self.proj.contents

        def third(i):
            t = g.cont(g.view_3d(self.proj, p.ne[0] // 3, p.ne[1], p.ne[2], p.nb[1], p.nb[2], i * (p.nb[1] // 3)))
            t = g.reshape_4d(t, D, H, t.contents.ne[1], t.contents.ne[2])
            return g.permute(t, 0, 2, 1, 3)

        q, k, v = third(0), third(1), third(2)
        if rope:
            q, k = _apply_rope(g, q, k, rotr, roti)
        k = g.set_rows(self.kc, k, self.idx)
        v = g.set_rows(self.vc, v, self.idx)
        w = g.soft_max_ext(g.mul_mat(k, q), self.mask, attn_scale(D), 0.0)
        o = g.mul_mat(g.cont(g.transpose(v)), w)
        self.out = g.cont(g.permute(o, 0, 2, 1, 3))   # [D, H, 1, B]
        g.build([self.out])
        g.alloc()

    def run(self, case):
        """-> ([per column [H, 1, D]], (K bits, V bits))"""
        g, geo, B = self.g, self.geo, self.B
        assert case.geo == geo and case.B == B and case.rope == self.rope and (case.shared or self.per_stream)
        n = B if self.per_stream else 1
        pick = (lambda a: [a[0]] * n) if case.shared else (lambda a: list(a))
        _set_raw(g, self.proj, case.proj.astype(np.float32))
        _set_raw(g, self.kc, case.kbits)
        _set_raw(g, self.vc, case.vbits)
        _set_raw(g, self.mask, np.stack(pick(case.masks)).astype(np.float32))
        _set_raw(g, self.idx, np.array(pick(case.slots), np.int32))
        if self.rope:
            _set_raw(g, self.rot, np.stack([rope_row(p, geo.D) for p in pick(case.positions)]))
        g.compute()
        out = g.get(self.out).reshape(B, geo.H, 1, geo.D)
        shape = (B, geo.H, geo.C, geo.D)
        return [out[b] for b in range(B)], (_ring_bits_of(g, self.kc, shape), _ring_bits_of(g, self.vc, shape))

    def stats(self):
        return self.g.stats()

    def free(self):
        self.g.free()


class JobsGraph:
    """attention_jobs() between the projections, for one pass shape: `projected` [3 H D, T], per attention sequence the rows' q / k / v views, RoPE, the
    [D, C, H] view of its ring column, set_rows at the sequence's slots, the masked soft_max, P x V and the copy into its rows of one [D, H, T] tensor
    (negative view offsets as the driver's). A pass with ring-ordered rows expands every sequence into the graph before the next one is built. Mask
    blocks, ring slots and RoPE rows are uploaded constants, created ahead of the sequences in the driver's order (mask, slots, RoPE per sequence)."""
    U64 = 1 << 64

    def __init__(self, kind, case, flags=0):
        geo = case.geo
        D, H, C, B = geo.D, geo.H, geo.C, case.B
        self.case, self.kind = case, kind
        g = self.g = gu.Graph(kind, mem_mb=96, graph_size=8192)
        if kind == "hip" and flags:
            g.set_flags(flags)
        L = g.L
        T = case.proj.shape[0]
        self.T = T
        self.proj = g.input(case.proj.astype(np.float32))   # [3 H D, T]
        self.kc = g.input_raw(case.kbits, BF16, D, C, H, B)
        self.vc = g.input_raw(case.vbits, BF16, D, C, H, B)
        seqs, _ = jobs_sequences(case)
        self.seq_jobs = [s for job in case.jobs for s in job_sequences(job)]
        any_ordered = any(j.ordered for j in case.jobs)
        consts = []
        for s in seqs:
            mask = g.input(s.mask)                       # [C, n]
            idx = g.input(s.idx.astype(np.int32), I32)   # [n]
            rot = g.input(s.rot) if case.rope else None  # [D, n]
            consts.append((mask, idx, rot))
        g.graph = L.ggml_new_graph_custom(g.ctx, g.graph_size, False)
        halves = []
        for (_, _, rot), s in zip(consts, self.seq_jobs):
            if rot is None:
                halves.append((None, None))
                continue
            nb1 = rot.contents.nb[1]
            rotr, roti = g.view_2d(rot, D // 2, s.n, nb1, 0), g.view_2d(rot, D // 2, s.n, nb1, 4 * (D // 2))
            halves.append((rotr, roti))
            if any_ordered:
                L.ggml_build_forward_expand(g.graph, rotr)
        p = self.proj.contents
        row_nb, out_row = p.nb[1], D * H * 4
        out = g.new(F32, D, H, T)
        out_at = 0
        kcc, vcc = self.kc.contents, self.vc.contents
        for (mask, idx, _), (rotr, roti), s in zip(consts, halves, self.seq_jobs):
            def rows(off):
                t = g.cont(g.view_3d(self.proj, p.ne[0] // 3, s.n, 1, row_nb, row_nb * s.n, s.row * row_nb + off))
                return g.permute(g.reshape_4d(t, D, H, s.n, 1), 0, 2, 1, 3)
            q, k, v = rows(0), rows(row_nb // 3), rows(row_nb * 2 // 3)
            if case.rope:
                q, k = _apply_rope(g, q, k, rotr, roti)
            kring = g.view_3d(self.kc, D, C, H, kcc.nb[1], kcc.nb[2], s.b * kcc.nb[3])
            vring = g.view_3d(self.vc, D, C, H, vcc.nb[1], vcc.nb[2], s.b * vcc.nb[3])
            k = g.set_rows(kring, k, idx)
            v = g.set_rows(vring, v, idx)
            w = g.soft_max_ext(g.mul_mat(k, q), mask, attn_scale(D), 0.0)
            o = g.mul_mat(g.cont(g.transpose(v)), w)
            dst = g.view_3d(out, D, H, s.n, D * 4, out_row, ((s.row - out_at) * out_row) % self.U64)
            out = g.cpy(g.permute(o, 0, 2, 1, 3), dst)
            out_at = s.row
            if any_ordered:
                L.ggml_build_forward_expand(g.graph, out)
        self.consts = consts
        self.all = g.view_3d(out, D * H, T, 1, out_row, out_row * T, (-out_at * out_row) % self.U64)
        L.ggml_build_forward_expand(g.graph, self.all)
        g.alloc()

    def set_sequence(self, i, seq):
        """sequence i's uploaded constants <- another sequence's of the same shape (its mask block, ring slots and RoPE rows)"""
        mask, idx, rot = self.consts[i]
        _set_raw(self.g, mask, seq.mask.astype(np.float32))
        _set_raw(self.g, idx, np.asarray(seq.idx, np.int32))
        if rot is not None:
            _set_raw(self.g, rot, seq.rot.astype(np.float32))

    def run(self, proj=None, rings=None):
        """(inputs may be rewritten: the handle then replays) -> ([per sequence [H, n, D]], (K bits, V bits))"""
        g, geo = self.g, self.case.geo
        if proj is not None:
            _set_raw(g, self.proj, proj.astype(np.float32))
        if rings is not None:
            _set_raw(g, self.kc, rings[0])
            _set_raw(g, self.vc, rings[1])
        g.compute()
        x = g.get(self.all).reshape(self.T, geo.H, geo.D)
        shape = (self.case.B, geo.H, geo.C, geo.D)
        outs = [np.ascontiguousarray(x[s.row:s.row + s.n].transpose(1, 0, 2)) for s in self.seq_jobs]
        return outs, (_ring_bits_of(g, self.kc, shape), _ring_bits_of(g, self.vc, shape))

    def stats(self):
        return self.g.stats()

    def free(self):
        self.g.free()


def jobs_reference(case, variant=None):
    seqs, _ = jobs_sequences(case)
    return attention_reference(case.kbits, case.vbits, seqs, variant)


def streams_reference(case, variant=None, **kw):
    return attention_reference(case.kbits, case.vbits, streams_sequences(case, **kw), variant)


# ---- the case table ------------------------------------------------------------------------------------------------------------------------------
def lockstep_cases(geo, B=3, rope=True):
    """every n_end of the table x written slot in {last live, 0, middle}"""
    cases = []
    for n in geo.n_ends:
        for slot in sorted({n - 1, 0, n // 2}):
            cases.append(streams_case(geo, B, [n], [slot], rope, seed=7 * n + slot + (1 if rope else 0), shared=True, name=f"{geo.name} lockstep n_end {n} slot {slot} rope {int(rope)}"))
    return cases


def slots_cases(geo, rope=True):
    """B = 3 in one launch: column 0 at the table's n_end, column 1 at live length 1, column 2 with a full ring; the written slot in the middle (the
    wrapped state); one case with a -inf hole inside the live range; one with the written slot outside the live range (written, not attended)."""
    C = geo.C
    cases = []
    for n in geo.n_ends:
        cases.append(streams_case(geo, 3, [n, 1, C], [n // 2, 0, C // 2], rope, seed=1000 + n, shared=False, name=f"{geo.name} slots n_end {n}"))
    n = geo.n_ends[-2]
    hole = (n // 3, n // 3 + max(1, n // 4))
    cases.append(streams_case(geo, 3, [n, 1, C], [n - 1, 0, C // 2], rope, seed=2000, shared=False, holes=[hole, None, (1, C - 1)], name=f"{geo.name} slots hole {hole} in {n}"))
    cases.append(streams_case(geo, 3, [n, 1, C], [min(n + 2, C - 1), 1, C // 2], rope, seed=2001, shared=False, holes=[None, None, (C // 2, C // 2 + 1)],
                              name=f"{geo.name} slots written outside the live range"))
    return cases


def same_position_case(geo, n, rope=True):
    """a lockstep case: the slots graph at one position in every column must give its bits"""
    return streams_case(geo, 3, [n], [n - 1], rope, seed=3000 + n, shared=True, name=f"{geo.name} one position n_end {n}")


def single_cases(geo, rope=True):
    return [streams_case(geo, 1, [n], [slot], rope, seed=4000 + 3 * n + slot % 3, shared=True, name=f"{geo.name} single n_end {n} slot {slot}")
            for n in geo.n_ends for slot in sorted({n - 1, 0, n // 2})]


def blocks_cases(geo, rope=True):
    """3 ring columns (17 for the seventeen one-row jobs: a launch pair never holds two jobs of one column). Positions are greater than 0 and such that a
    block crosses the entry-prefetch bound where the ring is long enough."""
    assert 4 * geo.D <= 512, "k_attn_blocks: ATTN_MAX_T * D <= 2 * ATTN_NW_BASE * 64"
    C = geo.C
    edge = min(entry_slots(geo), C - 13) - 4   # 13 rows from here cross the bound (or end 4 slots before the ring's end)
    big = min(edge, C - 64)                    # 64 rows fit behind it
    cases = [
        jobs_case(geo, 3, [Job(2, 0, 1, edge + 3, False), Job(0, 1, 4, edge + 1, False), Job(1, 5, 5, 12, False)], rope, 5000, f"{geo.name} blocks 1 + 4 + 5 rows"),
        jobs_case(geo, 3, [Job(1, 0, 13, edge, False)], rope, 5001, f"{geo.name} blocks 13 rows at {edge}"),
        jobs_case(geo, 3, [Job(0, 0, 64, big, False)], rope, 5002, f"{geo.name} blocks 64 rows at {big}"),
        jobs_case(geo, 17, [Job(b, b, 1, (edge - 8 + 5 * b) % (C - 1) + 1, False) for b in range(17)], rope, 5003, f"{geo.name} blocks 17 one-row jobs"),
    ]
    for c in cases:
        for j in c.jobs:
            assert j.pos > 0 and j.pos + j.n <= C, (c.name, j)
    return cases


def blocks_expect(case):
    """(attention block launches, jobs) of the plan: a pair per ATTN_BLOCKS_MAX = 16 jobs"""
    n = len(case.jobs)
    return 2 * ((n + 15) // 16), n


def rows_cases(geo, rope=True):
    """ring-ordered pieces: a column at position C - 3 taking 8 rows across the wrap beside a column taking 16 rows (RING_ORDERED_ROWS_MAX) - two columns'
    jobs in one launch; a block piece and a ring-ordered piece in one pass. Every row's mask includes the slot the previous row wrote."""
    C = geo.C
    cases = [jobs_case(geo, 3, [Job(0, 0, 8, C - 3, True), Job(1, 8, 16, 2 * C + 5, True)], rope, 6000, f"{geo.name} rows 8 across the wrap + 16")]
    if 4 * geo.D <= 512:   # (the block piece is a k_attn_blocks job)
        cases.append(jobs_case(geo, 3, [Job(2, 0, 5, min(entry_slots(geo), C - 5) - 2, False), Job(0, 5, 6, C + 7, True)], rope, 6001, f"{geo.name} rows 6 beside a block of 5"))
    return cases


def rows_expect(case):
    """(block launches, block jobs, row launches, row jobs, row rows)"""
    blocks = [j for j in case.jobs if not j.ordered]
    ordered = [j for j in case.jobs if j.ordered]
    return 2 * (1 if blocks else 0), len(blocks), 1 if ordered else 0, len(ordered), sum(j.n for j in ordered)
