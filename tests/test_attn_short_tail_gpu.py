"""The short-ring form of the attention tail of the merged in_proj + attention launch (attn_short_tail, moshi.cpp_amd/csrc/hip_attn_body.h, entered from
attn_decode_body<.., AT_GQKV> inside inproj_attn_kernel) and the live-length scan that now runs in front of the granule poll.

The form is entered block-uniformly when a head's live range ends at or below ATTN_SHORT_MAX = 128 ring slots; it must compute the general body's BITS.
Every case runs the same graph - norm1 -> in_proj (Q4_K) -> RoPE -> ring write -> attention over the ring, built node for node like the model's
attention() - on three handles: the merged launch with the form (default), the merged launch with the general body at every live length (backend
flag 2048, what MI355X_ATTN_SHORT_TAIL=0 selects), and separate launches (flag 512). Attention output and the K / V ring bytes must be identical.

Shapes: the smallest the merged launch accepts - 32 heads of 128 over K = 1024 (one activation batch per thread) and 8 heads of 128 over K = 4096 (two) -
with a ring of C = 172 slots (4 x 128 / 3 rounded up to a multiple of 4: both sides of the bound are reachable, the split path is not). The model-level
test crosses the bound inside one replayed hipGraph, at the ring of 172 and at a ring of 1 200 (the split instantiation of the kernel)."""
import hashlib

import numpy as np
import pytest

import ggml_util as gu
from ggml_util import BF16, I32, Q4_K

pytestmark = pytest.mark.gpu

SHORT_MAX = 128
D = 128
C_RING = (4 * SHORT_MAX // 3 + 1 + 3) // 4 * 4
FLAG_GENERAL, FLAG_SEPARATE = 2048, 512


class Block:
    """One in_proj + attention block on its own backend handle; inputs are rewritten between computes (the second compute on captures a hipGraph)."""

    def __init__(self, H, K, C, flags, seed):
        r = np.random.default_rng(seed)
        g = self.g = gu.Graph("hip", mem_mb=64)
        if flags:
            g.set_flags(flags)
        HD = H * D
        self.H, self.K, self.C = H, K, C
        self.x = g.input(np.zeros((1, K), np.float32))
        # (q / k / v rows of order 0.4 under ggml_util's synthetic Q4_K rows: the row written this step does not take the whole soft-max)
        alpha = g.input(((1.0 + 0.1 * r.standard_normal((1, K))) / (11.0 * np.sqrt(K))).astype(np.float32))
        w = g.input_raw(gu.random_q4_K(r, 3 * HD, K), Q4_K, K, 3 * HD)
        self.rot = g.input(np.zeros((1, D), np.float32))
        self.mask = g.input(np.zeros((1, C), np.float32))
        self.idx = g.input(np.zeros(1, np.int32), I32)
        self.kc = g.input(r.standard_normal((H, C, D)).astype(np.float32), BF16)
        self.vc = g.input(r.standard_normal((H, C, D)).astype(np.float32), BF16)

        proj = g.mul_mat(w, g.mul(alpha, g.rms_norm(self.x, 1e-8)))
        p = proj.contents

        def segment(i):
            t = g.cont(g.view_3d(proj, HD, p.ne[1], p.ne[2], p.nb[1], p.nb[2], i * HD * 4))
            t = g.reshape_4d(t, D, H, t.contents.ne[1], t.contents.ne[2])
            return g.permute(t, 0, 2, 1, 3)

        q, k, v = segment(0), segment(1), segment(2)
        nb1 = self.rot.contents.nb[1]
        rotr, roti = g.view_2d(self.rot, D // 2, 1, nb1, 0), g.view_2d(self.rot, D // 2, 1, nb1, 4 * (D // 2))

        def split(t):
            t = g.reshape_4d(g.cont(t), 2, D // 2, 1, H)
            t = g.cont(g.permute(t, 3, 0, 1, 2))
            tt = t.contents
            re = g.view_3d(t, D // 2, 1, H, tt.nb[1], tt.nb[2], 0)
            im = g.view_3d(t, D // 2, 1, H, tt.nb[1], tt.nb[2], tt.nb[2] * H)
            return g.reshape_4d(re, D // 2, 1, H, 1), g.reshape_4d(im, D // 2, 1, H, 1)

        def rope(t):
            re, im = split(t)
            return g.concat(g.sub(g.mul(re, rotr), g.mul(im, roti)), g.add(g.mul(re, roti), g.mul(im, rotr)), 0)

        q, k = rope(q), rope(k)
        k = g.set_rows(self.kc, k, self.idx)
        v = g.set_rows(self.vc, v, self.idx)
        wgt = g.soft_max_ext(g.mul_mat(k, q), self.mask, 1.0 / np.sqrt(D), 0.0)
        o = g.mul_mat(g.cont(g.transpose(v)), wgt)
        self.out = g.cont(g.permute(o, 0, 2, 1, 3))
        g.build([self.out])
        g.alloc()

    def step(self, x, mask_row, slot, position):
        g = self.g
        g.set(self.x, x)
        g.set(self.mask, mask_row)
        g.set(self.idx, np.array([slot], np.int32))
        ang = position * np.exp(-np.log(10000.0) * np.arange(D // 2) / (D // 2))
        g.set(self.rot, np.concatenate([np.cos(ang), np.sin(ang)]).astype(np.float32)[None])
        g.compute()
        return g.get(self.out), g.get(self.kc), g.get(self.vc)

    def free(self):
        self.g.free()


def live_mask(n, C=C_RING):
    m = np.full((1, C), -np.inf, np.float32)
    m[0, :n] = 0.0
    return m


def holed_mask(n_end, hole):
    m = live_mask(n_end)
    m[0, hole[0]:hole[1]] = -np.inf
    assert np.isfinite(m[0, n_end - 1]) and not np.isfinite(m[0, hole[0]])
    return m


LIVE = [1, 2, 63, 64, 65, SHORT_MAX - 1, SHORT_MAX, SHORT_MAX + 1, C_RING]
HOLES = [(100, (40, 52)), (121, (60, 120)), (SHORT_MAX, (1, 127)), (SHORT_MAX + 1, (64, 128)), (66, (0, 65))]
CROSSING = [SHORT_MAX - 6 + i for i in range(12)]
# every step of a shape's run, in order: (name, mask row, slot written). The slot written this step: slot 0, the last live slot, a slot inside the range
# (last writer wins: the row comes from LDS, not from the ring); with a hole: the last live slot and a slot inside the hole (written, not attended to).
STEPS = [(f"live {n} slot {slot}", live_mask(n), slot) for n in LIVE for slot in sorted({0, n - 1, n // 2})]
STEPS += [(f"hole {n_end} {hole} slot {slot}", holed_mask(n_end, hole), slot) for n_end, hole in HOLES for slot in (n_end - 1, hole[0])]
STEPS += [(f"crossing {n}", live_mask(n), n - 1) for n in CROSSING]      # consecutive launches of the one captured graph on either side of the bound


def run_steps(H, K, flags):
    """All STEPS on one handle (only one handle of a device may plan launches whose workgroups wait for each other, so the three runs are consecutive).
    -> {name: (attention output, K ring digest, V ring digest)}, the handle's statistics"""
    b = Block(H, K, C_RING, flags, seed=17 + H)
    rng = np.random.default_rng(1000 + H)
    res = {}
    for i, (name, mask_row, slot) in enumerate(STEPS):
        out, kc, vc = b.step(rng.standard_normal((1, K)).astype(np.float32), mask_row, slot, i + 1)
        res[name] = (out, hashlib.blake2b(kc.tobytes()).digest(), hashlib.blake2b(vc.tobytes()).digest())
    st = b.g.stats()
    b.free()
    return res, (st.attention_folds_planned, st.graph_replays)


@pytest.fixture(scope="module", params=[(32, 1024), (8, 4096)], ids=["32_heads_K_1024", "8_heads_K_4096"])
def runs(request):
    H, K = request.param
    return {name: run_steps(H, K, flags) for name, flags in (("short", 0), ("general", FLAG_GENERAL), ("separate", FLAG_SEPARATE))}


def check(runs, step):
    short = runs["short"][0][step]
    assert np.isfinite(short[0]).all() and np.abs(short[0]).max() > 0, step
    for other in ("general", "separate"):
        got = runs[other][0][step]
        assert np.array_equal(short[0].view(np.uint32), got[0].view(np.uint32)), f"{step}: attention output differs from the {other} run at {np.argwhere(short[0] != got[0])[:4].tolist()}"
        assert short[1] == got[1] and short[2] == got[2], f"{step}: K / V ring bytes differ from the {other} run"


def test_ring_capacity_puts_both_forms_within_reach_and_the_launch_is_merged(runs):
    assert C_RING == 172 and C_RING % 4 == 0 and SHORT_MAX < C_RING < 1024      # below ATTN_SPLIT_MIN_C: one workgroup per head
    planned = {name: r[1][0] for name, r in runs.items()}
    assert planned["short"] >= 1 and planned["general"] >= 1 and planned["separate"] == 0, planned
    assert runs["short"][1][1] > 0 and runs["general"][1][1] > 0                  # (replayed from a captured graph)


@pytest.mark.parametrize("n", LIVE)
def test_live_lengths_and_written_slots_bit_for_bit(runs, n):
    for slot in sorted({0, n - 1, n // 2}):
        check(runs, f"live {n} slot {slot}")


@pytest.mark.parametrize("n_end,hole", HOLES)
def test_mask_with_a_hole_inside_the_live_range(runs, n_end, hole):
    # n_end is the LAST live slot + 1, not a count of live slots: a live slot behind a -inf hole keeps the range long
    for slot in (n_end - 1, hole[0]):
        check(runs, f"hole {n_end} {hole} slot {slot}")


def test_twelve_steps_across_the_bound_on_one_replayed_graph(runs):
    # live length 122 .. 133, each step writing the slot it adds: the form changes between launches of one captured graph
    for n in CROSSING:
        check(runs, f"crossing {n}")


@pytest.mark.parametrize("context", [C_RING, 1200])
def test_model_frames_across_the_bound_tokens_and_rings(context):
    # twelve frames of a two-layer Temporal stack from 122 live slots on: tokens, logits, stack output and ring bytes against the general body; the ring of
    # 1 200 runs the split instantiation of the kernel (one workgroup per head below ATTN_SINGLE_MAX live slots)
    import hot_util as hu
    import test_attn_fold as taf
    cfg = taf.temporal_cfg(context)

    def run(flags):
        m = hu.Model("hip", cfg, seed=0, flags=flags)
        hu.L.moshi_hot_fill_ring(m.m, 0, -1, 11, 1.0)
        hu.L.moshi_hot_set_context_fill(m.m, SHORT_MAX - 6)
        rng = np.random.default_rng(3)
        rec = []
        for _ in range(12):
            r, txt, aud = m.lm_step(rng.integers(0, cfg.card, cfg.n_q - cfg.io_dep_q).tolist())
            rec.append((r, txt, aud, m.read("text_logits", cfg.text_card).copy(), m.read("stack_out", cfg.dim).copy()))
        rings = m.rings()
        st = m.stats()
        m.free()
        return rec, rings, st

    short, rings_s, st = run(0)
    general, rings_g, st_g = run(FLAG_GENERAL)
    assert st.attention_folds_planned >= cfg.num_layers and st_g.attention_folds_planned >= cfg.num_layers and st.graph_replays > 0
    taf.assert_same(general, short, f"context {context}")
    assert len(rings_s) == len(rings_g) and len(rings_s) > 0
    for (layer, kv, a), (_, _, b) in zip(rings_s, rings_g):
        assert np.array_equal(a, b), f"context {context}: layer {layer} {'KV'[kv]} ring differs"
