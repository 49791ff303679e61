"""-m gpu: per-conversation sampling on the MI355X. The B-column sampler (sample_topk_streams_kernel: one launch per sampler site, one workgroup per
column, per-column temperature and top-k) against the oracle's node chain at the op level; seeded slots models against the oracle's slots model over
whole frames; the sampled Depth plan's launch count."""
import numpy as np
import pytest

import ggml_util as gu
import hot_util as hu
import sampling_util as sp
import slots_util as sl
import streams_util as su
from ggml_util import BF16, F32, I32, Q4_0, Q4_K, Q8_0

pytestmark = pytest.mark.gpu
L = hu.L
RING = 8


def sampler_graph(logits, noise, k, temps=None, temp=0.8, with_cpy=False):
    """moshi_hot.cpp's sample_tokens_streams over given logits [B, n] and noise [B, k]: the `scale` form (one temperature) or, with temps = B
    values, the `mul` by a [1, B] input"""
    B, n = logits.shape

    def build(g):
        l2 = g.reshape_2d(g.input(logits.reshape(B, 1, n)), n, B)
        if temps is None:
            sc = g.scale(l2, np.float32(1.0) / np.float32(temp))
        else:
            sc = g.mul(l2, g.input((np.float32(1.0) / np.asarray(temps, np.float32)).reshape(B, 1)))
        probs = g.soft_max(sc)
        indices = g.cont(g.argsort_top_k(probs, k))
        rows = g.cont(g.permute(g.reshape_3d(probs, n, 1, B), 1, 0, 2, 3))
        in2 = g.reshape_2d(g.get_rows(rows, indices), k, B)
        nxt = g.argmax(g.div(in2, g.input(noise)))
        irows = g.cont(g.permute(g.reshape_3d(indices, k, 1, B), 1, 0, 2, 3))
        tok = g.reshape_1d(g.get_rows(irows, g.reshape_2d(nxt, 1, B)), B)
        if with_cpy:   # the Depth graph copies the B tokens into its token vector
            return [tok, g.cpy(tok, g.new(I32, B))]
        return [tok]
    return build


def hard_logits(r, B, n, k):
    """random rows, and per column one of the difficult rows of tests/test_hip_ops.py test_fused_sampler_matches_the_node_chain"""
    logits = (r.standard_normal((B, n)) * 3).astype(np.float32)
    for b in range(B):
        case = (b + B) % 5
        if case == 0:      # hundreds of equal values straddling the k-th place, and an exact tie for first place
            logits[b, r.integers(0, n, min(600, n // 2))] = np.float32(1.25)
            logits[b, 5] = logits[b, n - 100] = logits[b].max()
        elif case == 1:    # one dominant logit: most probabilities underflow to 0 (ties at zero: lower index first)
            logits[b] *= 40
        elif case == 2:    # all equal
            logits[b] = np.float32(0.5)
        elif case == 3:    # exact zeros from index 200 on
            logits[b, 200:] = -1e4
    return logits


@pytest.mark.parametrize("form", ["scale", "mul"])
@pytest.mark.parametrize("B", [2, 3, 8, 16])
@pytest.mark.parametrize("n,k", [(2048, 250), (32000, 25), (300, 40)])
def test_b_column_sampler_is_one_launch_and_matches_the_node_chain(n, k, B, form):
    r = np.random.default_rng(n + 7 * k + B)
    logits = hard_logits(r, B, n, k)
    temps = None if form == "scale" else [0.5 + 0.13 * b for b in range(B)]
    for draw in range(2):
        noise = r.exponential(1.0, (B, k)).astype(np.float32)
        for b in range(1, B, 2):                             # a smaller top-k in every other column: infinite noise past it
            noise[b, max(1, k // (b + 2)):] = np.inf
        build = sampler_graph(logits, noise, k, temps, with_cpy=bool(draw))
        ref, got, st = gu.compare(build)
        assert st.kernels_in_last_plan == 1, f"{st.kernels_in_last_plan} launches for one B-column sampler site"
        if draw:
            assert np.array_equal(got[0], got[1])
        for b in range(1, B, 2):                             # the token lies inside the column's own top-k: its logit is not below the top_b-th largest
            top_b, t = max(1, k // (b + 2)), 0.8 if temps is None else temps[b]
            kth = np.sort(logits[b].astype(np.float64))[::-1][top_b - 1]
            assert logits[b, got[0].reshape(-1)[b]] / t >= kth / t - 1e-3, (b, top_b)
        plain, _ = gu.run_graph("hip", build, flags=1)
        assert np.array_equal(plain[0], ref[0])


@pytest.mark.parametrize("n,k,B", [(300, 40, 17), (400, 300, 3)])
def test_graphs_outside_the_matcher_run_the_generic_chain(n, k, B):
    # B above SAMPLE_MAX_B / k above SAMPLE_MAX_K: the matcher declines, the node chain runs and gives the oracle's tokens
    r = np.random.default_rng(n + B)
    logits = hard_logits(r, B, n, k)
    noise = r.exponential(1.0, (B, k)).astype(np.float32)
    noise[1, 3:] = np.inf
    for temps in (None, [0.6 + 0.05 * b for b in range(B)]):
        ref, got, st = gu.compare(sampler_graph(logits, noise, k, temps))
        assert st.kernels_in_last_plan > 1


def tiny_slots(lt, et):
    cfg = su.lm_only(hu.hot.tiny(L, linear_type=lt, embed_type=et, context=RING))
    cfg.update_scale = 1.0 / 256   # contractive (include/moshi_hot.h), as every sampled device test: rounding flips stay local
    return sp.sampled(cfg)


def staggered_events(B):
    """as tests/test_slots_gpu.py: slot b opens at frame b (B - 1 stays closed at B = 8); slot 0 is reopened after its conversation ran past the
    8-slot ring's wrap; slot 1 (B = 3) / slot 3 (B = 8) is closed before its ring filled and reopened later"""
    ev = {}
    for b in range(B if B <= 3 else B - 1):
        ev.setdefault(b, []).append(("open", b))
    ev.setdefault(RING + 2, []).extend([("close", 0), ("open", 0)])
    short = 1 if B <= 3 else 3
    ev.setdefault(short + 5, []).append(("close", short))
    ev.setdefault(short + 8, []).append(("open", short))
    return ev


def slot_sampling(b):
    """a seed, temperatures and top-k values per slot; every third slot samples from fewer ranks than the configuration's 20 / 25"""
    return (4000 + 17 * b, 0.6 + 0.1 * (b % 5), 0.5 + 0.1 * (b % 4), 20 if b % 3 else 6, 25 if b % 3 != 1 else 4)


def run_seeded_slots(kind, cfg, B, codes, events):
    s = sp.Slots(kind, cfg, B, seed=0)
    for b in range(B):
        assert s.set_sampling(b, *slot_sampling(b)) == 0
    rec = sl.run_slots(s, codes, events)
    st = s.stats() if kind == "hip" else None
    s.free()
    return rec, st


@pytest.mark.parametrize("B", [3, 8])
@pytest.mark.parametrize("lt,et", [(Q4_K, Q4_0), (Q8_0, Q8_0), (BF16, BF16), (F32, F32)])
def test_seeded_slots_match_the_oracle_slots_model(lt, et, B):
    """No frame is left out: 0 of the B x 18 slot-frames of each case are excused as near ties (the cap would be 5 %)."""
    cfg = tiny_slots(lt, et)
    n = 2 * RING + 2
    codes = sl.slot_codes(cfg, B, n, seed=B)
    events = staggered_events(B)
    ref, _ = run_seeded_slots("oracle", cfg, B, codes, events)
    got, _ = run_seeded_slots("hip", cfg, B, codes, events)
    bad = [i for i, (a, b) in enumerate(zip(ref, got)) if a[:4] != b[:4]]
    for i in bad[:3]:
        print(f"frame {i}: oracle {ref[i][:4]} vs hip {got[i][:4]}")
    assert not bad, f"{len(bad)} of {n} frames differ, first at frame {bad[0]}"
    texts = {t for r in ref for t in r[2] if t >= 0}
    assert len(texts) > 1 and any(r[0] > 0 for r in ref)


def test_sampled_depth_plan_has_one_launch_per_sampler_site():
    cfg = tiny_slots(Q4_K, Q4_0)
    B = 8
    s = sp.Slots("hip", cfg, B)
    codes = sl.slot_codes(cfg, B, 4, seed=2)
    for b in range(B):
        s.open(b)
        assert s.set_sampling(b, *slot_sampling(b)) == 0
    for fr in codes:
        s.step(fr)
    depth = s.stats().kernels_in_last_plan                   # the Depth graph is the last graph of a step
    assert L.ggml_backend_graph_compute(s.be, L.moshi_hot_graph(s.m, 0)) == 0
    temporal = s.stats().kernels_in_last_plan
    s.free()
    print(f"sampled B = 8 tiny slots: {depth} launches in the Depth plan, {temporal} in the Temporal plan")
    # Per Depth step: the chained embedding row (get_rows, cast), depformer_in with its add, 6 launches per layer as in the Temporal bound of
    # tests/test_slots_gpu.py (6 * num_layers + 8), the logits mat-vec and ONE sampler launch that also writes the token vector: 6 * dep_layers + 6.
    # As a node chain the sampler alone was about ten launches a step (scale, soft_max, argsort, cont, cont, get_rows, div, argmax, cont, get_rows),
    # which this bound has no room for: dep_q * 10 more.
    bound = cfg.dep_q * (6 * cfg.dep_layers + 6)
    assert depth <= bound, f"{depth} launches in the sampled Depth plan (bound {bound})"
    assert temporal <= 6 * cfg.num_layers + 8, f"{temporal} launches in the sampled Temporal plan"
