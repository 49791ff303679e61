"""GPU: a tiny moshika-shaped slots model over Q8_0 K / V rings with the split step attention (kv_q8 = 11), B = 2, ring of 640 (three
chunks): a slot takes a 300-frame history in one moshi_hot_slots_prefill call, then 8 greedy frames - the live range crosses the first chunk border -
give the oracle's tokens, every Temporal layer of the step plan being one k_attn_streams_q8_split launch pair; kv_q8 = 3 gives the same tokens with one
k_attn_streams_q8 launch per layer."""
import pytest

import hot_util as hu
import slot_prefill_util as pu
import slot_state_util as ss
import streams_util as su

pytestmark = pytest.mark.gpu
RING, B, N_HIST, N_LIVE = 640, 2, 300, 8


def run(kind, kv_q8):
    cfg = su.lm_only(hu.hot.tiny(hu.L, context=RING))
    cfg.update_scale = 1.0 / 256   # (include/moshi_hot.h) rounding flips stay local instead of compounding over free-running frames
    cfg.kv_q8 = kv_q8
    s = ss.Slots(kind, cfg, B, seed=5)
    hist, live, other = pu.history(cfg, N_HIST, seed=41), pu.live_codes(cfg, N_LIVE, seed=51), pu.live_codes(cfg, N_LIVE, seed=52)
    assert s.open(0) == 0 and s.open(1) == 0
    assert s.prefill([(1, hist)]) == N_HIST
    out = [pu.step_all(s, {0: other[k], 1: live[k]})[:4] for k in range(N_LIVE)]
    plan = None
    if kind == "hip":
        assert hu.L.ggml_backend_graph_compute(s.be, hu.L.moshi_hot_graph(s.m, 0)) == 0   # the Temporal graph once more on its own: its plan is the last one
        plan = s.stats()
    s.free()
    return cfg, out, plan


def test_split_step_attention_gives_the_oracles_tokens_one_launch_pair_per_layer():
    (cfg, split, sp), (_, whole, wp), (_, ref, _) = run("hip", 11), run("hip", 3), run("oracle", 11)
    assert (sp.q8_attention_split_blocks_in_last_plan, sp.q8_attention_blocks_in_last_plan) == (cfg.num_layers, 0)
    assert (wp.q8_attention_split_blocks_in_last_plan, wp.q8_attention_blocks_in_last_plan) == (0, cfg.num_layers)
    for k, (a, b, c) in enumerate(zip(ref, split, whole)):
        assert a == b and a == c, f"frame {k}: {a} vs {b} vs {c}"
    assert any(r[0] > 0 for r in split)
