"""GPU: a tiny moshika-shaped slots model over Q8_0 K / V rings with histories past the ring's end (kv_q8 = 7), B = 3, ring of 32: a slot
takes 53 provided frames through _prefill_long beside a stepping neighbour (passes 32 | 16 | 5, the last two ring-ordered), then 8 greedy frames give the
oracle's tokens; the last pass is one k_attn_rows_q8 launch per layer and holds no generic attention node."""
import pytest

import hot_util as hu
import slot_prefill_long_util as lu
import slot_state_util as ss
import streams_util as su

pytestmark = pytest.mark.gpu
RING, B, N_HIST, N_LIVE = 32, 3, 53, 8


def run(kind):
    cfg = su.lm_only(hu.hot.tiny(hu.L, context=RING))
    cfg.update_scale = 1.0 / 256   # (include/moshi_hot.h) rounding flips stay local instead of compounding over free-running frames
    cfg.kv_q8 = 7
    s = lu.Slots(kind, cfg, B, seed=5)
    hist, live, other = lu.history(cfg, N_HIST, seed=41), lu.live_codes(cfg, N_LIVE, seed=51), lu.live_codes(cfg, N_LIVE + 1, seed=52)
    assert s.open(0) == 0
    out = [ss.step_all(s, {0: other[0]})[:4]]
    assert s.open(1) == 0 and s.prefill_long_one(1, hist, 0) == N_HIST and s.position(1) == N_HIST
    plan = s.stats() if kind == "hip" else None
    out += [ss.step_all(s, {0: other[1 + k], 1: live[k]})[:4] for k in range(N_LIVE)]
    s.free()
    return cfg, out, plan


def test_a_long_history_gives_the_oracles_tokens_in_one_rows_launch_per_layer():
    (cfg, dev, plan), (_, ref, _) = run("hip"), run("oracle")
    n, rows = cfg.num_layers, (N_HIST - RING) % 16
    assert (plan.attn_row_launches_in_last_plan, plan.attn_row_jobs_in_last_plan, plan.attn_row_rows_in_last_plan) == (n, n, rows * n)
    assert (plan.attn_block_launches_in_last_plan, plan.generic_attention_nodes_in_last_plan) == (0, 0)
    for k, (a, b) in enumerate(zip(ref, dev)):
        assert a == b, f"frame {k}: {a} vs {b}"
    assert any(r[0] > 0 for r in dev)
