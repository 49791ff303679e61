"""GPU: a tiny moshika-shaped slots model over Q8_0 K / V rings with histories (kv_q8 = 3), B = 3, ring of 8: a slot takes 5 provided frames
in one pass while its neighbour steps, then 12 greedy frames across the wrap give the oracle's tokens (test_kv_q8_streams_gpu.py's criterion); every
layer of the pass is one k_attn_blocks_q8 launch pair; a fork is one k_ring_copy launch and the copy continues with its source's tokens."""
import pytest

import hot_util as hu
import slot_prefill_util as pu
import slot_state_util as ss
import streams_util as su

pytestmark = pytest.mark.gpu
RING, B, N_HIST, N_LIVE = 8, 3, 5, 12


def run(kind):
    cfg = su.lm_only(hu.hot.tiny(hu.L, context=RING))
    cfg.update_scale = 1.0 / 256   # (include/moshi_hot.h) rounding flips stay local instead of compounding over free-running frames
    cfg.kv_q8 = 3
    s = ss.Slots(kind, cfg, B, seed=5)
    hist, live, other = pu.history(cfg, N_HIST, seed=41), pu.live_codes(cfg, N_LIVE + 1, seed=51), pu.live_codes(cfg, N_LIVE + 1, seed=52)
    assert s.open(0) == 0 and s.open(1) == 0
    out = [ss.step_all(s, {0: other[0]})[:4]]
    assert s.prefill([(1, hist)]) == N_HIST
    plan = s.stats() if kind == "hip" else None
    out += [ss.step_all(s, {0: other[1 + k], 1: live[k]})[:4] for k in range(4)]
    assert s.fork(1, 2) == 0
    copies = s.stats() if kind == "hip" else None
    out += [ss.step_all(s, {0: other[5 + k], 1: live[4 + k], 2: live[4 + k]})[:4] for k in range(N_LIVE - 4)]
    s.free()
    return cfg, out, plan, copies


def test_prefilled_and_forked_slots_give_the_oracles_tokens_in_one_launch_pair_per_layer():
    (cfg, dev, plan, copies), (_, ref, _, _) = run("hip"), run("oracle")
    assert (plan.attn_block_launches_in_last_plan, plan.attn_block_jobs_in_last_plan, plan.generic_attention_nodes_in_last_plan) == (2 * cfg.num_layers, cfg.num_layers, 0)
    assert (copies.ring_copy_launches_in_last_plan, copies.ring_copy_jobs_in_last_plan) == (1, 2 * cfg.num_layers)
    for k, (a, b) in enumerate(zip(ref, dev)):
        assert a == b, f"frame {k}: {a} vs {b}"
    assert all(r[2][1] == r[2][2] and r[3][1] == r[3][2] for r in dev[5:]) and any(r[0] > 0 for r in dev)
