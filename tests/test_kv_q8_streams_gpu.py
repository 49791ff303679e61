"""GPU: tiny moshika- and stt-shaped slots models with Q8_0 K / V rings (moshi_hot_config::kv_q8): B = 3, greedy, 24 frames across the wrap of
an 8-slot ring, slots opened at staggered frames. Tokens equal the oracle's for the same graph, every Temporal layer's attention is one
k_attn_streams_q8 launch, and the Depth plan keeps the BF16 launches it has without the option."""
import pytest

import hot_util as hu
import slots_util as sl
import streams_util as su
import stt_slots_util as st
import test_float_streams_gpu as fst

pytestmark = pytest.mark.gpu
L = hu.L
RING, FRAMES, B = 8, 24, 3
EVENTS = {0: [("open", 0)], 2: [("open", 1)], 5: [("open", 2)]}


def moshika_cfg(kv_q8):
    cfg = su.lm_only(hu.hot.tiny(L, context=RING))
    cfg.update_scale = 1.0 / 256   # (include/moshi_hot.h) rounding flips stay local instead of compounding over free-running frames
    cfg.kv_q8 = kv_q8
    return cfg


def stt_cfg(kv_q8):
    cfg = hu.hot.tiny_stt(L, context=RING)
    cfg.update_scale = 1.0 / 256
    cfg.kv_q8 = kv_q8
    return cfg


@pytest.mark.parametrize("make,slots_cls", [(moshika_cfg, sl.Slots), (stt_cfg, st.Slots)], ids=["moshika", "stt"])
def test_tokens_equal_the_oracles_and_every_temporal_layer_is_one_q8_launch(make, slots_cls):
    cfg = make(1)
    codes = sl.slot_codes(cfg, B, FRAMES, seed=9)
    runs = {}
    for kind in ("oracle", "hip"):
        s = slots_cls(kind, cfg, B)
        runs[kind] = [r[:4] for r in sl.run_slots(s, codes, EVENTS)]
        if kind == "hip":
            assert L.ggml_backend_graph_compute(s.be, L.moshi_hot_graph(s.m, 0)) == 0   # the Temporal graph once more on its own: its plan is the last one
            assert s.stats().q8_attention_blocks_in_last_plan == cfg.num_layers
        s.free()
    assert any(r[0] > 0 for r in runs["hip"])
    for k, (a, b) in enumerate(zip(runs["oracle"], runs["hip"])):
        assert a == b, f"frame {k}: {a} vs {b}"


def test_the_depth_plan_keeps_its_bf16_launches():
    (_, d1), (t0, d0) = fst.plan_counters(moshika_cfg(1), B), fst.plan_counters(moshika_cfg(0), B)
    assert d1.q8_attention_blocks_in_last_plan == 0 and t0.q8_attention_blocks_in_last_plan == 0
    assert d1.kernels_in_last_plan == d0.kernels_in_last_plan and d1.generic_attention_nodes_in_last_plan == d0.generic_attention_nodes_in_last_plan == 0
