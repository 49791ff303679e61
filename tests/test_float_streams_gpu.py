"""-m gpu: B-column models with BF16 / F16 linears on the MI355X. Their multi-column products run on the f64-MFMA mat-mul (k_mm_f_batched), which keeps
the arithmetic of ggml's generic BF16 / F16 product (rows rounded to the weight's type, exact products, double sums, one rounding to float): slots
models against the oracle's slots model, one prefill pass beside a live neighbour, and one Temporal layer at moshika's widths.

Bars: token ids equal on the contractive model; logits under the BF16 bars of tests/test_streams_gpu.py (median below 1e-6, 90 % of slot-frames
within 1e-6, every one below 0.1), for F16 linears too; moshika widths under the BF16 bar of tests/test_hip_frame.py's TYPE_TOL (1e-6)."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import hot_util as hu
import slot_prefill_util as pu
import slots_util as sl
import streams_util as su
from ggml_util import BF16, F16

pytestmark = pytest.mark.gpu
L = hu.L
RING = 8
BF16_TOL = 1e-6        # tests/test_streams_gpu.py TYPE_TOL[BF16], tests/test_hip_frame.py TYPE_TOL[BF16]
TYPES = pytest.mark.parametrize("lt,et", [(BF16, BF16), (F16, F16)], ids=["bf16", "f16"])


def tiny_slots(lt, et, context=RING):
    cfg = su.lm_only(hu.hot.tiny(L, linear_type=lt, embed_type=et, context=context))
    cfg.wide_streams = 1
    cfg.update_scale = 1.0 / 256   # (include/moshi_hot.h) rounding flips stay local instead of compounding over free-running frames
    return cfg


def staggered_events(B):
    """slot b opens at frame b % 6 (beyond B = 3 the last slot stays closed); slot 0 is reopened after its conversation ran past the 8-slot ring's wrap"""
    ev = {}
    for b in range(B if B <= 3 else B - 1):
        ev.setdefault(b % 6, []).append(("open", b))
    ev.setdefault(RING + 2, []).extend([("close", 0), ("open", 0)])
    return ev


def plan_counters(cfg, B):
    """-> (Temporal plan, Depth plan) counters of a slots step with every slot open"""
    s = sl.Slots("hip", cfg, B)
    for b in range(B):
        assert s.open(b) == 0
    for fr in sl.slot_codes(cfg, B, 2, seed=2):
        s.step(fr)
    depth = s.stats()                                        # the Depth graph is the last graph of a step
    assert L.ggml_backend_graph_compute(s.be, L.moshi_hot_graph(s.m, 0)) == 0   # the Temporal graph once more on its own: its plan is the last one
    temporal = s.stats()
    s.free()
    return temporal, depth


@TYPES
@pytest.mark.parametrize("B", [3, 33])
def test_staggered_slots_match_oracle_across_the_ring_wrap(lt, et, B):
    cfg = tiny_slots(lt, et)
    n = 12
    codes = sl.slot_codes(cfg, B, n, seed=B)
    events = staggered_events(B)
    rec = {}
    for kind in ("oracle", "hip"):
        s = sl.Slots(kind, cfg, B, seed=0)
        rec[kind] = sl.run_slots(s, codes, events, logits=True, dep_logits=True)
        s.free()
    errs = []
    for i, (a, b) in enumerate(zip(rec["oracle"], rec["hip"])):
        assert a[:4] == b[:4], f"frame {i}: tokens differ: oracle {a[:4]} vs hip {b[:4]}"
        for c in range(B):
            if a[1][c] != -1:
                errs.append(max(hu.rel_err(a[4][c], b[4][c]), hu.rel_err(a[5][c], b[5][c])))
    assert any(r[0] >= min(B, 3) for r in rec["oracle"]) and len({t for r in rec["oracle"] for t in r[2] if t >= 0}) > 1
    errs = np.array(errs)
    print(f"B = {B}: {errs.size} slot-frames, median logit error {np.median(errs):.2e}, {np.mean(errs < BF16_TOL):.3f} within {BF16_TOL:.0e}, max {errs.max():.2e}")
    assert np.median(errs) < BF16_TOL, f"median logit error {np.median(errs):.2e}"
    assert np.mean(errs < BF16_TOL) >= 0.9 and errs.max() < 0.1, f"logit errors over the bar {BF16_TOL:.0e}: {np.sort(errs)[-8:]}"
    temporal, depth = plan_counters(cfg, B)
    # in_proj, out_proj, linear_in, linear_out of every layer and the text head
    assert temporal.float_batched_mms_in_last_plan == 4 * cfg.num_layers + 1, temporal.float_batched_mms_in_last_plan
    assert depth.float_batched_mms_in_last_plan > 0


def test_temporal_plan_is_shorter_than_with_the_generic_product():
    # MI355X_MMF is read once per process: the same model's Temporal plan in a child process with the switch off (norms, gates and residual adds are
    # launches of their own there)
    cfg = tiny_slots(BF16, BF16)
    here = plan_counters(cfg, 3)[0]
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--temporal-plan"], env=dict(os.environ, MI355X_MMF="0"),
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert p.returncode == 0 and lines, p.stdout[-2000:]
    off = json.loads(lines[-1])
    print(f"Temporal plan: {here.kernels_in_last_plan} launches, {off['kernels']} with MI355X_MMF=0")
    assert off["float_batched_mms"] == 0 and here.float_batched_mms_in_last_plan > 0
    assert here.kernels_in_last_plan < off["kernels"]


# ---- one prefill pass of 20 rows over two jobs beside a live slot ---------------------------------------------------------------------------
HIST = {1: 13, 2: 7}
N_BEFORE, N_LIVE = 2, 4


@functools.lru_cache(maxsize=None)
def prefill_scenario(kind, with_prefill=True):
    cfg = tiny_slots(BF16, BF16, context=24)                 # ring of 24 >= 13 history + 4 live frames
    s = pu.Slots(kind, cfg, 3)
    codes = su.stream_codes(cfg, 3, N_BEFORE + N_LIVE, seed=21)
    assert s.open(0) == 0
    frames, passes = [], None
    for k, fr in enumerate(codes):
        if k == N_BEFORE and with_prefill:
            assert s.open(1) == 0 and s.open(2) == 0
            assert s.prefill([(b, pu.history(cfg, n, seed=60 + b)) for b, n in HIST.items()], 32) == sum(HIST.values())   # one pass of 20 rows
            passes = s.stats().float_batched_mms_in_last_plan if kind == "hip" else None
        r = s.step(fr)
        frames.append(r[1:] + (s.read("text_logits", cfg.text_card),))
    s.free()
    return frames, passes, cfg.num_layers


def test_prefill_pass_of_20_rows_then_live_frames_match_oracle_tokens():
    ref, _, _ = prefill_scenario("oracle")
    got, mms, layers = prefill_scenario("hip")
    assert mms >= 4 * layers, f"{mms} f64-MFMA mat-muls in the pass's plan"
    for k, (a, g) in enumerate(zip(ref, got)):
        assert a[:3] == g[:3], f"frame {k}: tokens differ: oracle {a[:3]} vs hip {g[:3]}"
    assert any(st == [1, 1, 1] for st, _, _, _ in ref[N_BEFORE:])


def test_live_neighbour_is_bit_identical_with_and_without_the_prefill():
    a, _, _ = prefill_scenario("hip", False)
    b, _, _ = prefill_scenario("hip")
    for k, (x, y) in enumerate(zip(a, b)):
        assert x[0][0] == y[0][0] and x[1][0] == y[1][0] and x[2][0] == y[2][0], f"frame {k}: slot 0's tokens differ"
        assert np.array_equal(x[3][0], y[3][0]), f"frame {k}: slot 0's text logits differ"
    assert any(x[0][0] == 1 for x in a)


# ---- moshika's Temporal widths: K = 4096 / 11264, M = 12288 / 22528 / 32000 through the real graph --------------------------------------------
def test_one_temporal_layer_at_moshika_widths_matches_oracle():
    cfg = su.lm_only(hu.hot.moshika(L))
    cfg.num_layers, cfg.context = 1, 8
    # (the Depth transformer at the tiny model's widths: this test is about the Temporal layer and the text head, and the oracle's time is the test's)
    cfg.dep_dim, cfg.dep_heads, cfg.dep_layers, cfg.dep_ffn_hidden = 256, 4, 1, 512
    cfg.linear_type = cfg.embed_type = BF16
    cfg.update_scale = 1.0 / 256                          # contractive stack (include/moshi_hot.h): no chaotic rounding flips at full width
    B, n = 3, 2
    codes = su.stream_codes(cfg, B, n, seed=5)
    ref = su.run_streams("oracle", cfg, codes, logits=True)
    got = su.run_streams("hip", cfg, codes, logits=True)
    for k, (a, g) in enumerate(zip(ref, got)):
        assert a[0] == g[0] and a[1] == g[1], f"frame {k}: text tokens differ: oracle {a[1]} vs hip {g[1]}"
        for b in range(B):
            e = hu.rel_err(a[3][b], g[3][b])
            print(f"frame {k} stream {b}: text logits rel err {e:.2e}")
            assert e < BF16_TOL, f"frame {k} stream {b}: text logits rel err {e:.2e}"


if __name__ == "__main__" and sys.argv[1:] == ["--temporal-plan"]:
    st = plan_counters(tiny_slots(BF16, BF16), 3)[0]
    print(json.dumps({"kernels": st.kernels_in_last_plan, "float_batched_mms": st.float_batched_mms_in_last_plan}))
