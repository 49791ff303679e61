"""The LM step over Q8_0 K / V rings with the step attention unsplit and split along the ring (ggml_backend_mi355x_set_attn_q8_split):
moshika q4_k LM only, slots, kv_q8 = 1, context 3000, one MI355X. For B = 2, 4, 8, 16 and ring fills of about 130, 750 and 2800 live slots (every slot
put there with moshi_hot_slot_set_fill before every timed unit: positions only), in ONE process on one handle, alternating per round:
  unsplit   setter value 0: one k_attn_streams_q8 launch per Temporal layer (what a kv_q8 model ran before the setter existed)
  auto      setter value 1: the k_attn_streams_q8_split launch pair where usable CUs / (H x B) gives S >= 2
A change of the setter drops the handle's plans, so every unit starts with WARMUP untimed steps (plan build, hipGraph capture). A unit is STEPS frames
between two synchronises; a second set of rounds runs with moshi_hot_set_timing on and reports the Temporal phase alone. One JSON line per
(B, fill, config): the median round, every round, the spread (max - min); then one summary line per (B, fill).
    python tests/microbench/kv_q8_split_bench.py [--out FILE] [--cus N]     (N: the stream's usable compute units, for the reported S; default 256)"""
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402

STEPS, WARMUP, ROUNDS = 20, 3, 5
BS, FILLS = (2, 4, 8, 16), (130, 750, 2800)
CONFIGS = {"unsplit": 0, "auto": 1}
pkg = load_package()
L = pkg.load()
from moshi_cpp_amd import hot  # noqa: E402


class Bench:
    def __init__(self, be, B):
        cfg = hot.moshika(L)
        cfg.enable_mimi_encoder = cfg.enable_mimi_decoder = 0
        cfg.kv_q8 = 1
        assert cfg.context == 3000
        self.be, self.cfg, self.B = be, cfg, B
        self.m = L.moshi_hot_create_slots(be, C.byref(cfg), 0, B)
        assert self.m
        for b in range(B):
            assert L.moshi_hot_slot_open(self.m, b) == 0
        n_in, dq = cfg.n_q - cfg.dep_q, cfg.dep_q
        self.codes = np.ascontiguousarray(np.random.default_rng(1).integers(0, cfg.card, B * n_in).astype(np.int32))
        self.txt, self.aud, self.st = np.zeros(B, np.int32), np.zeros(B * dq, np.int32), np.zeros(B, np.int32)

    def steps(self, n):
        for _ in range(n):
            L.moshi_hot_lm_step_slots(self.m, self.codes.ctypes.data, self.txt.ctypes.data, self.aud.ctypes.data, self.st.ctypes.data)

    def unit(self, fill, setting, timing):
        """-> ms per step (timing off) or the Temporal phase's ms per step (timing on)"""
        L.ggml_backend_mi355x_set_attn_q8_split(self.be, setting)
        for b in range(self.B):
            L.moshi_hot_slot_set_fill(self.m, b, fill)
        self.steps(WARMUP)
        L.moshi_hot_set_timing(self.m, 1 if timing else 0)
        L.ggml_backend_synchronize(self.be); t0 = time.perf_counter()
        self.steps(STEPS)
        L.ggml_backend_synchronize(self.be); dt = time.perf_counter() - t0
        if not timing:
            return dt * 1e3 / STEPS
        us = (C.c_double * 4)()
        L.moshi_hot_get_timing(self.m, us)
        L.moshi_hot_set_timing(self.m, 0)
        return us[1] / 1e3

    def plan(self):
        """the Temporal plan's counters under the setting in force"""
        st = pkg.Stats()
        assert L.ggml_backend_graph_compute(self.be, L.moshi_hot_graph(self.m, 0)) == 0
        L.ggml_backend_mi355x_get_stats(self.be, C.byref(st))
        return {"kernels_in_temporal_plan": st.kernels_in_last_plan, "q8_attention_blocks": st.q8_attention_blocks_in_last_plan,
                "q8_attention_split_blocks": st.q8_attention_split_blocks_in_last_plan}


def main():
    args = sys.argv[1:]
    out_path = args[args.index("--out") + 1] if "--out" in args else None
    cus = int(args[args.index("--cus") + 1]) if "--cus" in args else 256
    L.ggml_backend_load_all()
    be = L.ggml_backend_init_by_type(pkg.DEV_GPU, None)
    assert be, "no MI355X device"
    lines = []
    for B in BS:
        bench = Bench(be, B)
        H = bench.cfg.num_heads
        for fill in FILLS:
            step = {k: [] for k in CONFIGS}
            temporal = {k: [] for k in CONFIGS}
            for times, timing in ((step, False), (temporal, True)):
                for _ in range(ROUNDS):
                    for k, v in CONFIGS.items():
                        times[k].append(bench.unit(fill, v, timing))
            by = {}
            for k, v in CONFIGS.items():
                L.ggml_backend_mi355x_set_attn_q8_split(be, v)
                bench.steps(1)
                plan = bench.plan()
                S = min((bench.cfg.context + 255) // 256, 16, cus // (H * B)) if plan["q8_attention_split_blocks"] else 1
                by[k] = dict({"config": k, "B": B, "fill": fill, "ms_per_step": round(statistics.median(step[k]), 4), "rounds_ms": [round(t, 4) for t in step[k]],
                              "spread_ms": round(max(step[k]) - min(step[k]), 4), "temporal_ms": round(statistics.median(temporal[k]), 4),
                              "temporal_spread_ms": round(max(temporal[k]) - min(temporal[k]), 4), "S": S, "steps_per_round": STEPS, "rounds": ROUNDS,
                              "warmup": WARMUP}, **plan)
                lines.append(by[k])
                print(json.dumps(by[k]), flush=True)
            u, a = by["unsplit"], by["auto"]
            spread = max(u["spread_ms"], a["spread_ms"])
            lines.append({"config": "summary", "B": B, "fill": fill, "S": a["S"], "unsplit_minus_auto_ms": round(u["ms_per_step"] - a["ms_per_step"], 4), "larger_spread_ms": spread,
                          "auto_wins": u["ms_per_step"] - a["ms_per_step"] > spread, "auto_loses": a["ms_per_step"] - u["ms_per_step"] > spread,
                          "temporal_unsplit_minus_auto_ms": round(u["temporal_ms"] - a["temporal_ms"], 4)})
            print(json.dumps(lines[-1]), flush=True)
        L.ggml_backend_mi355x_set_attn_q8_split(be, 0)
        L.moshi_hot_free(bench.m)
    L.ggml_backend_free(be)
    if out_path:
        with open(out_path, "w") as f:
            json.dump({"bench": "kv_q8_split_bench", "model": "moshika q4_k, LM only, slots, kv_q8 = 1, context 3000", "usable_cus_assumed": cus, "lines": lines}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
