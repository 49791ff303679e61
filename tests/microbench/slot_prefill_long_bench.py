"""Slot prefill past the ring's end: moshika q4_k LM only, B = 8 slots, context 3000, one MI355X. Slot 1 is put past the wrap with
moshi_hot_slot_set_fill(m, 1, 3100) before every timed unit (positions only: no recompute is needed for timing), so every unit sees a full ring.
Timed in alternation on the same box, ROUNDS rounds of PASSES units each after WARMUP:
  (i)   rows_pass_T16    one moshi_hot_slot_prefill_long pass of 16 ring-ordered rows into held slot 1 (one k_attn_rows launch per layer)
  (ii)  steps16          16 moshi_hot_lm_step_slots calls of the same model with slot 1 live at the same fill: what stepping a history frame by
                         frame costs (Depth graph and sampler included - there is no cheaper way to step a slots model)
  (iii) per_row_pass_T16 the pass of (i) in a process of its own with MI355X_NO_ATTN_ROWS=1: every row its own attention launches
One JSON line per configuration: the median round, every round, and the spread (max - min) over rounds; first_pass_ms is the first pass of the
process (graph building, planning and the launch, against a reused plan in every later pass). With MI355X_TIME_PLAN=1 the backend prints on
stderr, for every graph it computes, the time to build (or reuse) its plan and to launch it.
    python tests/microbench/slot_prefill_long_bench.py [--out FILE]"""
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402

PASSES, WARMUP, ROUNDS, B, T, FILL = 3, 2, 5, 8, 16, 3100
pkg = load_package()
L = pkg.load()
from moshi_cpp_amd import hot  # noqa: E402


class Bench:
    def __init__(self, be):
        cfg = hot.moshika(L)
        cfg.enable_mimi_encoder = cfg.enable_mimi_decoder = 0
        assert cfg.context == 3000
        self.be, self.cfg = be, cfg
        self.m = L.moshi_hot_create_slots(be, C.byref(cfg), 0, B)
        assert self.m and L.moshi_hot_slot_open(self.m, 1) == 0
        rng = np.random.default_rng(1)
        ncb = cfg.n_q + 1
        self.frames = np.ascontiguousarray(np.concatenate([rng.integers(0, cfg.text_card, (T, 1)), rng.integers(0, cfg.card, (T, ncb - 1))], axis=1).astype(np.int32))
        n_in, dq = cfg.n_q - cfg.dep_q, cfg.dep_q
        self.codes = np.ascontiguousarray(rng.integers(0, cfg.card, B * n_in).astype(np.int32))
        self.txt, self.aud, self.st = np.zeros(B, np.int32), np.zeros(B * dq, np.int32), np.zeros(B, np.int32)

    def sync(self):
        L.ggml_backend_synchronize(self.be)

    def rows_pass_T16(self):
        assert L.moshi_hot_slot_hold(self.m, 1, 1) == 0
        L.moshi_hot_slot_set_fill(self.m, 1, FILL)
        self.sync(); t0 = time.perf_counter()
        assert L.moshi_hot_slot_prefill_long(self.m, 1, self.frames.ctypes.data, T, T) == T
        self.sync(); return time.perf_counter() - t0

    def steps16(self):
        assert L.moshi_hot_slot_hold(self.m, 1, 0) == 0
        L.moshi_hot_slot_set_fill(self.m, 1, FILL)
        self.sync(); t0 = time.perf_counter()
        for _ in range(T):
            L.moshi_hot_lm_step_slots(self.m, self.codes.ctypes.data, self.txt.ctypes.data, self.aud.ctypes.data, self.st.ctypes.data)
        self.sync(); return time.perf_counter() - t0

    def plan(self):
        st = pkg.Stats()
        self.rows_pass_T16()
        L.ggml_backend_mi355x_get_stats(self.be, C.byref(st))
        return {"nodes_in_pass_plan": st.nodes_in_last_plan, "kernels_in_pass_plan": st.kernels_in_last_plan, "attn_row_launches": st.attn_row_launches_in_last_plan,
                "attn_row_jobs": st.attn_row_jobs_in_last_plan, "attn_row_rows": st.attn_row_rows_in_last_plan, "attn_block_launches": st.attn_block_launches_in_last_plan,
                "generic_attention_nodes": st.generic_attention_nodes_in_last_plan}

    def free(self):
        L.moshi_hot_free(self.m)


def measure(kinds):
    L.ggml_backend_load_all()
    be = L.ggml_backend_init_by_type(pkg.DEV_GPU, None)
    assert be, "no MI355X device"
    b = Bench(be)
    first = b.rows_pass_T16() * 1e3
    times = {k: [] for k in kinds}
    for k in kinds:
        for _ in range(WARMUP):
            getattr(b, k)()
    for _ in range(ROUNDS):
        for k in kinds:
            times[k].append(statistics.median(getattr(b, k)() for _ in range(PASSES)))
    lines = []
    for k in kinds:
        ms = [t * 1e3 for t in times[k]]
        lines.append({"config": k, "ms": round(statistics.median(ms), 4), "rounds_ms": [round(t, 4) for t in ms], "spread_ms": round(max(ms) - min(ms), 4),
                      "n_slots": B, "rows": T, "fill": FILL, "units_per_round": PASSES, "rounds": ROUNDS, "warmup": WARMUP})
    lines.append(dict({"config": "plan", "first_pass_ms": round(first, 3)}, **b.plan()))
    b.free()
    L.ggml_backend_free(be)
    return lines


def main():
    if sys.argv[1:2] == ["--child"]:                          # (iii): this process was started with MI355X_NO_ATTN_ROWS=1
        for l in measure(["rows_pass_T16"]):
            print(json.dumps(l), flush=True)
        return
    out_path = sys.argv[2] if sys.argv[1:2] == ["--out"] else None
    lines = measure(["rows_pass_T16", "steps16"])
    env = dict(os.environ, MI355X_NO_ATTN_ROWS="1")
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, stdout=subprocess.PIPE, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:]
    for l in (json.loads(x) for x in p.stdout.splitlines() if x.startswith("{")):
        l["config"] = {"rows_pass_T16": "per_row_pass_T16", "plan": "per_row_plan"}[l["config"]]
        lines.append(l)
    by = {l["config"]: l for l in lines}
    i, ii, iii = by["rows_pass_T16"], by["steps16"], by["per_row_pass_T16"]
    lines.append({"config": "summary", "steps16_over_rows_pass": round(ii["ms"] / i["ms"], 3), "steps16_minus_rows_pass_ms": round(ii["ms"] - i["ms"], 4),
                  "larger_spread_ms": max(i["spread_ms"], ii["spread_ms"]), "rows_pass_faster_by_more_than_the_spread": ii["ms"] - i["ms"] > max(i["spread_ms"], ii["spread_ms"]),
                  "per_row_pass_over_rows_pass": round(iii["ms"] / i["ms"], 3)})
    for l in lines:
        print(json.dumps(l), flush=True)
    if out_path:
        with open(out_path, "w") as f:
            json.dump({"bench": "slot_prefill_long_bench", "model": "moshika q4_k, LM only, B = 8, context 3000", "lines": lines}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
