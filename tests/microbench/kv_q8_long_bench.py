"""Slot prefill past the ring's end over Q8_0 K / V rings (kv_q8 = 7): moshika q4_k LM only, B = 8 slots, context 3000, one MI355X.
Slot 1 is put past the wrap with moshi_hot_slot_set_fill(m, 1, 3100) before every timed unit (positions only), so every unit sees a full ring.
Timed in alternation on the same box, ROUNDS rounds of PASSES units each after WARMUP:
  (i)   q8_rows_pass_T16     one moshi_hot_slot_prefill_long pass of 16 ring-ordered rows with kv_q8 = 7 (one k_attn_rows_q8 launch per layer)
  (ii)  q8_per_row_pass_T16  the same pass in a process of its own with MI355X_NO_ATTN_ROWS=1: every row its own k_attn_blocks_q8 launch pair
  (iii) bf16_rows_pass_T16   the same pass of a kv_q8 = 0 model in the process of (i): k_attn_rows, slot_prefill_long_bench.py's (i)
One JSON line per configuration: the median round, every round, and the spread (max - min) over rounds.
    python tests/microbench/kv_q8_long_bench.py [--out FILE]"""
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
    def __init__(self, be, kv_q8):
        cfg = hot.moshika(L)
        cfg.enable_mimi_encoder = cfg.enable_mimi_decoder = 0
        cfg.kv_q8 = kv_q8
        assert cfg.context == 3000
        self.be, self.cfg = be, cfg
        self.m = L.moshi_hot_create_slots(be, C.byref(cfg), 0, B)
        assert self.m and L.moshi_hot_slot_open(self.m, 1) == 0 and L.moshi_hot_slot_hold(self.m, 1, 1) == 0
        rng = np.random.default_rng(1)
        self.frames = np.ascontiguousarray(np.concatenate([rng.integers(0, cfg.text_card, (T, 1)), rng.integers(0, cfg.card, (T, cfg.n_q))], axis=1).astype(np.int32))

    def rows_pass(self):
        L.moshi_hot_slot_set_fill(self.m, 1, FILL)
        L.ggml_backend_synchronize(self.be); t0 = time.perf_counter()
        assert L.moshi_hot_slot_prefill_long(self.m, 1, self.frames.ctypes.data, T, T) == T
        L.ggml_backend_synchronize(self.be); return time.perf_counter() - t0

    def plan(self):
        st = pkg.Stats()
        self.rows_pass()
        L.ggml_backend_mi355x_get_stats(self.be, C.byref(st))
        return {"kernels_in_pass_plan": st.kernels_in_last_plan, "attn_row_launches": st.attn_row_launches_in_last_plan, "attn_row_rows": st.attn_row_rows_in_last_plan,
                "attn_block_launches": st.attn_block_launches_in_last_plan, "generic_attention_nodes": st.generic_attention_nodes_in_last_plan}


def measure(models):
    """models: {config name: kv_q8} -> one line per config"""
    L.ggml_backend_load_all()
    be = L.ggml_backend_init_by_type(pkg.DEV_GPU, None)
    assert be, "no MI355X device"
    bench = {k: Bench(be, v) for k, v in models.items()}
    times = {k: [] for k in bench}
    for b in bench.values():
        for _ in range(WARMUP):
            b.rows_pass()
    for _ in range(ROUNDS):
        for k, b in bench.items():
            times[k].append(statistics.median(b.rows_pass() for _ in range(PASSES)))
    lines = []
    for k, b in bench.items():
        ms = [t * 1e3 for t in times[k]]
        lines.append(dict({"config": k, "ms": round(statistics.median(ms), 4), "rounds_ms": [round(t, 4) for t in ms], "spread_ms": round(max(ms) - min(ms), 4),
                           "n_slots": B, "rows": T, "fill": FILL, "units_per_round": PASSES, "rounds": ROUNDS, "warmup": WARMUP}, **b.plan()))
        L.moshi_hot_free(b.m)
    L.ggml_backend_free(be)
    return lines


def main():
    if sys.argv[1:2] == ["--child"]:                          # (ii): this process was started with MI355X_NO_ATTN_ROWS=1
        for l in measure({"q8_per_row_pass_T16": 7}):
            print(json.dumps(l), flush=True)
        return
    out_path = sys.argv[2] if sys.argv[1:2] == ["--out"] else None
    lines = measure({"q8_rows_pass_T16": 7, "bf16_rows_pass_T16": 0})
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=dict(os.environ, MI355X_NO_ATTN_ROWS="1"), stdout=subprocess.PIPE, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:]
    lines += [json.loads(x) for x in p.stdout.splitlines() if x.startswith("{")]
    by = {l["config"]: l for l in lines}
    i, ii, iii = by["q8_rows_pass_T16"], by["q8_per_row_pass_T16"], by["bf16_rows_pass_T16"]
    spread = max(i["spread_ms"], ii["spread_ms"])
    lines.append({"config": "summary", "per_row_over_rows_pass": round(ii["ms"] / i["ms"], 3), "per_row_minus_rows_pass_ms": round(ii["ms"] - i["ms"], 4), "larger_spread_ms": spread,
                  "rows_pass_faster_by_more_than_the_spread": ii["ms"] - i["ms"] > spread, "bf16_rows_over_q8_rows_pass": round(iii["ms"] / i["ms"], 3)})
    for l in lines:
        print(json.dumps(l), flush=True)
    if out_path:
        with open(out_path, "w") as f:
            json.dump({"bench": "kv_q8_long_bench", "model": "moshika q4_k, LM only, B = 8, context 3000", "lines": lines}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
