"""Slot prefill passes: moshika q4_k LM only, B = 8 slots, one MI355X. Timed in alternation on the same box, ROUNDS rounds of PASSES passes each
after WARMUP (every pass starts at stream position 0, so all passes see the same ring fill):
  (a) single_T64     one moshi_hot_prefill pass of 64 rows on a single-stream model (the yardstick)
  (b) slot_T64       one moshi_hot_slot_prefill pass of 64 rows into slot 0 of the slots model
  (c) jobs4x16_one   four jobs of 16 rows (slots 0 .. 3) in ONE pass;  jobs4x16_four: the same four jobs as four calls (four passes)
  live               a frame step of four live slots (4 .. 7) alone, and with one 64-row pass into held slot 0 in front of it
One JSON line per configuration: the median round, every round, and the spread (max - min) over rounds.
    python tests/microbench/slot_prefill_bench.py [--out FILE]"""
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

PASSES, WARMUP, ROUNDS, B, T = 6, 2, 5, 8, 64
pkg = load_package()
L = pkg.load()
from moshi_cpp_amd import hot  # noqa: E402


def config():
    cfg = hot.moshika(L)
    cfg.enable_mimi_encoder = cfg.enable_mimi_decoder = 0
    return cfg


class Bench:
    def __init__(self, be):
        self.be, self.cfg = be, config()
        cfg = self.cfg
        self.single = L.moshi_hot_create(be, C.byref(cfg), 0)
        self.slots = L.moshi_hot_create_slots(be, C.byref(cfg), 0, B)
        assert self.single and self.slots
        for b in range(B):
            assert L.moshi_hot_slot_open(self.slots, b) == 0
        rng = np.random.default_rng(1)
        ncb = cfg.n_q + 1
        self.frames = np.ascontiguousarray(np.concatenate([rng.integers(0, cfg.text_card, (T, 1)), rng.integers(0, cfg.card, (T, ncb - 1))], axis=1).astype(np.int32))
        self.ncb = ncb
        n_in, dq = cfg.n_q - cfg.dep_q, cfg.dep_q
        self.codes = np.ascontiguousarray(rng.integers(0, cfg.card, B * n_in).astype(np.int32))
        self.txt, self.aud, self.st = np.zeros(B, np.int32), np.zeros(B * dq, np.int32), np.zeros(B, np.int32)

    def sync(self):
        L.ggml_backend_synchronize(self.be)

    def jobs(self, slots, rows):
        n = len(slots)
        s = (C.c_int32 * n)(*slots)
        p = (C.c_void_p * n)(*[self.frames[i * rows:].ctypes.data for i in range(n)])
        c = (C.c_int32 * n)(*([rows] * n))
        assert L.moshi_hot_slots_prefill(self.slots, n, s, p, c, T) == n * rows

    def rewind(self, slots):
        for b in slots:
            L.moshi_hot_slot_set_fill(self.slots, b, 0)

    # one timed unit of each configuration (positions rewound outside the clock)
    def single_T64(self):
        L.moshi_hot_set_context_fill(self.single, 0)
        self.sync(); t0 = time.perf_counter()
        L.moshi_hot_prefill(self.single, self.frames.ctypes.data, T, T)
        self.sync(); return time.perf_counter() - t0

    def slot_T64(self):
        self.rewind([0])
        self.sync(); t0 = time.perf_counter()
        self.jobs([0], T)
        self.sync(); return time.perf_counter() - t0

    def jobs4x16_one(self):
        self.rewind(range(4))
        self.sync(); t0 = time.perf_counter()
        self.jobs([0, 1, 2, 3], 16)
        self.sync(); return time.perf_counter() - t0

    def jobs4x16_four(self):
        self.rewind(range(4))
        self.sync(); t0 = time.perf_counter()
        for b in range(4):
            self.jobs([b], 16)
        self.sync(); return time.perf_counter() - t0

    def step(self):
        L.moshi_hot_lm_step_slots(self.slots, self.codes.ctypes.data, self.txt.ctypes.data, self.aud.ctypes.data, self.st.ctypes.data)

    def live_setup(self, on):
        for b in range(4):
            assert L.moshi_hot_slot_hold(self.slots, b, 1 if on else 0) == 0
        self.rewind(range(4, B))

    def live_step(self):
        self.sync(); t0 = time.perf_counter()
        self.step()
        self.sync(); return time.perf_counter() - t0

    def live_step_after_pass(self):
        self.rewind([0])
        self.sync(); t0 = time.perf_counter()
        self.jobs([0], T)
        self.step()
        self.sync(); return time.perf_counter() - t0

    def free(self):
        L.moshi_hot_free(self.single)
        L.moshi_hot_free(self.slots)


PASS_KINDS = ["single_T64", "slot_T64", "jobs4x16_one", "jobs4x16_four"]
LIVE_KINDS = ["live_step", "live_step_after_pass"]


def main():
    out_path = sys.argv[2] if sys.argv[1:2] == ["--out"] else None
    L.ggml_backend_load_all()
    be = L.ggml_backend_init_by_type(pkg.DEV_GPU, None)
    assert be, "no MI355X device"
    b = Bench(be)
    times = {k: [] for k in PASS_KINDS + LIVE_KINDS}
    for k in PASS_KINDS:
        for _ in range(WARMUP):
            getattr(b, k)()
    for _ in range(ROUNDS):
        for k in PASS_KINDS:
            times[k].append(statistics.median(getattr(b, k)() for _ in range(PASSES)))
    b.live_setup(True)
    for k in LIVE_KINDS:
        for _ in range(WARMUP):
            getattr(b, k)()
    for _ in range(ROUNDS):
        for k in LIVE_KINDS:
            times[k].append(statistics.median(getattr(b, k)() for _ in range(PASSES)))
    b.live_setup(False)
    st = pkg.Stats()
    b.slot_T64()
    L.ggml_backend_mi355x_get_stats(be, C.byref(st))
    lines = []
    for k in PASS_KINDS + LIVE_KINDS:
        ms = [t * 1e3 for t in times[k]]
        lines.append({"config": k, "ms": round(statistics.median(ms), 4), "rounds_ms": [round(t, 4) for t in ms], "spread_ms": round(max(ms) - min(ms), 4),
                      "n_slots": B, "rows": T, "passes_per_round": PASSES, "rounds": ROUNDS, "warmup": WARMUP})
    med = {l["config"]: l["ms"] for l in lines}
    lines.append({"config": "summary", "slot_minus_single_ms": round(med["slot_T64"] - med["single_T64"], 4),
                  "single_spread_ms": next(l["spread_ms"] for l in lines if l["config"] == "single_T64"),
                  "four_calls_over_one_pass": round(med["jobs4x16_four"] / med["jobs4x16_one"], 3),
                  "pass_adds_to_live_step_ms": round(med["live_step_after_pass"] - med["live_step"], 4),
                  "kernels_in_slot_pass_plan": st.kernels_in_last_plan, "attn_block_launches_in_slot_pass_plan": st.attn_block_launches_in_last_plan,
                  "generic_attention_nodes_in_slot_pass_plan": st.generic_attention_nodes_in_last_plan})
    for l in lines:
        print(json.dumps(l), flush=True)
    if out_path:
        with open(out_path, "w") as f:
            json.dump({"bench": "slot_prefill_bench", "model": "moshika q4_k, LM only", "lines": lines}, f, indent=1)
            f.write("\n")
    b.free()
    L.ggml_backend_free(be)


if __name__ == "__main__":
    main()
