"""Stream slots throughput: moshika q4_k LM only. For each B, one lockstep model (moshi_hot_create_streams) and two slots models
(moshi_hot_create_slots): every slot opened at frame 0 (equal positions, the lockstep model's), and slots whose fills are spread evenly over
0 .. 2 800 (moshi_hot_slot_set_fill). The three are timed in alternation, ROUNDS x FRAMES frame steps each after WARMUP; one JSON line per
(B, configuration) with the median round.
    python tests/microbench/slots_bench.py [--only CONFIG] [B ...]          (default 4 8 16; CONFIG: lockstep | slots_equal | slots_spread)
--only times one configuration alone (a profiler run of the slots step: SLOTS_BENCH_FLAGS=2 under rocprofv3 --kernel-trace --stats)."""
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

FRAMES, WARMUP, ROUNDS, MAX_FILL = 40, 5, 3, 2800
pkg = load_package()
L = pkg.load()
from moshi_cpp_amd import hot  # noqa: E402


class Runner:
    def __init__(self, be, B, kind):
        cfg = hot.moshika(L)
        cfg.enable_mimi_encoder = cfg.enable_mimi_decoder = 0
        self.be, self.B, self.kind, self.i = be, B, kind, 0
        if kind == "lockstep":
            self.m = L.moshi_hot_create_streams(be, C.byref(cfg), 0, B)
        else:
            self.m = L.moshi_hot_create_slots(be, C.byref(cfg), 0, B)
        assert self.m, (B, kind)
        if kind != "lockstep":
            for b in range(B):
                assert L.moshi_hot_slot_open(self.m, b) == 0
                if kind == "slots_spread":
                    L.moshi_hot_slot_set_fill(self.m, b, round(MAX_FILL * b / (B - 1)))
        n_in, dq = cfg.n_q - cfg.dep_q, cfg.dep_q
        rng = np.random.default_rng(B)
        self.codes = [np.ascontiguousarray(rng.integers(0, cfg.card, B * n_in).astype(np.int32)) for _ in range(64)]
        self.txt = np.zeros(B, np.int32)
        self.aud = np.zeros(B * dq, np.int32)
        self.st = np.zeros(B, np.int32)

    def step(self):
        c = self.codes[self.i % len(self.codes)]
        self.i += 1
        if self.kind == "lockstep":
            return L.moshi_hot_lm_step_streams(self.m, c.ctypes.data, self.txt.ctypes.data, self.aud.ctypes.data)
        return L.moshi_hot_lm_step_slots(self.m, c.ctypes.data, self.txt.ctypes.data, self.aud.ctypes.data, self.st.ctypes.data)

    def timed(self, n):
        L.ggml_backend_synchronize(self.be)
        t0 = time.perf_counter()
        for _ in range(n):
            self.step()
        L.ggml_backend_synchronize(self.be)
        return (time.perf_counter() - t0) / n

    def kernels_temporal(self):
        # the Temporal graph's plan, computed once more on its own (same inputs, same ring slots)
        st = pkg.Stats()
        L.ggml_backend_graph_compute(self.be, L.moshi_hot_graph(self.m, 0))
        L.ggml_backend_mi355x_get_stats(self.be, C.byref(st))
        return st.kernels_in_last_plan

    def free(self):
        L.moshi_hot_free(self.m)


KINDS = ["lockstep", "slots_equal", "slots_spread"]


def bench(be, B, kinds=KINDS):
    runs = {k: Runner(be, B, k) for k in kinds}
    for r in runs.values():
        r.timed(WARMUP)
    times = {k: [] for k in kinds}
    for _ in range(ROUNDS):
        for k in kinds:
            times[k].append(runs[k].timed(FRAMES))
    out = []
    for k in kinds:
        dt = statistics.median(times[k])
        r = runs[k]
        fills = [int(L.moshi_hot_slot_position(r.m, b)) for b in range(B)] if k != "lockstep" else None
        out.append({"n_streams": B, "config": k, "ms_per_step": round(dt * 1e3, 4), "aggregate_frames_per_s": round(B / dt, 1),
                    "rounds_ms": [round(t * 1e3, 4) for t in times[k]], "kernels_in_temporal_plan": r.kernels_temporal(),
                    "fill_min": min(fills) if fills else None, "fill_max": max(fills) if fills else None,
                    "frames": FRAMES, "rounds": ROUNDS, "warmup": WARMUP})
    for r in runs.values():
        r.free()
    return out


def main():
    args = sys.argv[1:]
    kinds = KINDS
    if args[:1] == ["--only"]:
        assert args[1] in KINDS, args[1]
        kinds, args = [args[1]], args[2:]
    Bs = [int(a) for a in args] or [4, 8, 16]
    L.ggml_backend_load_all()
    be = L.ggml_backend_init_by_type(pkg.DEV_GPU, None)
    assert be, "no MI355X device"
    L.ggml_backend_mi355x_set_flags(be, int(os.environ.get("SLOTS_BENCH_FLAGS", "0")))   # 2 = no hipGraph capture (under rocprofv3)
    for B in Bs:
        for line in bench(be, B, kinds):
            print(json.dumps(line), flush=True)
    L.ggml_backend_free(be)


if __name__ == "__main__":
    main()
