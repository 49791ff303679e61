"""Slot snapshots: moshika q4_k LM only, B = 8 slots, one MI355X, one slot at ring fills of 125 and 2 800 rows. In one process, ROUNDS rounds after
WARMUP, the variants alternating inside every round:
  fork / save / load          moshi_hot_slot_fork 0 -> 1, moshi_hot_slot_save of slot 0, moshi_hot_slot_load into slot 1 (the planned graph: one
                              ring_copy_kernel launch for the 2 x 32 ring copies), and the same three under backend flag 1 (no fusion: 64 generic strided copies)
  live_step / live_step_fork  a frame step of live slot 4 alone, and with a fork 0 -> 1 in front of it
  prefill                     moshi_hot_slot_prefill of a history of the same length into slot 1 (what a snapshot replaces; runs last)
Times are host clocks around calls that end in a device synchronise (the calls block). bytes_per_s of a fork = 2 x the ring bytes copied (read plus
write) over the call's time, against the 8 TB/s HBM roofline of DESIGN.md: the call includes building and planning the graph, so it is a lower bound
of the kernel's own rate. One JSON line per configuration.
    python tests/microbench/slot_state_bench.py [--out FILE] [--no-prefill]"""
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

WARMUP, ROUNDS, B, FILLS, LIVE = 1, 5, 8, (125, 2800), 4
HBM_BYTES_PER_S = 8e12
pkg = load_package()
L = pkg.load()
from moshi_cpp_amd import hot  # noqa: E402


class Bench:
    def __init__(self, be):
        cfg = hot.moshika(L)
        cfg.enable_mimi_encoder = cfg.enable_mimi_decoder = 0
        self.be, self.cfg = be, cfg
        self.m = L.moshi_hot_create_slots(be, C.byref(cfg), 0, B)
        assert self.m
        assert L.moshi_hot_slot_open(self.m, 0) == 0 and L.moshi_hot_slot_open(self.m, LIVE) == 0
        assert L.moshi_hot_slot_hold(self.m, 0, 1) == 0   # the source stays at its fill while the live slot steps
        rng = np.random.default_rng(1)
        n_in, dq = cfg.n_q - cfg.dep_q, cfg.dep_q
        self.codes = np.ascontiguousarray(rng.integers(0, cfg.card, B * n_in).astype(np.int32))
        self.txt, self.aud, self.st = np.zeros(B, np.int32), np.zeros(B * dq, np.int32), np.zeros(B, np.int32)
        self.history = np.ascontiguousarray(np.concatenate([rng.integers(0, cfg.text_card, (max(FILLS), 1)),
                                                            rng.integers(0, cfg.card, (max(FILLS), cfg.n_q))], axis=1).astype(np.int32))
        self.blob = None

    def sync(self):
        L.ggml_backend_synchronize(self.be)

    def set_fill(self, fill):
        L.moshi_hot_slot_set_fill(self.m, 0, fill)
        L.moshi_hot_slot_set_fill(self.m, LIVE, fill)
        n = L.moshi_hot_slot_save(self.m, 0, None, 0)
        assert n > 0
        self.blob = np.zeros(n, np.uint8)

    def ring_bytes(self, fill):
        return 2 * self.cfg.num_layers * self.cfg.dim * min(fill, self.cfg.context) * 2

    def timed(self, fn):
        self.sync(); t0 = time.perf_counter()
        fn()
        self.sync(); return time.perf_counter() - t0

    def fork(self):
        dt = self.timed(lambda: L.moshi_hot_slot_fork(self.m, 0, 1))
        assert L.moshi_hot_slot_close(self.m, 1) == 0
        return dt

    def save(self):
        return self.timed(lambda: L.moshi_hot_slot_save(self.m, 0, self.blob.ctypes.data, self.blob.nbytes))

    def load(self):   # (after a save: the blob is slot 0's)
        dt = self.timed(lambda: L.moshi_hot_slot_load(self.m, 1, self.blob.ctypes.data, self.blob.nbytes))
        assert L.moshi_hot_slot_close(self.m, 1) == 0
        return dt

    def step(self):
        L.moshi_hot_lm_step_slots(self.m, self.codes.ctypes.data, self.txt.ctypes.data, self.aud.ctypes.data, self.st.ctypes.data)

    def live_step(self, fill):
        L.moshi_hot_slot_set_fill(self.m, LIVE, fill)
        return self.timed(self.step)

    def live_step_fork(self, fill):
        L.moshi_hot_slot_set_fill(self.m, LIVE, fill)

        def both():
            assert L.moshi_hot_slot_fork(self.m, 0, 1) == 0
            self.step()
        dt = self.timed(both)
        assert L.moshi_hot_slot_close(self.m, 1) == 0
        return dt

    def prefill(self, fill):
        assert L.moshi_hot_slot_open(self.m, 1) == 0
        dt = self.timed(lambda: L.moshi_hot_slot_prefill(self.m, 1, self.history.ctypes.data, fill, 64))
        assert L.moshi_hot_slot_position(self.m, 1) == fill
        assert L.moshi_hot_slot_close(self.m, 1) == 0
        return dt

    def free(self):
        L.moshi_hot_free(self.m)


def line(config, fill, ts, **extra):
    ms = [t * 1e3 for t in ts]
    d = {"config": config, "fill": fill, "ms": round(statistics.median(ms), 4), "rounds_ms": [round(t, 4) for t in ms], "spread_ms": round(max(ms) - min(ms), 4),
         "n_slots": B, "rounds": len(ms)}
    d.update(extra)
    return d


def write(path, lines):
    if path:
        with open(path, "w") as f:
            json.dump({"bench": "slot_state_bench", "model": "moshika q4_k, LM only", "lines": lines}, f, indent=1)
            f.write("\n")


def main():
    args = sys.argv[1:]
    out_path = args[args.index("--out") + 1] if "--out" in args else None
    L.ggml_backend_load_all()
    be = L.ggml_backend_init_by_type(pkg.DEV_GPU, None)
    assert be, "no MI355X device"
    b = Bench(be)
    lines = []

    def emit(l):
        lines.append(l)
        print(json.dumps(l), flush=True)
        write(out_path, lines)

    for fill in FILLS:
        b.set_fill(fill)
        ops = ("fork", "save", "load")
        times = {(op, fl): [] for op in ops for fl in (0, 1)}
        plan = {}
        for r in range(WARMUP + ROUNDS):
            for fl in (0, 1):
                L.ggml_backend_mi355x_set_flags(be, fl)          # (drops the cached plans; outside the clocks)
                for op in ops:
                    dt = getattr(b, op)()
                    if r >= WARMUP:
                        times[(op, fl)].append(dt)
                    if op == "fork":
                        st = pkg.Stats()
                        L.ggml_backend_mi355x_get_stats(be, C.byref(st))
                        plan[fl] = (int(st.kernels_in_last_plan), int(st.ring_copy_launches_in_last_plan), int(st.ring_copy_jobs_in_last_plan))
        L.ggml_backend_mi355x_set_flags(be, 0)
        moved = 2 * b.ring_bytes(fill)
        for fl in (0, 1):
            for op in ops:
                extra = {"backend_flags": fl, "blob_bytes": int(b.blob.nbytes)}
                if op == "fork":
                    rate = moved / statistics.median(times[(op, fl)])
                    extra.update({"bytes_moved": moved, "bytes_per_s": round(rate, 1), "share_of_8TBps": round(rate / HBM_BYTES_PER_S, 4),
                                  "kernels_in_plan": plan[fl][0], "ring_copy_launches": plan[fl][1], "ring_copy_jobs": plan[fl][2]})
                emit(line(op + ("_generic" if fl else ""), fill, times[(op, fl)], **extra))
        # a live neighbour's frame, with and without a fork between its frames (alternating)
        live = {"live_step": [], "live_step_fork": []}
        for r in range(2 * WARMUP + 2 + ROUNDS):     # (the step graphs are re-planned and captured after the flag changes above)
            for k in live:
                dt = getattr(b, k)(fill)
                if r >= 2 * WARMUP + 2:
                    live[k].append(dt)
        for k in live:
            emit(line(k, fill, live[k]))
        emit({"config": "summary", "fill": fill, "fork_adds_to_live_step_ms": round((statistics.median(live["live_step_fork"]) - statistics.median(live["live_step"])) * 1e3, 4),
              "generic_over_planned_fork": round(statistics.median(times[("fork", 1)]) / statistics.median(times[("fork", 0)]), 3)})
    if "--no-prefill" not in args:
        for fill in FILLS:
            ts = [b.prefill(fill) for _ in range(3)]
            emit(line("prefill", fill, ts[1:], passes=(fill + 63) // 64))
    b.free()
    L.ggml_backend_free(be)


if __name__ == "__main__":
    main()
