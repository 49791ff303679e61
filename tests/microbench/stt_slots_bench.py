"""STT stream slots throughput: hot.stt_like at full width (dim 2048, 16 layers, 32 input codebooks, 3 extra heads of 6, no Depth transformer), q4_k,
codec halves off. For each B, timed in alternation in one process:
  lockstep     one B-column model of moshi_hot_create_streams
  slots        one B-column model of moshi_hot_create_slots, every slot opened at frame 0
  serial       B single-stream stt models stepped one after another with moshi_hot_lm_step_n(.., &vad): how B callers were served before B-column
               stt models existed (each step ends in its own token read-back, then the VAD head's scratch graph with a second one)
ROUNDS x FRAMES_PER_ROUND = 125 timed frame steps each after WARMUP steps; the median round is reported with all rounds beside it. The Temporal plan's
launch count is read with the heads and from a model built with extra_heads = 0. Prints ONE JSON line.
    python tests/microbench/stt_slots_bench.py [B ...]          (default 2 4 8 16)"""
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

FRAMES_PER_ROUND, ROUNDS, WARMUP = 25, 5, 10
pkg = load_package()
L = pkg.load()
from moshi_cpp_amd import hot  # noqa: E402


def stt_cfg(heads=True):
    cfg = hot.stt_like(L)
    cfg.enable_mimi_encoder = cfg.enable_mimi_decoder = 0
    if not heads:
        cfg.extra_heads = cfg.extra_heads_dim = 0
    return cfg


class Columns:
    def __init__(self, be, B, kind, heads=True):
        cfg = stt_cfg(heads)
        self.be, self.B, self.kind, self.i, self.cfg = be, B, kind, 0, cfg
        self.m = (L.moshi_hot_create_streams if kind == "lockstep" else L.moshi_hot_create_slots)(be, C.byref(cfg), 0, B)
        assert self.m, (B, kind)
        if kind == "slots":
            for b in range(B):
                assert L.moshi_hot_slot_open(self.m, b) == 0
        rng = np.random.default_rng(B)
        self.codes = [np.ascontiguousarray(rng.integers(0, cfg.card, B * cfg.n_q).astype(np.int32)) for _ in range(64)]
        self.txt, self.st = np.zeros(B, np.int32), np.zeros(B, np.int32)
        self.heads = np.zeros(B * max(1, cfg.extra_heads * cfg.extra_heads_dim), np.float32)

    def step(self):
        c = self.codes[self.i % len(self.codes)]
        self.i += 1
        if self.kind == "lockstep":
            r = L.moshi_hot_lm_step_streams(self.m, c.ctypes.data, self.txt.ctypes.data, None)
        else:
            r = L.moshi_hot_lm_step_slots(self.m, c.ctypes.data, self.txt.ctypes.data, None, self.st.ctypes.data)
        if self.cfg.extra_heads:
            L.moshi_hot_last_heads(self.m, self.heads.ctypes.data, self.heads.size)   # (a host copy: the probabilities came back with the tokens)
        return r

    def kernels_temporal(self):
        st = pkg.Stats()
        L.ggml_backend_graph_compute(self.be, L.moshi_hot_graph(self.m, 0))   # the Temporal graph once more on its own: its plan is the last one
        L.ggml_backend_mi355x_get_stats(self.be, C.byref(st))
        return int(st.kernels_in_last_plan)

    def free(self):
        L.moshi_hot_free(self.m)


class Serial:
    """the first B of a pool of single-stream stt models, stepped one after another"""

    def __init__(self, be, pool, B):
        cfg = stt_cfg()
        self.be, self.B, self.i, self.models = be, B, 0, pool[:B]
        rng = np.random.default_rng(100 + B)
        self.codes = [np.ascontiguousarray(rng.integers(0, cfg.card, cfg.n_q).astype(np.int32)) for _ in range(64)]
        self.txt, self.vad, self.aud = C.c_int32(0), C.c_float(0.0), (C.c_int32 * 64)()
        self.n_q = cfg.n_q

    def step(self):
        for m in self.models:
            c = self.codes[self.i % len(self.codes)]
            self.i += 1
            L.moshi_hot_lm_step_n(m, c.ctypes.data, self.n_q, C.byref(self.txt), self.aud, C.byref(self.vad))


def timed(be, r, n):
    L.ggml_backend_synchronize(be)
    t0 = time.perf_counter()
    for _ in range(n):
        r.step()
    L.ggml_backend_synchronize(be)
    return (time.perf_counter() - t0) / n


def bench(be, pool, B):
    runs = {"lockstep": Columns(be, B, "lockstep"), "slots": Columns(be, B, "slots"), "serial": Serial(be, pool, B)}
    for r in runs.values():
        timed(be, r, WARMUP)
    times = {k: [] for k in runs}
    for _ in range(ROUNDS):
        for k, r in runs.items():
            times[k].append(timed(be, r, FRAMES_PER_ROUND))
    bare = Columns(be, B, "slots", heads=False)
    timed(be, bare, 2)
    plan = {"with_heads": runs["slots"].kernels_temporal(), "without_heads": bare.kernels_temporal(), "lockstep_with_heads": runs["lockstep"].kernels_temporal()}
    bare.free()
    out = {"n_streams": B, "temporal_plan_launches": plan}
    for k in runs:
        dt = statistics.median(times[k])
        out[k] = {"ms_per_step": round(dt * 1e3, 4), "aggregate_frames_per_s": round(B / dt, 1), "frames_per_s_per_stream": round(1.0 / dt, 1),
                  "rounds_ms": [round(t * 1e3, 4) for t in times[k]]}
    out["aggregate_speedup_over_serial"] = {k: round(out["serial"]["ms_per_step"] / out[k]["ms_per_step"], 3) for k in ("lockstep", "slots")}
    runs["lockstep"].free()
    runs["slots"].free()
    return out


def main():
    Bs = [int(a) for a in sys.argv[1:]] or [2, 4, 8, 16]
    L.ggml_backend_load_all()
    be = L.ggml_backend_init_by_type(pkg.DEV_GPU, None)
    assert be, "no MI355X device"
    cfg = stt_cfg()
    pool = [L.moshi_hot_create(be, C.byref(cfg), 0) for _ in range(max(Bs))]
    assert all(pool)
    res = [bench(be, pool, B) for B in Bs]
    for m in pool:
        L.moshi_hot_free(m)
    L.ggml_backend_free(be)
    print(json.dumps({"bench": "stt_slots", "model": "hot.stt_like q4_k, LM only, 3 heads x 6", "frames_timed": FRAMES_PER_ROUND * ROUNDS, "rounds": ROUNDS,
                      "warmup": WARMUP, "results": res}), flush=True)


if __name__ == "__main__":
    main()
