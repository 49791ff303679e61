"""Lockstep streams throughput: one moshika q4_k LM-only model per B (moshi_hot_create_streams), warmed up, then FRAMES timed frame steps of all B
streams at once. One JSON line per B. B = 1 is the single-stream model (moshi_hot_create's, the optimised path) and the yardstick.
    python tests/microbench/streams_bench.py [B ...]          (default 1 2 4 8 16)"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402

FRAMES, WARMUP = 125, 5
pkg = load_package()
L = pkg.load()
from moshi_cpp_amd import hot  # noqa: E402


def bench(be, B):
    cfg = hot.moshika(L)
    cfg.enable_mimi_encoder = cfg.enable_mimi_decoder = 0
    m = L.moshi_hot_create_streams(be, C.byref(cfg), 0, B)
    assert m, B
    n_in, dq = cfg.n_q - cfg.dep_q, cfg.dep_q
    rng = np.random.default_rng(B)
    codes = [np.ascontiguousarray(rng.integers(0, cfg.card, B * n_in).astype(np.int32)) for _ in range(WARMUP + FRAMES)]
    txt = np.zeros(B, np.int32)
    aud = np.zeros(B * dq, np.int32)

    def step(i):
        return L.moshi_hot_lm_step_streams(m, codes[i].ctypes.data, txt.ctypes.data, aud.ctypes.data)
    for i in range(WARMUP):
        step(i)
    L.ggml_backend_synchronize(be)
    t0 = time.perf_counter()
    for i in range(WARMUP, WARMUP + FRAMES):
        step(i)
    L.ggml_backend_synchronize(be)
    dt = (time.perf_counter() - t0) / FRAMES
    st = pkg.Stats()
    L.ggml_backend_mi355x_get_stats(be, C.byref(st))
    kernels_last = st.kernels_in_last_plan                      # (the Depth graph's plan: the last graph of a step)
    # the Temporal graph's plan, computed once more on its own (same inputs, same ring slot)
    L.ggml_backend_graph_compute(be, L.moshi_hot_graph(m, 0))
    L.ggml_backend_mi355x_get_stats(be, C.byref(st))
    kernels_temporal = st.kernels_in_last_plan
    # per-phase wall clock (synchronised around each phase: a few us above the free-running step)
    L.moshi_hot_set_timing(m, 1)
    for i in range(20):
        step(i)
    us = (C.c_double * 4)()
    L.moshi_hot_get_timing(m, us)
    L.moshi_hot_set_timing(m, 0)
    L.moshi_hot_free(m)
    return {"n_streams": B, "ms_per_step": round(dt * 1e3, 4), "aggregate_frames_per_s": round(B / dt, 1), "per_stream_frames_per_s": round(1 / dt, 1),
            "kernels_in_last_plan": kernels_last, "kernels_in_temporal_plan": kernels_temporal,
            "temporal_us": round(us[1], 1), "depth_us": round(us[2], 1), "frames": FRAMES, "warmup": WARMUP}


def main():
    Bs = [int(a) for a in sys.argv[1:]] or [1, 2, 4, 8, 16]
    L.ggml_backend_load_all()
    be = L.ggml_backend_init_by_type(pkg.DEV_GPU, None)
    assert be, "no MI355X device"
    L.ggml_backend_mi355x_set_flags(be, int(os.environ.get("STREAMS_BENCH_FLAGS", "0")))   # 2 = no hipGraph capture (under rocprofv3)
    for B in Bs:
        print(json.dumps(bench(be, B)), flush=True)
    L.ggml_backend_free(be)


if __name__ == "__main__":
    main()
