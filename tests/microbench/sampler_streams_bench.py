"""The SAMPLED B-column LM step: one moshika q4_k LM-only lockstep model per B (moshi_hot_create_streams) in the reference's --bench sampling mode
(Depth temperature 0.8, text temperature 0.7, top-k 250 / 25), warmed up, then ROUNDS x FRAMES timed frame steps of all B streams at once. One JSON
line per B with the median round's ms / step and the launch counts of the Temporal and the Depth plan (1 + dep_q sampler sites per frame).
    python tests/microbench/sampler_streams_bench.py [--seeded] [--rounds N] [B ...]          (default 4 8 16)
--seeded gives every column a seed of its own (moshi_hot_set_sampling: counter-based noise instead of the rand() sweep, same graphs and launches).
A/B against another build: MI355X_LIB=/path/to/libggml-mi355x.so (moshi.cpp_amd/__init__.py); alternate the two and compare medians.
Under rocprofv3 --kernel-trace --stats: SAMPLER_STREAMS_BENCH_FLAGS=2 (no hipGraph capture, every launch shows by name)."""
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

FRAMES, WARMUP, ROUNDS = 40, 5, 3
pkg = load_package()
L = pkg.load()
from moshi_cpp_amd import hot  # noqa: E402


def bench(be, B, seeded, rounds):
    cfg = hot.moshika(L)
    cfg.enable_mimi_encoder = cfg.enable_mimi_decoder = 0
    cfg.temp, cfg.temp_text, cfg.top_k, cfg.top_k_text = 0.8, 0.7, 250, 25
    m = L.moshi_hot_create_streams(be, C.byref(cfg), 0, B)
    assert m, B
    if seeded:
        for b in range(B):
            assert hot.set_sampling(L, m, b, 1000 + b, 0.8, 0.7, 250, 25) == 0
    n_in, dq = cfg.n_q - cfg.dep_q, cfg.dep_q
    rng = np.random.default_rng(B)
    codes = [np.ascontiguousarray(rng.integers(0, cfg.card, B * n_in).astype(np.int32)) for _ in range(WARMUP + FRAMES)]
    txt = np.zeros(B, np.int32)
    aud = np.zeros(B * dq, np.int32)

    def step(i):
        return L.moshi_hot_lm_step_streams(m, codes[i].ctypes.data, txt.ctypes.data, aud.ctypes.data)
    for i in range(WARMUP):
        step(i)
    times = []
    for _ in range(rounds):
        L.ggml_backend_synchronize(be)
        t0 = time.perf_counter()
        for i in range(WARMUP, WARMUP + FRAMES):
            step(i)
        L.ggml_backend_synchronize(be)
        times.append((time.perf_counter() - t0) / FRAMES)
    st = pkg.Stats()
    L.ggml_backend_mi355x_get_stats(be, C.byref(st))
    kernels_depth = st.kernels_in_last_plan                     # (the Depth graph's plan: the last graph of a step)
    # the Temporal graph's plan, computed once more on its own (same inputs, same ring slot)
    L.ggml_backend_graph_compute(be, L.moshi_hot_graph(m, 0))
    L.ggml_backend_mi355x_get_stats(be, C.byref(st))
    kernels_temporal = st.kernels_in_last_plan
    L.moshi_hot_free(m)
    dt = statistics.median(times)
    return {"n_streams": B, "sampled": True, "seeded": bool(seeded), "ms_per_step": round(dt * 1e3, 4), "ms_per_step_rounds": [round(t * 1e3, 4) for t in times],
            "aggregate_frames_per_s": round(B / dt, 1), "kernels_in_last_plan": kernels_depth, "kernels_in_temporal_plan": kernels_temporal,
            "sampler_sites_per_frame": 1 + dq, "frames": FRAMES, "warmup": WARMUP, "rounds": rounds}


def main():
    args = sys.argv[1:]
    seeded = "--seeded" in args
    rounds = ROUNDS
    if "--rounds" in args:
        rounds = int(args[args.index("--rounds") + 1])
        del args[args.index("--rounds"):args.index("--rounds") + 2]
    Bs = [int(a) for a in args if not a.startswith("--")] or [4, 8, 16]
    L.ggml_backend_load_all()
    be = L.ggml_backend_init_by_type(pkg.DEV_GPU, None)
    assert be, "no MI355X device"
    L.ggml_backend_mi355x_set_flags(be, int(os.environ.get("SAMPLER_STREAMS_BENCH_FLAGS", "0")))
    for B in Bs:
        print(json.dumps(bench(be, B, seeded, rounds)), flush=True)
    L.ggml_backend_free(be)


if __name__ == "__main__":
    main()
