"""Wide batches: the moshika q4_k LM step (lockstep streams, LM only) at B = 16, 32, 48 and 64, one fresh child process per (B, setting).
Each child: WARMUP frames, ROUNDS x FRAMES timed frame steps, the median round, then the per-phase times (moshi_hot_set_timing).

Every model is created with context = 750 (64 columns of K / V rings are then about 25 GB instead of 100 GB), B = 16 included, so the lines
compare; the timed frames keep every ring at fills <= 130 live slots, as DESIGN.md section 13's lines do. A child asks torch for the free device
memory before it creates its model and prints a "skipped" line if the model does not fit.

For every B > 32 the one-pass form of the batched mat-muls (33 .. 64 columns per launch) and the two-pass form (MI355X_MMQ_WIDE=0) are timed in
alternation, REPS times each; the switch is read once per process. --settings adds other values of the switch (a mask: 1 the Q4_K split-K kernel,
2 the Q4_K rows kernel, 4 the Q8_0 / Q4_0 kernel).
--linear-type q8_0 times the same model with Q8_0 linears (the family of the tts / stt checkpoints) instead of Q4_K.
    python tests/microbench/wide_streams_bench.py [--out FILE] [--reps N] [--settings default,0[,1,..]] [--linear-type q4_k|q8_0] [B ...]   (default 16 32 48 64)"""
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
FRAMES, WARMUP, ROUNDS, CONTEXT = 40, 5, 3, 750


def child(B):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    from __graft_entry__ import load_package
    pkg = load_package()
    L = pkg.load()
    from moshi_cpp_amd import hot
    cfg = hot.moshika(L)
    cfg.enable_mimi_encoder = cfg.enable_mimi_decoder = 0
    cfg.context = CONTEXT
    cfg.wide_streams = 1
    linear = os.environ.get("WIDE_BENCH_LINEAR_TYPE", "q4_k")
    cfg.linear_type = {"q4_k": pkg.Q4_K, "q8_0": pkg.Q8_0}[linear]
    setting = os.environ.get("MI355X_MMQ_WIDE", "default")
    ring_bytes = 2 * cfg.num_layers * cfg.dim * cfg.context * 2 * B
    need = ring_bytes + (6 if linear == "q4_k" else 11) * (1 << 30)    # the rings, 4.45 GB of Q4_K weights (Q8_0: 8.4 GB), workspaces
    free, total = torch.cuda.mem_get_info()
    if free < need:
        print(json.dumps({"n_streams": B, "mmq_wide": setting, "skipped": f"needs {need >> 20} MiB, {free >> 20} MiB free"}), flush=True)
        return
    L.ggml_backend_load_all()
    be = L.ggml_backend_init_by_type(pkg.DEV_GPU, None)
    assert be, "no MI355X device"
    t_create = time.perf_counter()
    m = L.moshi_hot_create_streams(be, C.byref(cfg), 0, B)
    if not m:
        print(json.dumps({"n_streams": B, "mmq_wide": setting, "skipped": "moshi_hot_create_streams returned NULL (allocation)"}), flush=True)
        return
    t_create = time.perf_counter() - t_create
    n_in, dq = cfg.n_q - cfg.dep_q, cfg.dep_q
    rng = np.random.default_rng(B)
    codes = [np.ascontiguousarray(rng.integers(0, cfg.card, B * n_in).astype(np.int32)) for _ in range(64)]
    txt = np.zeros(B, np.int32)
    aud = np.zeros(B * dq, np.int32)
    i = 0

    def timed(n):
        nonlocal i
        L.ggml_backend_synchronize(be)
        t0 = time.perf_counter()
        for _ in range(n):
            L.moshi_hot_lm_step_streams(m, codes[i % 64].ctypes.data, txt.ctypes.data, aud.ctypes.data)
            i += 1
        L.ggml_backend_synchronize(be)
        return (time.perf_counter() - t0) / n
    timed(WARMUP)
    rounds = [timed(FRAMES) for _ in range(ROUNDS)]
    dt = statistics.median(rounds)
    st = pkg.Stats()
    L.ggml_backend_graph_compute(be, L.moshi_hot_graph(m, 0))          # the Temporal plan on its own
    L.ggml_backend_mi355x_get_stats(be, C.byref(st))
    L.moshi_hot_set_timing(m, 1)
    for _ in range(10):
        timed(1)
    us = (C.c_double * 4)()
    L.moshi_hot_get_timing(m, us)
    L.moshi_hot_set_timing(m, 0)
    L.moshi_hot_free(m)
    L.ggml_backend_free(be)
    print(json.dumps({"n_streams": B, "mmq_wide": setting, "linear_type": linear, "context": CONTEXT, "ms_per_step": round(dt * 1e3, 4),
                      "aggregate_frames_per_s": round(B / dt, 1), "per_stream_frames_per_s": round(1 / dt, 1),
                      "rounds_ms": [round(t * 1e3, 4) for t in rounds], "temporal_us": round(us[1], 1), "depth_us": round(us[2], 1),
                      "kernels_in_temporal_plan": st.kernels_in_last_plan, "max_fill": i, "ring_gib": round(ring_bytes / 2 ** 30, 2),
                      "create_s": round(t_create, 1), "frames": FRAMES, "rounds": ROUNDS, "warmup": WARMUP}), flush=True)


def run_child(B, setting):
    env = dict(os.environ)
    env.pop("MI355X_MMQ_WIDE", None)
    if setting != "default":
        env["MI355X_MMQ_WIDE"] = setting
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(B)], env=env, stdout=subprocess.PIPE, text=True, timeout=600)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    if p.returncode != 0 or not lines:
        raise SystemExit(f"child B = {B}, MI355X_MMQ_WIDE = {setting} ended with status {p.returncode}: nothing more is started")
    return json.loads(lines[-1])


def main():
    args = sys.argv[1:]
    if args[:1] == ["--child"]:
        return child(int(args[1]))
    out, reps, settings = None, 2, ["default", "0"]                   # "default": the switch unset, the library's own choice per kernel family
    while args and args[0].startswith("--"):
        if args[0] == "--out":
            out = args[1]
        elif args[0] == "--reps":
            reps = int(args[1])
        elif args[0] == "--linear-type":
            os.environ["WIDE_BENCH_LINEAR_TYPE"] = args[1]
        elif args[0] == "--settings":
            settings = args[1].split(",")
        args = args[2:]
    Bs = [int(a) for a in args] or [16, 32, 48, 64]
    result = {"note": f"moshika {os.environ.get('WIDE_BENCH_LINEAR_TYPE', 'q4_k')} LM step, lockstep streams, context {CONTEXT}; fills stay <= 130 live slots in the timed rounds "
                      f"({WARMUP} warm-up + {ROUNDS} x {FRAMES} frames from an empty ring); one fresh process per line", "lines": [], "ab": []}
    for B in Bs:
        todo = [(s, r) for r in range(reps) for s in settings] if B > 32 else [("default", 0)]
        by_setting = {}
        for s, _ in todo:
            line = run_child(B, s)
            print(json.dumps(line), flush=True)
            result["lines"].append(line)
            if "ms_per_step" in line:
                by_setting.setdefault(s, []).append(line["ms_per_step"])
        if B > 32 and by_setting:
            ab = {"n_streams": B, "median_ms_per_step": {s: round(statistics.median(v), 4) for s, v in by_setting.items()}, "runs_ms": by_setting}
            print(json.dumps(ab), flush=True)
            result["ab"].append(ab)
    best = {}
    for line in result["lines"]:
        if "aggregate_frames_per_s" in line and line["mmq_wide"] == "default":
            best.setdefault(line["n_streams"], []).append(line["aggregate_frames_per_s"])
    agg = {B: statistics.median(v) for B, v in best.items()}
    if 16 in agg:
        result["aggregate_vs_b16"] = {str(B): {"aggregate_frames_per_s": a, "exceeds_b16": a > agg[16]} for B, a in sorted(agg.items())}
        print(json.dumps(result["aggregate_vs_b16"]), flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
