"""BF16 checkpoints at B columns: the moshika LM step with BF16 linears and embeddings (lockstep streams, LM only, context 750) at B = 2 .. 64, one fresh
child process per (B, setting). Each child: WARMUP frames, ROUNDS x FRAMES timed frame steps, the median round, then the per-phase times
(moshi_hot_set_timing).

The children run one after another, each under a time limit that kills it, and nothing is started after one that failed or ran out of time (as
wide_streams_bench.py does). Creating the model is ~95 s of host work per child (7.7 G synthetic BF16 weights): the default run is about 25 minutes.
B = 64 runs a quarter of the frames per round (the generic product takes ~0.6 s per step there).

Settings (every switch is read once per process):
  default   the f64-MFMA mat-mul (k_mm_f_batched)
  mmf0      MI355X_MMF=0: the generic float mul_mat (what the parent commit runs)
--mfma-rate first runs tests/microbench/mfma_f64_rate (a bare loop of v_mfma_f64_16x16x4_f64; built with hipcc if the binary is missing) and records its lines.
    python tests/microbench/float_streams_bench.py [--out FILE] [--reps N] [--settings default,mmf0] [--frames N] [--rounds N] [--mfma-rate] [B ...]   (default 2 4 8 16 32 64)"""
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
HERE = os.path.dirname(os.path.abspath(__file__))
WARMUP, CONTEXT = 5, 750
SETTINGS = {"default": {}, "mmf0": {"MI355X_MMF": "0"}}
# floors of a step: every weight byte once at the copy rate, and 2 x parameters x 16 x tiles double FLOPs at the measured MFMA rate
WEIGHT_GB = 13.2 + 1.3 + 0.26
COPY_TBS = 6.29


def child(B, frames, rounds):
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
    cfg.linear_type = cfg.embed_type = pkg.BF16
    setting = os.environ.get("FLOAT_BENCH_SETTING", "default")
    ring_bytes = 2 * cfg.num_layers * cfg.dim * cfg.context * 2 * B
    need = ring_bytes + 20 * (1 << 30)    # the rings, ~15.5 GB of BF16 weights, workspaces
    free, total = torch.cuda.mem_get_info()
    if free < need:
        print(json.dumps({"n_streams": B, "setting": setting, "skipped": f"needs {need >> 20} MiB, {free >> 20} MiB free"}), flush=True)
        return
    L.ggml_backend_load_all()
    be = L.ggml_backend_init_by_type(pkg.DEV_GPU, None)
    assert be, "no MI355X device"
    t_create = time.perf_counter()
    m = L.moshi_hot_create_streams(be, C.byref(cfg), 0, B)
    if not m:
        print(json.dumps({"n_streams": B, "setting": setting, "skipped": "moshi_hot_create_streams returned NULL (allocation)"}), flush=True)
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
    rnd = [timed(frames) for _ in range(rounds)]
    dt = statistics.median(rnd)
    st = pkg.Stats()
    L.ggml_backend_graph_compute(be, L.moshi_hot_graph(m, 0))          # the Temporal plan on its own
    L.ggml_backend_mi355x_get_stats(be, C.byref(st))
    L.moshi_hot_set_timing(m, 1)
    for _ in range(5):
        timed(1)
    us = (C.c_double * 4)()
    L.moshi_hot_get_timing(m, us)
    L.moshi_hot_set_timing(m, 0)
    L.moshi_hot_free(m)
    L.ggml_backend_free(be)
    print(json.dumps({"n_streams": B, "setting": setting, "linear_type": "bf16", "context": CONTEXT, "ms_per_step": round(dt * 1e3, 4),
                      "aggregate_frames_per_s": round(B / dt, 1), "rounds_ms": [round(t * 1e3, 4) for t in rnd], "temporal_us": round(us[1], 1),
                      "depth_us": round(us[2], 1), "kernels_in_temporal_plan": st.kernels_in_last_plan,
                      "float_batched_mms_in_temporal_plan": st.float_batched_mms_in_last_plan, "max_fill": i, "ring_gib": round(ring_bytes / 2 ** 30, 2),
                      "create_s": round(t_create, 1), "frames": frames, "rounds": rounds, "warmup": WARMUP}), flush=True)


CHILD_TIMEOUT = 600   # s: ~95 s to create the model, then at most 5 + 3 x 40 + 5 frames of <= 0.6 s


def run_child(B, setting, frames, rounds):
    env = dict(os.environ, FLOAT_BENCH_SETTING=setting)
    env.pop("MI355X_MMF", None)
    env.update(SETTINGS[setting])
    fr = frames if B <= 32 else max(10, frames // 4)
    try:   # (subprocess.run kills the child when the limit runs out)
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(B), str(fr), str(rounds)], env=env, stdout=subprocess.PIPE, text=True, timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired:
        raise SystemExit(f"child B = {B}, setting {setting} did not end within {CHILD_TIMEOUT} s and was killed: nothing more is started")
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    if p.returncode != 0 or not lines:
        raise SystemExit(f"child B = {B}, setting {setting} ended with status {p.returncode}: nothing more is started")
    return json.loads(lines[-1])


def mfma_rate():
    exe = os.path.join(HERE, "mfma_f64_rate")
    if not os.path.exists(exe):
        subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O2", exe + ".hip", "-o", exe])
    p = subprocess.run([exe], stdout=subprocess.PIPE, text=True, timeout=120)
    if p.returncode != 0:
        raise SystemExit(f"mfma_f64_rate ended with status {p.returncode}: nothing more is started")
    return [json.loads(ln)["mfma_f64_16x16x4"] for ln in p.stdout.splitlines() if ln.startswith("{")]


def main():
    args = sys.argv[1:]
    if args[:1] == ["--child"]:
        return child(int(args[1]), int(args[2]), int(args[3]))
    out, reps, settings, frames, rounds, rate = None, 1, ["default", "mmf0"], 40, 3, False
    while args and args[0].startswith("--"):
        if args[0] == "--mfma-rate":
            rate, args = True, args[1:]
            continue
        if args[0] == "--out":
            out = args[1]
        elif args[0] == "--reps":
            reps = int(args[1])
        elif args[0] == "--settings":
            settings = args[1].split(",")
        elif args[0] == "--frames":
            frames = int(args[1])
        elif args[0] == "--rounds":
            rounds = int(args[1])
        args = args[2:]
    Bs = [int(a) for a in args] or [2, 4, 8, 16, 32, 64]
    result = {"note": f"moshika BF16 LM step, lockstep streams, context {CONTEXT}; {WARMUP} warm-up + {rounds} x {frames} frames from an empty ring; one fresh "
                      f"process per line, one at a time", "lines": [], "ab": []}
    tflops = None
    if rate:
        result["mfma_f64_rate"] = mfma_rate()
        tflops = max(r["tflops"] for r in result["mfma_f64_rate"])
        print(json.dumps(result["mfma_f64_rate"]), flush=True)
    for B in Bs:
        for _ in range(reps):
            for s in settings:   # (alternated)
                result["lines"].append(run_child(B, s, frames, rounds))
                print(json.dumps(result["lines"][-1]), flush=True)
    for B in Bs:
        by_setting = {}
        for line in result["lines"]:
            if line["n_streams"] == B and "ms_per_step" in line:
                by_setting.setdefault(line["setting"], []).append(line["ms_per_step"])
        if by_setting:
            med = {s: round(statistics.median(v), 4) for s, v in by_setting.items()}
            ab = {"n_streams": B, "median_ms_per_step": med, "runs_ms": by_setting, "floor_weight_bytes_once_ms": round(WEIGHT_GB / COPY_TBS, 3)}
            if tflops:   # the kernel multiplies whole 16-column tiles
                ab["floor_f64_mfma_ms"] = round(2 * (WEIGHT_GB / 2) * 16 * ((B + 15) // 16) / tflops, 3)
            if "default" in med and "mmf0" in med:
                ab["speedup_vs_generic"] = round(med["mmf0"] / med["default"], 2)
            print(json.dumps(ab), flush=True)
            result["ab"].append(ab)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
