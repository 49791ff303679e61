"""The one-launch f64-MFMA transposed convolution (bit 1 of f32_matrix, include/moshi_hot.h) on one MI355X: decoder slots at Mimi's own size, every
slot open, B = 2 / 8 / 16 / 32 / 64, f32_matrix = 1 (the partial + finish pair) against f32_matrix = 3 (k_convtr_cols_mfma).
  decode_B<B>  ms per moshi_hot_mimi_decode_slots call, both values
The two models live in one process on two handles of one device and are fed the same codes, as in f32_matrix_bench.py (whose Side, inputs and
handles this uses). After a warm-up of both, ROUNDS rounds alternate FRAMES frames of one with FRAMES frames of the other, wall clock around work
that ends in the call's own read-back and a synchronise. One JSON line per B: every round of both, the medians, their ratio, the spread of the
rounds, the plan's counters and the max-abs difference of the two models' last PCM.
    python tests/microbench/convtr_matrix_bench.py [--out FILE]
    python tests/microbench/convtr_matrix_bench.py --trace B VALUE    (a kernel-trace run of its own: plain launches, TRACE_FRAMES frames of one
                                                                       model - convtr_partial_cols_kernel + convtr_finish_cols_kernel at
                                                                       VALUE = 1, convtr_cols_mfma_kernel at 3)"""
import json
import statistics
import sys
import time

import numpy as np

import f32_matrix_bench as fb

L = fb.L
FRAMES, ROUNDS, WARMUP, TRACE_FRAMES = fb.FRAMES, fb.ROUNDS, fb.WARMUP, fb.TRACE_FRAMES


def bench(out_path):
    be, be_on = fb.handles()
    rng = np.random.default_rng(1)
    lines = []
    for B in fb.BATCHES:
        sides = {"pair": fb.Side(be, "decode", B, 1), "matrix": fb.Side(be_on, "decode", B, 3)}
        inp = fb.inputs("decode", B, FRAMES, rng)
        for k in range(WARMUP):
            for s in sides.values():
                s.frame(inp[k])
        ms = {name: [] for name in sides}
        for _ in range(ROUNDS):
            for name, s in sides.items():
                L.ggml_backend_synchronize(s.be)
                t0 = time.perf_counter()
                for k in range(FRAMES):
                    s.frame(inp[k])
                L.ggml_backend_synchronize(s.be)
                ms[name].append((time.perf_counter() - t0) / FRAMES * 1e3)
        st = {name: s.stats() for name, s in sides.items()}
        med = {name: statistics.median(v) for name, v in ms.items()}
        line = {"config": f"decode_B{B}", "pair_ms_per_call": round(med["pair"], 4), "matrix_ms_per_call": round(med["matrix"], 4),
                "pair_over_matrix": round(med["pair"] / med["matrix"], 3),
                "round_spread_ms": {name: round(max(v) - min(v), 4) for name, v in ms.items()},
                "rounds_ms": {name: [round(t, 4) for t in v] for name, v in ms.items()},
                "launches_per_call": {n: int(s.kernels_in_last_plan) for n, s in st.items()},
                "convtr_matrix_groups": {n: int(s.convtr_matrix_groups_in_last_plan) for n, s in st.items()},
                "f32_matrix_mms": {n: int(s.f32_matrix_mms_in_last_plan) for n, s in st.items()},
                "max_abs_pcm_difference_last_frame": float(np.abs(sides["pair"].pcm - sides["matrix"].pcm).max()),
                "frames_per_round": FRAMES, "rounds": ROUNDS, "warmup_frames": WARMUP}
        lines.append(line)
        print(json.dumps(line), flush=True)
        for s in sides.values():
            s.free()
    if out_path:
        with open(out_path, "w") as f:
            json.dump({"bench": "convtr_matrix_bench", "model": "Mimi decoder slots, 8 RVQ levels, f32_matrix = 1 against 3", "lines": lines}, f, indent=1)
            f.write("\n")
    L.ggml_backend_free(be_on)
    L.ggml_backend_free(be)


def trace(B, value):
    be, be_on = fb.handles(flags=2)                   # no hipGraph capture: the tracer sees every launch
    s = fb.Side(be, "decode", B, value)
    inp = fb.inputs("decode", B, TRACE_FRAMES, np.random.default_rng(1))
    for k in range(TRACE_FRAMES):
        s.frame(inp[k])
    L.ggml_backend_synchronize(be)
    print(json.dumps({"trace": "decode", "B": B, "f32_matrix": value, "frames": TRACE_FRAMES,
                      "convtr_matrix_groups": int(s.stats().convtr_matrix_groups_in_last_plan)}), flush=True)
    s.free()
    L.ggml_backend_free(be_on)
    L.ggml_backend_free(be)


if __name__ == "__main__":
    if sys.argv[1:2] == ["--trace"]:
        trace(int(sys.argv[2]), int(sys.argv[3]))
    else:
        bench(sys.argv[2] if sys.argv[1:2] == ["--out"] else None)
