"""The one-launch implicit-im2col convolution group (bit 2 of f32_matrix, include/moshi_hot.h) on one MI355X: decoder slots and encoder slots at
Mimi's own size, every slot open, B = 2 / 8 / 16 / 32 / 64, f32_matrix = 3 (today's launches per group) against f32_matrix = 7 (k_conv_cols_mfma).
  decode_B<B>  ms per moshi_hot_mimi_decode_slots call, both values
  encode_B<B>  ms per moshi_hot_mimi_encode_slots call, both values
The two models live in one process on two handles of one device and are fed the same inputs, as in f32_matrix_bench.py (whose Side, inputs and
handles this uses). After a warm-up of both, ROUNDS rounds alternate FRAMES frames of one with FRAMES frames of the other, wall clock around work
that ends in the call's own read-back and a synchronise. One JSON line per pair: every round of both, the medians, their ratio, the spread of the
rounds, the plan's counters and the difference of the two models' last outputs.
    python tests/microbench/conv_matrix_bench.py [--out FILE]
    python tests/microbench/conv_matrix_bench.py --trace decode|encode B VALUE   (a kernel-trace run of its own: plain launches, TRACE_FRAMES frames
                                                                                  of one model - unary / concat / cpy / im2col / conv_cols_* / binary
                                                                                  kernels at VALUE = 3, conv_cols_implicit_mfma_kernel at 7)"""
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
    for what in ("decode", "encode"):
        for B in fb.BATCHES:
            sides = {"launches": fb.Side(be, what, B, 3), "matrix": fb.Side(be_on, what, B, 7)}
            inp = fb.inputs(what, B, FRAMES, rng)
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
            line = {"config": f"{what}_B{B}", "launches_ms_per_call": round(med["launches"], 4), "matrix_ms_per_call": round(med["matrix"], 4),
                    "launches_over_matrix": round(med["launches"] / med["matrix"], 3),
                    "round_spread_ms": {name: round(max(v) - min(v), 4) for name, v in ms.items()},
                    "rounds_ms": {name: [round(t, 4) for t in v] for name, v in ms.items()},
                    "launches_per_call": {n: int(s.kernels_in_last_plan) for n, s in st.items()},
                    "conv_matrix_groups": {n: int(s.conv_matrix_groups_in_last_plan) for n, s in st.items()},
                    "frames_per_round": FRAMES, "rounds": ROUNDS, "warmup_frames": WARMUP}
            if what == "decode":
                line["max_abs_pcm_difference_last_frame"] = float(np.abs(sides["launches"].pcm - sides["matrix"].pcm).max())
            else:
                line["codes_equal_last_frame"] = float(np.mean(sides["launches"].codes == sides["matrix"].codes))
            lines.append(line)
            print(json.dumps(line), flush=True)
            for s in sides.values():
                s.free()
    if out_path:
        with open(out_path, "w") as f:
            json.dump({"bench": "conv_matrix_bench", "model": "Mimi decoder / encoder slots, 8 RVQ levels, f32_matrix = 3 against 7", "lines": lines}, f, indent=1)
            f.write("\n")
    L.ggml_backend_free(be_on)
    L.ggml_backend_free(be)


def trace(what, B, value):
    be, be_on = fb.handles(flags=2)                   # no hipGraph capture: the tracer sees every launch
    s = fb.Side(be, what, B, value)
    inp = fb.inputs(what, B, TRACE_FRAMES, np.random.default_rng(1))
    for k in range(TRACE_FRAMES):
        s.frame(inp[k])
    L.ggml_backend_synchronize(be)
    print(json.dumps({"trace": what, "B": B, "f32_matrix": value, "frames": TRACE_FRAMES,
                      "conv_matrix_groups": int(s.stats().conv_matrix_groups_in_last_plan)}), flush=True)
    s.free()
    L.ggml_backend_free(be_on)
    L.ggml_backend_free(be)


if __name__ == "__main__":
    if sys.argv[1:2] == ["--trace"]:
        trace(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]))
    else:
        bench(sys.argv[2] if sys.argv[1:2] == ["--out"] else None)
