"""The f64-MFMA mat-mul for F32 weights (f32_matrix = 1, include/moshi_hot.h) on one MI355X: decoder slots and encoder slots at Mimi's own size
(8 RVQ levels of 2048 codes), every slot open, B = 2 / 8 / 16 / 32 / 64.
  decode_B<B>  ms per moshi_hot_mimi_decode_slots call, the option off and on
  encode_B<B>  ms per moshi_hot_mimi_encode_slots call, the option off and on
The two models of a pair live in one process on two handles of one device (the option belongs to the handle: the "on" model sits on a sibling stream
handle, ggml_backend_mi355x_init_stream) and are fed the same inputs. After a warm-up of both, ROUNDS rounds alternate FRAMES frames of "off" with
FRAMES frames of "on", wall clock around work that ends in the call's own read-back and a synchronise. One JSON line per pair: every round of both,
the medians, off / on, the launches of the plan and the f64-MFMA linears in it, and the max-abs difference of the two models' last outputs.
    python tests/microbench/f32_matrix_bench.py [--out FILE]
    python tests/microbench/f32_matrix_bench.py --trace decode|encode B     (a kernel-trace run of its own: plain launches, TRACE_FRAMES frames of
                                                                             "off", then of "on" - mul_mat_kernel against mm_mfma_kernel<mm_op_f64_f32, NT>)"""
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

FRAMES, ROUNDS, WARMUP, TRACE_FRAMES = 25, 5, 10, 30
BATCHES = (2, 8, 16, 32, 64)
pkg = load_package()
L = pkg.load()
from moshi_cpp_amd import hot  # noqa: E402


def config(what, wide, on):
    cfg = hot.moshika(L)
    cfg.enable_lm, cfg.enable_mimi_encoder, cfg.enable_mimi_decoder = 0, int(what == "encode"), int(what == "decode")
    cfg.mimi_n_q, cfg.mimi_codebook_size = 8, 2048
    cfg.wide_streams = 1 if wide else 0
    cfg.f32_matrix = on
    return cfg


class Side:
    """one codec-slots model (decoder or encoder) with every slot open"""

    def __init__(self, be, what, B, on):
        self.be, self.what, self.B = be, what, B
        cfg = config(what, B > 16, on)
        create = L.moshi_hot_create_codec_slots if what == "decode" else L.moshi_hot_create_encoder_slots
        self.m = create(be, C.byref(cfg), 0, B)
        assert self.m, f"no {what} slots model at B = {B}"
        for b in range(B):
            assert L.moshi_hot_codec_slot_open(self.m, b) == 0
        self.pcm, self.codes, self.status = np.zeros((B, 1920), np.float32), np.zeros((B, 8), np.int32), np.zeros(B, np.int32)

    def frame(self, inp):
        if self.what == "decode":
            r = L.moshi_hot_mimi_decode_slots(self.m, inp.ctypes.data, self.pcm.ctypes.data, self.status.ctypes.data)
        else:
            r = L.moshi_hot_mimi_encode_slots(self.m, inp.ctypes.data, self.codes.ctypes.data, self.status.ctypes.data)
        assert r == self.B

    def stats(self):
        st = pkg.Stats()
        L.ggml_backend_mi355x_get_stats(self.be, C.byref(st))
        return st

    def free(self):
        L.moshi_hot_free(self.m)


def inputs(what, B, n, rng):
    if what == "decode":
        return np.ascontiguousarray(rng.integers(0, 2048, (n, B, 8)).astype(np.int32))
    t = np.arange(n * 1920) / 24000.0
    tone = 0.3 * np.sin(2 * np.pi * (110.0 * (1 + np.arange(B)[:, None] % 7)) * t[None, :]) + 0.05 * rng.standard_normal((B, t.size))
    return np.ascontiguousarray(tone.astype(np.float32).reshape(B, n, 1920).transpose(1, 0, 2))


def handles(flags=0):
    L.ggml_backend_load_all()
    be = L.ggml_backend_init_by_type(pkg.DEV_GPU, None)
    assert be, "no MI355X device"
    if flags:
        L.ggml_backend_mi355x_set_flags(be, flags)
    be_on = L.ggml_backend_mi355x_init_stream(be)     # its own plan cache and option; inherits the flags
    assert be_on
    return be, be_on


def bench(out_path):
    be, be_on = handles()
    rng = np.random.default_rng(1)
    lines = []
    for what in ("decode", "encode"):
        for B in BATCHES:
            sides = {"off": Side(be, what, B, 0), "on": Side(be_on, what, B, 1)}
            inp = inputs(what, B, FRAMES, rng)
            for k in range(WARMUP):
                for s in sides.values():
                    s.frame(inp[k])
            ms = {"off": [], "on": []}
            for _ in range(ROUNDS):
                for name, s in sides.items():
                    L.ggml_backend_synchronize(s.be)
                    t0 = time.perf_counter()
                    for k in range(FRAMES):
                        s.frame(inp[k])
                    L.ggml_backend_synchronize(s.be)
                    ms[name].append((time.perf_counter() - t0) / FRAMES * 1e3)
            st = {name: s.stats() for name, s in sides.items()}
            off, on = statistics.median(ms["off"]), statistics.median(ms["on"])
            a, b = (sides["off"].pcm, sides["on"].pcm) if what == "decode" else (sides["off"].codes, sides["on"].codes)
            line = {"config": f"{what}_B{B}", "off_ms_per_call": round(off, 4), "on_ms_per_call": round(on, 4), "off_over_on": round(off / on, 3),
                    "off_rounds_ms": [round(t, 4) for t in ms["off"]], "on_rounds_ms": [round(t, 4) for t in ms["on"]],
                    "launches_per_call": {n: int(s.kernels_in_last_plan) for n, s in st.items()},
                    "f32_matrix_mms": {n: int(s.f32_matrix_mms_in_last_plan) for n, s in st.items()},
                    "frames_per_round": FRAMES, "rounds": ROUNDS, "warmup_frames": WARMUP}
            if what == "decode":
                line["max_abs_pcm_difference_last_frame"] = float(np.abs(a - b).max())
            else:
                line["codes_equal_last_frame"] = float(np.mean(a == b))
            lines.append(line)
            print(json.dumps(line), flush=True)
            for s in sides.values():
                s.free()
    if out_path:
        with open(out_path, "w") as f:
            json.dump({"bench": "f32_matrix_bench", "model": "Mimi decoder / encoder slots, 8 RVQ levels, F32 transformer / F16 convolutions", "lines": lines}, f, indent=1)
            f.write("\n")
    L.ggml_backend_free(be_on)
    L.ggml_backend_free(be)


def trace(what, B):
    be, be_on = handles(flags=2)                      # no hipGraph capture: the tracer sees every launch
    inp = inputs(what, B, TRACE_FRAMES, np.random.default_rng(1))
    for handle, on in ((be, 0), (be_on, 1)):
        s = Side(handle, what, B, on)
        for k in range(TRACE_FRAMES):
            s.frame(inp[k])
        L.ggml_backend_synchronize(handle)
        print(json.dumps({"trace": what, "B": B, "f32_matrix": on, "frames": TRACE_FRAMES, "f32_matrix_mms": int(s.stats().f32_matrix_mms_in_last_plan)}), flush=True)
        s.free()
    L.ggml_backend_free(be_on)
    L.ggml_backend_free(be)


if __name__ == "__main__":
    if sys.argv[1:2] == ["--trace"]:
        trace(sys.argv[2], int(sys.argv[3]))
    else:
        bench(sys.argv[2] if sys.argv[1:2] == ["--out"] else None)
