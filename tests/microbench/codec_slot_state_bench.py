"""Codec slot snapshots: the Mimi decoder or encoder alone at Mimi's own size, B = 16 slots, one MI355X, one slot at n = 2 (one frame) and n = 250
(the full ring) live rows. In one process, ROUNDS rounds after WARMUP, the variants alternating inside every round:
  fork / save / load       moshi_hot_codec_slot_fork 0 -> 1, moshi_hot_codec_slot_save of slot 0, moshi_hot_codec_slot_load into slot 1 under the planned
                           graph (one ring_copy_kernel launch for the 16 ring copies, one state_copy_kernel launch for the 11 conv states), and the
                           same three under backend flag 1 (no fusion: 27 generic copies)
  frame                    one moshi_hot_mimi_decode_slots / _encode_slots call with slot 0 open: the scale a server compares against
Times are host clocks around calls that end in a device synchronise (the calls block); a call includes building and planning its scratch graph. One JSON
line per configuration; --out FILE collects the lines of both halves. One run per half, each GPU step under its own time limit, the second only if the
first ended well:
    timeout -k 10 120 python tests/microbench/codec_slot_state_bench.py --half decoder --out profiles/r16_codec_slot_state_bench.json &&
    timeout -k 10 120 python tests/microbench/codec_slot_state_bench.py --half encoder --out profiles/r16_codec_slot_state_bench.json"""
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

WARMUP, ROUNDS, B, FRAMES = 2, 9, 16, (1, 125)   # positions in frames: n = 2 and n = 250 rows
pkg = load_package()
L = pkg.load()
from moshi_cpp_amd import hot  # noqa: E402


class Bench:
    def __init__(self, be, half):
        cfg = hot.moshika(L)
        cfg.enable_lm, cfg.mimi_n_q, cfg.mimi_codebook_size = 0, 8, 2048
        cfg.enable_mimi_decoder, cfg.enable_mimi_encoder = (1, 0) if half == "decoder" else (0, 1)
        self.be, self.cfg, self.dec = be, cfg, half == "decoder"
        self.m = (L.moshi_hot_create_codec_slots if self.dec else L.moshi_hot_create_encoder_slots)(be, C.byref(cfg), 0, B)
        assert self.m
        assert L.moshi_hot_codec_slot_open(self.m, 0) == 0
        rng = np.random.default_rng(1)
        self.codes = np.ascontiguousarray(rng.integers(0, 2048, (B, 8)).astype(np.int32))
        self.pcm = np.ascontiguousarray((0.1 * rng.standard_normal((B, 1920))).astype(np.float32))
        self.status = np.zeros(B, np.int32)
        self.blob = None

    def sync(self):
        L.ggml_backend_synchronize(self.be)

    def set_fill(self, frames):
        L.moshi_hot_codec_slot_set_fill(self.m, 0, frames)
        n = L.moshi_hot_codec_slot_save(self.m, 0, None, 0)
        assert n > 0
        self.blob = np.zeros(n, np.uint8)

    def timed(self, fn):
        self.sync(); t0 = time.perf_counter()
        fn()
        self.sync(); return time.perf_counter() - t0

    def fork(self):
        dt = self.timed(lambda: L.moshi_hot_codec_slot_fork(self.m, 0, 1))
        assert L.moshi_hot_codec_slot_close(self.m, 1) == 0
        return dt

    def save(self):
        return self.timed(lambda: L.moshi_hot_codec_slot_save(self.m, 0, self.blob.ctypes.data, self.blob.nbytes))

    def load(self):   # (after a save: the blob is slot 0's)
        dt = self.timed(lambda: L.moshi_hot_codec_slot_load(self.m, 1, self.blob.ctypes.data, self.blob.nbytes))
        assert L.moshi_hot_codec_slot_close(self.m, 1) == 0
        return dt

    def frame(self, frames):
        L.moshi_hot_codec_slot_set_fill(self.m, 0, frames)   # the slot stays where it is measured
        if self.dec:
            return self.timed(lambda: L.moshi_hot_mimi_decode_slots(self.m, self.codes.ctypes.data, self.pcm.ctypes.data, self.status.ctypes.data))
        return self.timed(lambda: L.moshi_hot_mimi_encode_slots(self.m, self.pcm.ctypes.data, self.codes.ctypes.data, self.status.ctypes.data))

    def free(self):
        L.moshi_hot_free(self.m)


def line(half, config, frames, ts, **extra):
    ms = [t * 1e3 for t in ts]
    d = {"half": half, "config": config, "n_rows": min(2 * frames, 250), "ms": round(statistics.median(ms), 4), "rounds_ms": [round(t, 4) for t in ms],
         "spread_ms": round(max(ms) - min(ms), 4), "n_slots": B, "rounds": len(ms)}
    d.update(extra)
    return d


def write(path, half, lines):
    if not path:
        return
    old = []
    if os.path.exists(path):
        with open(path) as f:
            old = [l for l in json.load(f)["lines"] if l.get("half") != half]
    with open(path, "w") as f:
        json.dump({"bench": "codec_slot_state_bench", "model": "Mimi decoder / encoder alone, 8 RVQ levels, B = 16", "lines": old + lines}, f, indent=1)
        f.write("\n")


def main():
    args = sys.argv[1:]
    half = args[args.index("--half") + 1]
    assert half in ("decoder", "encoder")
    out_path = args[args.index("--out") + 1] if "--out" in args else None
    L.ggml_backend_load_all()
    be = L.ggml_backend_init_by_type(pkg.DEV_GPU, None)
    assert be, "no MI355X device"
    b = Bench(be, half)
    lines = []

    def emit(l):
        lines.append(l)
        print(json.dumps(l), flush=True)
        write(out_path, half, lines)

    for frames in FRAMES:
        b.set_fill(frames)
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
                    st = pkg.Stats()
                    L.ggml_backend_mi355x_get_stats(be, C.byref(st))
                    plan[(op, fl)] = (int(st.kernels_in_last_plan), int(st.ring_copy_launches_in_last_plan), int(st.state_copy_launches_in_last_plan))
        L.ggml_backend_mi355x_set_flags(be, 0)
        for fl in (0, 1):
            for op in ops:
                k, rc, sc = plan[(op, fl)]
                emit(line(half, op + ("_generic" if fl else ""), frames, times[(op, fl)], backend_flags=fl, blob_bytes=int(b.blob.nbytes),
                          kernels_in_plan=k, ring_copy_launches=rc, state_copy_launches=sc))
        ts = [b.frame(frames) for _ in range(2 * WARMUP + 2 + ROUNDS)][2 * WARMUP + 2:]   # (the frame graph is re-planned and captured after the flag changes)
        emit(line(half, "frame", frames, ts))
        summary = {"half": half, "config": "summary", "n_rows": min(2 * frames, 250)}
        for op in ops:
            planned, generic = times[(op, 0)], times[(op, 1)]
            spread = max(max(planned) - min(planned), max(generic) - min(generic))
            summary[op + "_planned_minus_generic_ms"] = round((statistics.median(planned) - statistics.median(generic)) * 1e3, 4)
            summary[op + "_spread_between_rounds_ms"] = round(spread * 1e3, 4)
        emit(summary)
    b.free()
    L.ggml_backend_free(be)


if __name__ == "__main__":
    main()
