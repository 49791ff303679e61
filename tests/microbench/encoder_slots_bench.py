"""Encoder slots on one MI355X: the Mimi encoder alone at Mimi's own size (8 RVQ levels of 2048 codes).
  slots_B<B>   ms per moshi_hot_mimi_encode_slots call at B = 2 / 8 / 16 / 32 / 64 with every slot open, wall clock around work that ends in the
               call's own read-back
  serial       the yardstick in the same process: B consecutive moshi_hot_mimi_encode calls on a single-stream codec-only model (the single-column
               path as it was before encoder slots, default flags), one model for all B
After a warm-up of both, ROUNDS rounds alternate FRAMES frames of the B-column call with FRAMES x B serial calls - ROUNDS x FRAMES = 125 timed frames
per B. One JSON line per B: every round of both with its spread, the medians, their ratio, the launches of the encode plan and its B-column counters;
then a summary with the requirement (one B = 16 call takes less time than the 16 serial calls it replaces).
    python tests/microbench/encoder_slots_bench.py [--out FILE]        (default FILE: profiles/r15_encoder_slots_bench.json)
    python tests/microbench/encoder_slots_bench.py --frames B N         N B-column calls at batch B and nothing else (for a kernel trace)"""
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

FRAMES, ROUNDS, WARMUP = 25, 5, 10
BATCHES = (2, 8, 16, 32, 64)
pkg = load_package()
L = pkg.load()
from moshi_cpp_amd import hot  # noqa: E402


def config(wide):
    cfg = hot.moshika(L)
    cfg.enable_lm, cfg.enable_mimi_encoder, cfg.enable_mimi_decoder = 0, 1, 0
    cfg.mimi_n_q, cfg.mimi_codebook_size = 8, 2048
    cfg.wide_streams = 1 if wide else 0
    return cfg


def tone(rng, n, B):
    """n frames for B columns: a tone per column under a slow envelope plus noise, amplitude ~0.3, float32 [n, B, 1920]"""
    t = np.arange(n * 1920) / 24000.0
    cols = [0.3 * np.sin(2 * np.pi * (110.0 + 37.0 * b) * t) * (0.5 + 0.5 * np.sin(2 * np.pi * 0.7 * t + b)) + 0.05 * rng.standard_normal(t.size) for b in range(B)]
    return np.ascontiguousarray(np.stack(cols, 1).reshape(B, n, 1920).transpose(1, 0, 2).astype(np.float32))


def make_slots(be, B):
    cfg = config(B > 16)
    m = L.moshi_hot_create_encoder_slots(be, C.byref(cfg), 0, B)
    assert m, f"no encoder-slots model at B = {B}"
    for b in range(B):
        assert L.moshi_hot_codec_slot_open(m, b) == 0
    return cfg, m


def frames_only(be, B, n):
    cfg, m = make_slots(be, B)
    pcm = tone(np.random.default_rng(1), FRAMES, B)
    codes, status = np.zeros((B, cfg.mimi_n_q), np.int32), np.zeros(B, np.int32)
    for k in range(n):
        assert L.moshi_hot_mimi_encode_slots(m, pcm[k % FRAMES].ctypes.data, codes.ctypes.data, status.ctypes.data) == B
    L.moshi_hot_free(m)


def main():
    L.ggml_backend_load_all()
    be = L.ggml_backend_init_by_type(pkg.DEV_GPU, None)
    assert be, "no MI355X device"
    if sys.argv[1:2] == ["--frames"]:
        frames_only(be, int(sys.argv[2]), int(sys.argv[3]))
        L.ggml_backend_free(be)
        return
    out_path = sys.argv[2] if sys.argv[1:2] == ["--out"] else os.path.join(ROOT, "profiles", "r15_encoder_slots_bench.json")
    rng = np.random.default_rng(1)
    one_cfg = config(False)
    one = L.moshi_hot_create(be, C.byref(one_cfg), 0)
    assert one
    one_codes = np.zeros(32, np.int32)
    lines = []

    def emit(line):
        lines.append(line)
        print(json.dumps(line), flush=True)
    for B in BATCHES:
        cfg, m = make_slots(be, B)
        pcm = tone(rng, FRAMES, B)
        codes, status = np.zeros((B, cfg.mimi_n_q), np.int32), np.zeros(B, np.int32)

        def slots_frame(k):
            assert L.moshi_hot_mimi_encode_slots(m, pcm[k].ctypes.data, codes.ctypes.data, status.ctypes.data) == B

        def serial_frame(k):
            for b in range(B):
                L.moshi_hot_mimi_encode(one, pcm[k, b].ctypes.data, one_codes.ctypes.data)
        for k in range(WARMUP):
            slots_frame(k)
            serial_frame(k)
        slots_ms, serial_ms = [], []
        for _ in range(ROUNDS):
            for fn, acc in ((slots_frame, slots_ms), (serial_frame, serial_ms)):
                L.ggml_backend_synchronize(be)
                t0 = time.perf_counter()
                for k in range(FRAMES):
                    fn(k)
                L.ggml_backend_synchronize(be)
                acc.append((time.perf_counter() - t0) / FRAMES * 1e3)
        st = pkg.Stats()
        slots_frame(0)
        L.ggml_backend_mi355x_get_stats(be, C.byref(st))
        a, s = statistics.median(slots_ms), statistics.median(serial_ms)
        emit({"config": f"slots_B{B}", "ms_per_call": round(a, 4), "serial_ms_per_frame": round(s, 4), "serial_ms_per_encode": round(s / B, 4),
              "serial_over_slots": round(s / a, 2), "ms_per_column": round(a / B, 4),
              "rounds_ms": [round(t, 4) for t in slots_ms], "serial_rounds_ms": [round(t, 4) for t in serial_ms],
              "round_spread": round((max(slots_ms) - min(slots_ms)) / a, 4), "serial_round_spread": round((max(serial_ms) - min(serial_ms)) / s, 4),
              "launches_per_call": int(st.kernels_in_last_plan), "vq_column_levels": int(st.vq_column_levels_in_last_plan),
              "code_gather_columns": int(st.code_gather_columns_in_last_plan),
              "codec_attn_launches": int(st.codec_attn_launches_in_last_plan), "frames_per_round": FRAMES, "rounds": ROUNDS, "warmup_frames": WARMUP})
        L.moshi_hot_free(m)
    L.moshi_hot_mimi_encode(one, pcm[0, 0].ctypes.data, one_codes.ctypes.data)
    st = pkg.Stats()
    L.ggml_backend_mi355x_get_stats(be, C.byref(st))
    by = {l["config"]: l for l in lines}
    emit({"config": "summary", "single_stream_launches_per_encode": int(st.kernels_in_last_plan),
          "serial_over_slots": {f"B{B}": by[f"slots_B{B}"]["serial_over_slots"] for B in BATCHES},
          "requirement_one_B16_call_faster_than_16_serial_calls": by["slots_B16"]["ms_per_call"] < by["slots_B16"]["serial_ms_per_frame"]})
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump({"bench": "encoder_slots_bench", "model": "Mimi encoder, 8 RVQ levels, F32 transformer / F16 convolutions", "lines": lines}, f, indent=1)
        f.write("\n")
    L.moshi_hot_free(one)
    L.ggml_backend_free(be)


if __name__ == "__main__":
    main()
