"""TTS stream slots throughput: hot.tts_like at full width (dim 2048, 16 layers, n_q = dep_q = 32, cross-attention over 64 condition rows, demuxed text,
low-rank Depth embeddings, a weight schedule, delay_steps 16), q8_0, codec halves off. Every column has its own conditions
(moshi_hot_set_conditions_column) and is stepped with a fixed forced text stream (moshi_hot_lm_step_slots_text). For each B:
  B = 1        the existing single-stream model: moshi_hot_set_conditions, a text hook returning the same tokens, moshi_hot_lm_step_n
  B > 1        one B-column model of moshi_hot_create_slots, every slot opened at frame 0
WARMUP steps (past delay_steps, so that every timed step runs the Depth graph), then ROUNDS x FRAMES_PER_ROUND = 125 timed frame steps; the median round
is reported with all rounds beside it, and the Temporal plan's launch count. Prints ONE JSON line.
    python tests/microbench/tts_slots_bench.py [B ...]          (default 1 2 4 8 16)"""
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

FRAMES_PER_ROUND, ROUNDS, WARMUP = 25, 5, 20
pkg = load_package()
L = pkg.load()
from moshi_cpp_amd import hot  # noqa: E402


def tts_cfg():
    cfg = hot.tts_like(L)
    cfg.enable_mimi_encoder = cfg.enable_mimi_decoder = 0
    return cfg


def conditions(cfg, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(cfg.dim) * 0.1).astype(np.float32), rng.standard_normal((cfg.cross_len, cfg.dim)).astype(np.float32)


def text_token(cfg, i, b):
    return ((i % 7) + 1) * (cfg.text_card + 1) + (11 + 3 * i + b) % cfg.text_card   # a demuxed pair: both halves of the text embedding run


class Single:
    def __init__(self, be):
        cfg = tts_cfg()
        self.be, self.B, self.cfg, self.i = be, 1, cfg, 0
        self.m = L.moshi_hot_create(be, C.byref(cfg), 0)
        assert self.m
        s, x = conditions(cfg, 4)
        L.moshi_hot_set_conditions(self.m, s.ctypes.data, x.ctypes.data)
        self.hook = hot.TEXT_HOOK(lambda user, offset, sampled: text_token(cfg, offset, 0))
        L.moshi_hot_set_text_hook(self.m, C.cast(self.hook, C.c_void_p), None)
        self.txt, self.aud = C.c_int32(0), (C.c_int32 * 64)()

    def step(self):
        self.i += 1
        return L.moshi_hot_lm_step_n(self.m, None, 0, C.byref(self.txt), self.aud, None)


class Slots:
    def __init__(self, be, B):
        cfg = tts_cfg()
        self.be, self.B, self.cfg, self.i = be, B, cfg, 0
        self.m = L.moshi_hot_create_slots(be, C.byref(cfg), 0, B)
        assert self.m, B
        for b in range(B):
            assert hot.set_conditions_column(L, self.m, b, *conditions(cfg, 4 + b)) == 0
            assert L.moshi_hot_slot_open(self.m, b) == 0
        self.text = [np.ascontiguousarray(np.array([text_token(cfg, i, b) for b in range(B)], np.int32)) for i in range(64)]
        self.txt, self.st, self.aud = np.zeros(B, np.int32), np.zeros(B, np.int32), np.zeros(B * cfg.dep_q, np.int32)

    def step(self):
        t = self.text[self.i % len(self.text)]
        self.i += 1
        return L.moshi_hot_lm_step_slots_text(self.m, None, t.ctypes.data, self.txt.ctypes.data, self.aud.ctypes.data, self.st.ctypes.data)


def kernels_temporal(r):
    st = pkg.Stats()
    L.ggml_backend_graph_compute(r.be, L.moshi_hot_graph(r.m, 0))   # the Temporal graph once more on its own: its plan is the last one
    L.ggml_backend_mi355x_get_stats(r.be, C.byref(st))
    return int(st.kernels_in_last_plan)


def timed(be, r, n):
    L.ggml_backend_synchronize(be)
    t0 = time.perf_counter()
    for _ in range(n):
        r.step()
    L.ggml_backend_synchronize(be)
    return (time.perf_counter() - t0) / n


def bench(be, B):
    r = Single(be) if B == 1 else Slots(be, B)
    timed(be, r, WARMUP)
    assert WARMUP >= r.cfg.delay_steps
    times = [timed(be, r, FRAMES_PER_ROUND) for _ in range(ROUNDS)]
    dt = statistics.median(times)
    out = {"n_streams": B, "path": "single-stream" if B == 1 else "slots", "ms_per_step": round(dt * 1e3, 4), "aggregate_frames_per_s": round(B / dt, 1),
           "frames_per_s_per_stream": round(1.0 / dt, 1), "real_time_factor_per_stream": round(1.0 / dt / 12.5, 2),
           "rounds_ms": [round(t * 1e3, 4) for t in times], "temporal_plan_launches": kernels_temporal(r)}
    L.moshi_hot_free(r.m)
    return out


def main():
    Bs = [int(a) for a in sys.argv[1:]] or [1, 2, 4, 8, 16]
    L.ggml_backend_load_all()
    be = L.ggml_backend_init_by_type(pkg.DEV_GPU, None)
    assert be, "no MI355X device"
    res = [bench(be, B) for B in Bs]
    L.ggml_backend_free(be)
    print(json.dumps({"bench": "tts_slots", "model": "hot.tts_like q8_0, LM only, cross_len 64, per-column conditions, forced text", "frames_timed": FRAMES_PER_ROUND * ROUNDS,
                      "rounds": ROUNDS, "warmup": WARMUP, "results": res}), flush=True)


if __name__ == "__main__":
    main()
