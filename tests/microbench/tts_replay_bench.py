"""Replay on tts slots: hot.tts_like (Q8_0, context 500, cross_len 64), LM only, B = 8 slots, one MI355X. What it takes to bring a slot to the state
after 256 frames of history:
  replay_1x256   moshi_hot_slot_replay: one job of 256 frames (four passes of 64 rows)
  replay_4x64    moshi_hot_slots_replay: four jobs of 64 frames (slots 0 .. 3) in one call (four passes of 64 rows too, each another column's)
  live_256       the same 256 frames stepped live through moshi_hot_lm_step_slots_text with the slot alone open - the only way before replay existed
Each configuration runs in a process of its own (MI355X_NO_CROSS_ATTN_FUSION is read once per process): `fused`, `plain` (that switch set) and `live`,
ROUNDS timed rounds after WARMUP, the slots reopened at position 0 outside the clock; host clock around work that ends in a device synchronise.
    python tests/microbench/tts_replay_bench.py [--out FILE]          all three children, one JSON line each
    python tests/microbench/tts_replay_bench.py --child live          one child (runs on a tree without the replay calls too: the baseline of the parent commit)"""
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

FRAMES, B, WARMUP, ROUNDS, LIVE_ROUNDS = 256, 8, 2, 9, 3


def child(kind):
    from __graft_entry__ import load_package
    pkg = load_package()
    L = pkg.load()
    from moshi_cpp_amd import hot
    L.ggml_backend_load_all()
    be = L.ggml_backend_init_by_type(pkg.DEV_GPU, None)
    assert be, "no MI355X device"
    cfg = hot.tts_like(L)
    cfg.enable_mimi_encoder = cfg.enable_mimi_decoder = 0
    m = L.moshi_hot_create_slots(be, C.byref(cfg), 0, B)
    assert m
    rng = np.random.default_rng(1)
    ncb = cfg.n_q + 1
    for b in range(B):
        s = (rng.standard_normal(cfg.dim) * 0.1).astype(np.float32)
        x = rng.standard_normal((cfg.cross_len, cfg.dim)).astype(np.float32)
        assert hot.set_conditions_column(L, m, b, s, x) == 0
    text = ((rng.integers(-1, cfg.text_card, FRAMES) + 1) * (cfg.text_card + 1) + rng.integers(0, cfg.text_card, FRAMES)).astype(np.int32)
    frames = np.ascontiguousarray(np.concatenate([text.reshape(-1, 1), rng.integers(0, cfg.card, (FRAMES, ncb - 1))], axis=1).astype(np.int32))

    def sync():
        L.ggml_backend_synchronize(be)

    def reopen(slots):
        for b in range(B):
            L.moshi_hot_slot_close(m, b)
        for b in slots:
            assert L.moshi_hot_slot_open(m, b) == 0

    def replay(slots, rows):
        reopen(slots)
        n = len(slots)
        s = (C.c_int32 * n)(*slots)
        p = (C.c_void_p * n)(*[frames[i * rows:].ctypes.data for i in range(n)])
        c = (C.c_int32 * n)(*([rows] * n))
        sync(); t0 = time.perf_counter()
        assert L.moshi_hot_slots_replay(m, n, s, p, c, 64) == n * rows
        sync(); return time.perf_counter() - t0

    def live():
        reopen([0])
        txt, aud, st = np.zeros(B, np.int32), np.zeros(B * cfg.dep_q, np.int32), np.zeros(B, np.int32)
        tin = np.full(B, hot.TEXT_KEEP, np.int64).astype(np.int32)
        sync(); t0 = time.perf_counter()
        for i in range(FRAMES):
            tin[0] = text[i]
            L.moshi_hot_lm_step_slots_text(m, None, tin.ctypes.data, txt.ctypes.data, aud.ctypes.data, st.ctypes.data)
        sync(); return time.perf_counter() - t0

    units = {"live_256": live} if kind == "live" else {"replay_1x256": lambda: replay([0], FRAMES), "replay_4x64": lambda: replay([0, 1, 2, 3], FRAMES // 4)}
    rounds = LIVE_ROUNDS if kind == "live" else ROUNDS
    times = {k: [] for k in units}
    for k, fn in units.items():
        for _ in range(1 if kind == "live" else WARMUP):
            fn()
    for _ in range(rounds):
        for k, fn in units.items():
            times[k].append(fn())
    line = {"child": kind, "frames": FRAMES, "n_slots": B, "rounds": rounds,
            "device": L.ggml_backend_dev_description(L.ggml_backend_get_device(be)).decode() if hasattr(L, "ggml_backend_dev_description") else "MI355X"}
    for k, ts in times.items():
        ms = [t * 1e3 for t in ts]
        line[k] = {"ms": round(statistics.median(ms), 3), "rounds_ms": [round(t, 3) for t in ms], "spread_ms": round(max(ms) - min(ms), 3),
                   "ms_per_frame": round(statistics.median(ms) / FRAMES, 4)}
    if kind != "live":
        st = pkg.Stats()
        L.ggml_backend_mi355x_get_stats(be, C.byref(st))
        line["last_pass_plan"] = {"kernels": st.kernels_in_last_plan, "cross_block_launches": st.cross_block_launches_in_last_plan,
                                  "cross_block_jobs": st.cross_block_jobs_in_last_plan, "attn_block_launches": st.attn_block_launches_in_last_plan,
                                  "generic_attention_nodes": st.generic_attention_nodes_in_last_plan}
    print(json.dumps(line), flush=True)
    L.moshi_hot_free(m)
    L.ggml_backend_free(be)


def main():
    if sys.argv[1:2] == ["--child"]:
        return child(sys.argv[2])
    out_path = sys.argv[2] if sys.argv[1:2] == ["--out"] else None
    lines = []
    for kind in ("fused", "plain", "live"):
        env = dict(os.environ)
        if kind == "plain":
            env["MI355X_NO_CROSS_ATTN_FUSION"] = "1"
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", kind], capture_output=True, text=True, env=env, timeout=900)
        assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
        lines.append(json.loads(r.stdout.strip().splitlines()[-1]))
        print(json.dumps(lines[-1]), flush=True)
    if out_path:
        with open(out_path, "w") as f:
            json.dump({"bench": "tts_replay_bench", "model": "hot.tts_like q8_0, LM only, context 500, cross_len 64", "lines": lines}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
