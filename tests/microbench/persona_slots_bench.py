"""PersonaPlex slots on one MI355X: PersonaPlex's widths (tools/personaplex-config.json), q4_k, context 2000, the LM alone.
  live      ms per moshi_hot_lm_step_slots frame at B = 2 / 8 / 16 (every slot open at stream position FILL), wall clock, and its Temporal / Depth
            split from a second run in timing mode (moshi_hot_set_timing synchronises around each phase)
  admit     ms to admit ONE persona and FOUR personas (250 voice rows BF16 + 6 silence + 50 text + 6 silence = 312 rows each) into freshly opened
            slots of the B = 8 model with one moshi_hot_slots_persona call at chunk 64
  single    the same 312 rows on a single-stream model of the same configuration: 250 x moshi_hot_lm_step_embedding, then
            moshi_hot_personaplex_system_prompts - all the parent commit offers (x 4 for four callers: it has no batch)
  generic   the admission on a second backend handle with flag 1 (no fusion at all: the pass input runs as embedding sums, row gathers and concat
            copies - and every other node of the pass runs generic too, so this is an upper bound of what the one launch saves, not its price)
  plain     the admission on a third handle with flag 4096: the pass-input matcher alone off (an embedding-sum launch per token piece, a row gather per
            voice piece, the concat copies), everything else fused - what the one launch itself saves
  mixed     one pass of 64 rows that holds both kinds (58 voice rows + 6 silence frames): the only kind of pass whose input is the pass-input launch -
            a pass of voice rows alone is one row gather, a pass of token rows alone the embedding sum of a prefill pass
One JSON line per configuration: every round, the median round, the spread (max - min) over rounds and, for the whole-call lines, the FASTEST round
with the number of rounds that took more than 1.5 x it. Whole-call rounds have been bimodal on every run so far (a round either takes its fast time or
stalls for seconds outside the graphs, the single-stream line included), so the summary's ratios compare fastest rounds with fastest rounds: what
the work costs when nothing stalls. The stalls are a separate, open question (MOSHI_HOT_TIME_SCRATCH=1 prints where a slow scratch graph spent its time).
    python tests/microbench/persona_slots_bench.py [--out FILE]"""
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

STEPS, WARMUP, ROUNDS, FILL, CONTEXT = 20, 5, 5, 1000, 2000
N_VOICE, N_TEXT, SILENCE = 250, 50, 6
ROWS = N_VOICE + 2 * SILENCE + N_TEXT
pkg = load_package()
L = pkg.load()
from moshi_cpp_amd import hot  # noqa: E402


def config():
    cfg = hot.personaplex(L)
    cfg.enable_mimi_encoder = cfg.enable_mimi_decoder = 0
    cfg.context, cfg.persona_columns = CONTEXT, 1
    return cfg


def whole_call(name, rounds, nd, **more):
    """the line of a whole-call configuration: every round; the fastest one and how many rounds stalled beside it"""
    fast = min(rounds)
    return dict({"config": name, "fast_ms": round(fast, nd), "stalled_rounds": sum(t > 1.5 * fast for t in rounds), "ms": round(statistics.median(rounds), nd),
                 "rounds_ms": [round(t, nd) for t in rounds], "spread_ms": round(max(rounds) - min(rounds), nd)}, **more)


def sync(be):
    L.ggml_backend_synchronize(be)


def bf16_bits(x):
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    return ((u + (0x7FFF + ((u >> 16) & 1))) >> 16).astype(np.uint16)


class Personas:
    def __init__(self, cfg, n, n_voice=N_VOICE, n_text=N_TEXT, silence=SILENCE):
        rng = np.random.default_rng(2)
        self.rows = n_voice + 2 * silence + n_text
        self.voice_f32 = [(rng.standard_normal((n_voice, cfg.dim)) * 0.5).astype(np.float32) for _ in range(n)]
        self.voice = [bf16_bits(v).reshape(v.shape) for v in self.voice_f32]
        self.voice_f32 = [(v.astype(np.uint32) << 16).view(np.float32) for v in self.voice]
        self.text = [rng.integers(0, cfg.text_card, n_text).astype(np.int32) for _ in range(n)]
        made = [hot.persona(self.voice[i], pkg.BF16, None, self.text[i], silence) for i in range(n)]
        self.keep = [k for _, k in made]
        self.structs = (hot.Persona * n)(*[p for p, _ in made])


def live_steps(be, cfg, B):
    m = L.moshi_hot_create_slots(be, C.byref(cfg), 0, B)
    assert m, f"no PersonaPlex slots model at B = {B}"
    rng = np.random.default_rng(1)
    codes = np.ascontiguousarray(rng.integers(0, cfg.card, B * (cfg.n_q - cfg.io_dep_q)).astype(np.int32))
    txt, aud, st = np.zeros(B, np.int32), np.zeros(B * cfg.io_dep_q, np.int32), np.zeros(B, np.int32)
    for b in range(B):
        assert L.moshi_hot_slot_open(m, b) == 0
        L.moshi_hot_slot_set_fill(m, b, FILL)

    def step():
        L.moshi_hot_lm_step_slots(m, codes.ctypes.data, txt.ctypes.data, aud.ctypes.data, st.ctypes.data)
    for _ in range(WARMUP):
        step()
    rounds = []
    for _ in range(ROUNDS):
        sync(be); t0 = time.perf_counter()
        for _ in range(STEPS):
            step()
        sync(be); rounds.append((time.perf_counter() - t0) / STEPS * 1e3)
    L.moshi_hot_set_timing(m, 1)
    for _ in range(STEPS):
        step()
    us = (C.c_double * 4)()
    L.moshi_hot_get_timing(m, us)
    L.moshi_hot_set_timing(m, 0)
    return m, {"config": f"live_B{B}", "ms": round(statistics.median(rounds), 4), "rounds_ms": [round(t, 4) for t in rounds], "spread_ms": round(max(rounds) - min(rounds), 4),
               "temporal_ms_timing_mode": round(us[1] / 1e3, 4), "depth_ms_timing_mode": round(us[2] / 1e3, 4), "fill": FILL, "steps": STEPS, "rounds": ROUNDS}


def admissions(be, m, B, p, n_jobs, name):
    """n_jobs personas into slots 0 .. n_jobs - 1, reopened (position 0) before every round"""
    slots = (C.c_int32 * n_jobs)(*range(n_jobs))
    rounds = []
    for r in range(ROUNDS + 1):
        for b in range(n_jobs):
            assert L.moshi_hot_slot_close(m, b) == 0 and L.moshi_hot_slot_open(m, b) == 0
        sync(be); t0 = time.perf_counter()
        assert L.moshi_hot_slots_persona(m, n_jobs, slots, p.structs, 64) == n_jobs * p.rows
        sync(be); dt = (time.perf_counter() - t0) * 1e3
        if r:                                             # round 0 warms the plans up
            rounds.append(dt)
    st = pkg.Stats()
    L.ggml_backend_mi355x_get_stats(be, C.byref(st))
    return whole_call(name, rounds, 3, personas=n_jobs, rows=n_jobs * p.rows, chunk=64, n_slots=B, kernels_in_last_pass_plan=st.kernels_in_last_plan,
                      pass_input_launches_in_last_pass_plan=st.pass_input_launches_in_last_plan, pass_input_rows_in_last_pass_plan=st.pass_input_rows_in_last_plan)


def single_stream(be, cfg, p):
    m = L.moshi_hot_create(be, C.byref(cfg), 0)
    assert m
    rounds = []
    for r in range(ROUNDS + 1):
        L.moshi_hot_set_context_fill(m, 0)
        sync(be); t0 = time.perf_counter()
        for row in p.voice_f32[0]:
            L.moshi_hot_lm_step_embedding(m, row.ctypes.data)
        L.moshi_hot_personaplex_system_prompts(m, p.text[0].ctypes.data, N_TEXT)
        sync(be); dt = (time.perf_counter() - t0) * 1e3
        if r:
            rounds.append(dt)
    L.moshi_hot_free(m)
    return whole_call("single_stream_one_persona", rounds, 3, rows=ROWS)


def main():
    out_path = sys.argv[2] if sys.argv[1:2] == ["--out"] else None
    L.ggml_backend_load_all()
    be = L.ggml_backend_init_by_type(pkg.DEV_GPU, None)
    assert be, "no MI355X device"
    cfg = config()
    p = Personas(cfg, 4)
    mixed = Personas(cfg, 1, n_voice=58, n_text=0, silence=3)
    lines = []

    def emit(line):
        lines.append(line)
        print(json.dumps(line), flush=True)
    for B in (2, 8, 16):
        m, line = live_steps(be, cfg, B)
        emit(line)
        if B == 8:
            emit(admissions(be, m, B, p, 1, "admit_one"))
            emit(admissions(be, m, B, p, 4, "admit_four"))
            emit(admissions(be, m, B, mixed, 1, "mixed_pass"))
        L.moshi_hot_free(m)
    emit(single_stream(be, cfg, p))
    be2 = L.ggml_backend_init_by_type(pkg.DEV_GPU, None)
    L.ggml_backend_mi355x_set_flags(be2, 1)
    m = L.moshi_hot_create_slots(be2, C.byref(cfg), 0, 8)
    assert m
    emit(admissions(be2, m, 8, p, 1, "admit_one_generic_plan"))
    emit(admissions(be2, m, 8, p, 4, "admit_four_generic_plan"))
    emit(admissions(be2, m, 8, mixed, 1, "mixed_pass_generic_plan"))
    L.moshi_hot_free(m)
    L.ggml_backend_free(be2)
    be3 = L.ggml_backend_init_by_type(pkg.DEV_GPU, None)
    L.ggml_backend_mi355x_set_flags(be3, 4096)            # the pass-input matcher alone off: what the one launch itself saves
    m = L.moshi_hot_create_slots(be3, C.byref(cfg), 0, 8)
    assert m
    emit(admissions(be3, m, 8, p, 1, "admit_one_plain_input"))
    emit(admissions(be3, m, 8, mixed, 1, "mixed_pass_plain_input"))
    L.moshi_hot_free(m)
    L.ggml_backend_free(be3)
    fast = {l["config"]: l["fast_ms"] for l in lines if "fast_ms" in l}
    emit({"config": "summary", "of": "fastest rounds",
          "single_stream_over_admit_one": round(fast["single_stream_one_persona"] / fast["admit_one"], 2),
          "four_single_streams_over_admit_four": round(4 * fast["single_stream_one_persona"] / fast["admit_four"], 2),
          "admit_four_over_admit_one": round(fast["admit_four"] / fast["admit_one"], 3),
          "generic_plan_over_fused_one": round(fast["admit_one_generic_plan"] / fast["admit_one"], 3),
          "generic_plan_over_fused_four": round(fast["admit_four_generic_plan"] / fast["admit_four"], 3),
          "mixed_pass_plain_input_minus_fused_ms": round(fast["mixed_pass_plain_input"] - fast["mixed_pass"], 4),
          "stalled_rounds": {l["config"]: l["stalled_rounds"] for l in lines if l.get("stalled_rounds")},
          "depth_share_of_live_step": {f"B{B}": round(next(l for l in lines if l["config"] == f"live_B{B}")["depth_ms_timing_mode"] /
                                                    (next(l for l in lines if l["config"] == f"live_B{B}")["depth_ms_timing_mode"] +
                                                     next(l for l in lines if l["config"] == f"live_B{B}")["temporal_ms_timing_mode"]), 3) for B in (2, 8, 16)}})
    if out_path:
        with open(out_path, "w") as f:
            json.dump({"bench": "persona_slots_bench", "model": f"PersonaPlex q4_k, LM only, context {CONTEXT}", "lines": lines}, f, indent=1)
            f.write("\n")
    L.ggml_backend_free(be)


if __name__ == "__main__":
    main()
