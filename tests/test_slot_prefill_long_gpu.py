"""-m gpu: slot prefill past the ring's end (moshi_hot_slots_prefill_long) on the MI355X. B = 3 slots over a ring of 24 (D = 128, H = 4, 2 layers);
seven scenarios, each followed by 8 live frames:
  a  slot 1 takes 37 frames at chunk 10: passes 10 | 10 | 4 (to the ring's end) | 10 | 3 ring-ordered rows
  b  slot 1 takes 53 frames (more than twice the ring) at chunk 0: 24 | 16 | 13
  d  slot 1 is stepped live to position 30, then takes 9 frames at chunk 5
  f  slot 0 is live from frame 0; after its second frame slots 1 and 2 take 11 frames (before the wrap) and 37 frames (past it) in one call at chunk 8
  m  slot 2 takes 26 frames; then ONE pass holds a block piece (slot 1, 5 rows from position 0) and a ring-ordered piece (slot 2, 8 rows from 26)
  t  slots 1 and 2 take 40 and 24 frames; then ONE pass holds two ring-ordered pieces (slot 1, 5 rows from 40; slot 2, 8 rows from 24)
  w  heads of 64 over a ring of 128 (8 heads; the eight-wave instantiation of the attention kernels): slot 1 takes 140 frames, 12 of them ring-ordered
Against the slots oracle, with and without the call beside a live slot, the fused plan against generic nodes, the rows kernel against per-row launches
(a child process with MI355X_NO_ATTN_ROWS=1), and the plan counts of a pass.

Bars: those of tests/test_slot_prefill_gpu.py, quoted: token ids equal; transformer_out / text logits and Depth logits against the oracle within
1e-5 / 1e-4 for F32 and 5e-2 / 0.2 for quantised weights; device against device the median relative text-logit error < 1e-5 for F32, < 1e-2 for
quantised weights. The rows kernel against per-row launches: bit-identical text logits (only the attention launches differ, and they share the body)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import hot_util as hu
import slot_prefill_long_util as lu
import streams_util as su
from ggml_util import F32, Q4_0, Q4_K, Q8_0

pytestmark = pytest.mark.gpu
L = hu.L

B, N_LIVE = 3, 8
TYPES = [(F32, F32), (Q8_0, Q8_0), (Q4_0, Q4_0), (Q4_K, Q4_0)]
IDS = ["f32", "q8_0", "q4_0", "q4_k"]
SCENARIOS = ["a", "b", "d", "f", "m", "t", "w"]


def make_cfg(lt, et, layers=2, wide=False):
    cfg = su.lm_only(hu.hot.tiny(L, linear_type=lt, embed_type=et, layers=layers, context=128 if wide else 24))
    if wide:
        cfg.num_heads = 8          # D = 64 over a ring of 128: the attention kernels take their eight-wave form (D <= 64, C >= 128)
    cfg.update_scale = 1.0 / 256   # (include/moshi_hot.h) rounding flips stay local instead of compounding over free-running frames
    return cfg


def run_scenario(kind, lt, et, name, flags=0, call=True):
    """-> {"after": transformer_out [B, dim] right after the prefill, "frames": per live frame (status, texts, audios, text_logits, transformer_out,
    Depth logits), "slots": the slots that are live in those frames}; call=False (scenario f): slots 1 and 2 stay closed"""
    cfg = make_cfg(lt, et, wide=name == "w")
    s = lu.Slots(kind, cfg, B, flags=flags)
    n_before = {"a": 0, "b": 0, "d": 30, "f": 2, "m": 0, "t": 0, "w": 0}[name]
    codes = su.stream_codes(cfg, B, n_before + N_LIVE, seed=21)
    out = {"frames": [], "slots": [1, 2] if name in "mt" else [1] if name != "f" else [0, 1, 2] if call else [0]}
    if name == "f":
        assert s.open(0) == 0
    else:
        assert s.open(1) == 0
    if name in "mt":
        assert s.open(2) == 0
    for k, fr in enumerate(codes):
        if k == n_before and call:
            if name == "a":
                assert s.prefill_long_one(1, lu.history(cfg, 37, seed=61), 10) == 37
            elif name == "b":
                assert s.prefill_long_one(1, lu.history(cfg, 53, seed=62), 0) == 53
            elif name == "d":
                assert s.position(1) == 30
                assert s.prefill_long_one(1, lu.history(cfg, 9, seed=63), 5) == 9
            elif name == "m":
                assert s.prefill_long_one(2, lu.history(cfg, 26, seed=65), 0) == 26
                assert s.prefill_long([(1, lu.history(cfg, 5, seed=66)), (2, lu.history(cfg, 8, seed=67))], 64) == 13      # one pass
                assert [s.position(b) for b in (1, 2)] == [5, 34]
            elif name == "t":
                assert s.prefill_long([(1, lu.history(cfg, 40, seed=68)), (2, lu.history(cfg, 24, seed=69))], 0) == 64
                assert s.prefill_long([(1, lu.history(cfg, 5, seed=66)), (2, lu.history(cfg, 8, seed=67))], 64) == 13      # one pass
                assert [s.position(b) for b in (1, 2)] == [45, 32]
            elif name == "w":
                assert s.prefill_long_one(1, lu.history(cfg, 140, seed=70), 0) == 140
            else:
                assert s.open(1) == 0 and s.open(2) == 0
                assert s.prefill_long([(1, lu.history(cfg, 11, seed=64)), (2, lu.history(cfg, 37, seed=61))], 8) == 48
                assert [s.position(b) for b in range(B)] == [2, 11, 37]
            out["after"] = s.read("transformer_out", cfg.dim)
        r = s.step(fr)
        if k >= n_before:
            out["frames"].append(r[1:] + (s.read("text_logits", cfg.text_card), s.read("transformer_out", cfg.dim), s.read(f"dep_logits{cfg.dep_q - 1}", cfg.card)))
    s.free()
    return out


scenario = functools.lru_cache(maxsize=None)(run_scenario)


@pytest.mark.parametrize("name", SCENARIOS)
@pytest.mark.parametrize("lt,et", TYPES, ids=IDS)
def test_slots_prefilled_past_the_ring_end_match_the_slots_oracle(lt, et, name):
    ref, got = scenario("oracle", lt, et, name), scenario("hip", lt, et, name)
    text_tol, dep_tol = (1e-5, 1e-4) if lt == F32 else (5e-2, 0.2)
    for b in (s for s in ref["slots"] if s != 0):
        e = hu.rel_err(ref["after"][b], got["after"][b])
        print(f"{name} slot {b}: transformer_out after the prefill: rel err {e:.2e}")
        assert e < text_tol, f"{name} slot {b}: transformer_out after the prefill: rel err {e:.2e}"
    for k, (a, g) in enumerate(zip(ref["frames"], got["frames"])):
        assert a[:3] == g[:3], f"{name} frame {k}: tokens differ: oracle {a[:3]} vs hip {g[:3]}"
        for b in ref["slots"]:
            e_out, e_txt, e_dep = hu.rel_err(a[4][b], g[4][b]), hu.rel_err(a[3][b], g[3][b]), hu.rel_err(a[5][b], g[5][b])
            print(f"{name} frame {k} slot {b}: transformer_out {e_out:.2e} text logits {e_txt:.2e} Depth logits {e_dep:.2e}")
            assert e_out < text_tol and e_txt < text_tol and e_dep < dep_tol, (name, k, b, e_out, e_txt, e_dep)
    assert any(all(st[b] == 1 for b in ref["slots"]) for st, _, _, _, _, _ in ref["frames"])


def test_live_neighbour_is_bit_identical_with_and_without_the_call():
    a, b = scenario("hip", Q4_K, Q4_0, "f", 0, False), scenario("hip", Q4_K, Q4_0, "f")
    for k, (x, y) in enumerate(zip(a["frames"], b["frames"])):
        assert x[0][0] == y[0][0] and x[1][0] == y[1][0] and x[2][0] == y[2][0], f"frame {k}: slot 0's tokens differ"
        assert np.array_equal(x[3][0], y[3][0]), f"frame {k}: slot 0's text logits differ"
    assert any(x[0][0] == 1 for x in a["frames"])


def device_pair_agrees(lt, x, y, what):
    errs = []
    for k, (a, g) in enumerate(zip(x["frames"], y["frames"])):
        assert a[:3] == g[:3], f"{what} frame {k}: tokens differ: {a[:3]} vs {g[:3]}"
        errs += [hu.rel_err(a[3][b], g[3][b]) for b in x["slots"]]
    print(f"{what}: text logit errors, sorted: {np.array2string(np.sort(errs), precision=2)}")
    assert np.median(errs) < (1e-5 if lt == F32 else 1e-2), f"{what}: median text logit error {np.median(errs):.2e}"


@pytest.mark.parametrize("name", ["a", "f"])
@pytest.mark.parametrize("lt,et", TYPES, ids=IDS)
def test_fused_plan_against_generic_nodes(lt, et, name):
    # backend flag 1: no fusion at all - the one-row sequences run node by node in graph order
    device_pair_agrees(lt, scenario("hip", lt, et, name, 1), scenario("hip", lt, et, name), f"{name}: generic vs fused")


def test_generic_plan_runs_the_rows_node_by_node():
    rl, rj, rr, bl, bj, gen, k = pass_counts(2, [(1, 30, 8)], flags=1)
    print(f"flag 1, one ring-ordered piece of 8 rows over 2 layers: {k} launches, {rl} rows launches, {bl} block launches, {gen} generic soft_max / set_rows")
    assert rl == 0 and bl == 0 and gen == 2 * 8 * 3                                     # per layer and row: two set_rows and a soft_max


PASSES = [[(1, 24, 8)], [(1, 3, 5), (2, 24, 8)], [(1, 40, 5), (2, 24, 8)]]   # one ring-ordered piece; beside a block piece; two ring-ordered pieces

ROWS_CHILD = r'''
import sys
import numpy as np
import test_slot_prefill_long_gpu as t
from ggml_util import F32, Q4_0, Q4_K
out = {}
for tag, (lt, et) in (("f32", (F32, F32)), ("q4_k", (Q4_K, Q4_0))):
    for name in t.SCENARIOS:
        r = t.run_scenario("hip", lt, et, name)
        out[f"{tag}_{name}_after"] = r["after"]
        out[f"{tag}_{name}_logits"] = np.stack([f[3] for f in r["frames"]])
        out[f"{tag}_{name}_tokens"] = np.array([f[1] for f in r["frames"]])
out["row_launches"] = np.array([t.pass_counts(2, jobs)[0] for jobs in t.PASSES])
out["block_jobs"] = np.array([t.pass_counts(2, jobs)[4] for jobs in t.PASSES])
np.savez(sys.argv[1], **out)
print("OK")
'''


def test_rows_kernel_is_bit_identical_to_per_row_launches(tmp_path):
    # the same scenarios in a fresh process whose planner leaves every one-row sequence its own launches: only the attention launches differ, and they
    # share attn_decode_body - any difference is a row that read a ring row before the previous row's store was visible
    path = str(tmp_path / "per_row.npz")
    env = dict(os.environ, PYTHONPATH=os.path.dirname(os.path.abspath(__file__)), MI355X_NO_ATTN_ROWS="1")
    r = subprocess.run([sys.executable, "-c", ROWS_CHILD, path], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and "OK" in r.stdout, (r.stdout + r.stderr)[-2000:]
    ref = np.load(path)
    # the switch switches: there every row is a job of a block launch pair (no rows launch), here a rows launch per layer - also in the mixed pass
    # and in the pass of two ring-ordered pieces, whose per-row launches must never hold two rows of one column
    assert ref["row_launches"].tolist() == [0, 0, 0] and [pass_counts(2, jobs)[0] for jobs in PASSES] == [2, 2, 2]
    assert ref["block_jobs"].tolist() == [2 * 8, 2 * (1 + 8), 2 * (5 + 8)]
    for tag, (lt, et) in (("f32", (F32, F32)), ("q4_k", (Q4_K, Q4_0))):
        for name in SCENARIOS:
            got = scenario("hip", lt, et, name)
            assert np.array_equal(ref[f"{tag}_{name}_tokens"], np.array([f[1] for f in got["frames"]])), (tag, name)
            assert np.array_equal(ref[f"{tag}_{name}_after"], got["after"]), (tag, name, "transformer_out after the prefill")
            assert np.array_equal(ref[f"{tag}_{name}_logits"], np.stack([f[3] for f in got["frames"]])), (tag, name, "text logits")


def pass_counts(layers, jobs, flags=0):
    """one pass on a Q4_K model of `layers` layers (flags: backend flags); jobs: [(slot, position before the pass, rows)] -> (row launches, row jobs, rows, block launches,
    block jobs, generic attention nodes, launches) of the pass's plan"""
    cfg = make_cfg(Q4_K, Q4_0, layers=layers)
    s = lu.Slots("hip", cfg, B, flags=flags)
    for b, pos, _ in jobs:
        assert s.open(b) == 0
        s.set_fill(b, pos)
    n = sum(t for _, _, t in jobs)
    assert s.prefill_long([(b, lu.history(cfg, t, seed=b)) for b, _, t in jobs], 64) == n
    st = s.stats()
    out = (int(st.attn_row_launches_in_last_plan), int(st.attn_row_jobs_in_last_plan), int(st.attn_row_rows_in_last_plan), int(st.attn_block_launches_in_last_plan),
           int(st.attn_block_jobs_in_last_plan), int(st.generic_attention_nodes_in_last_plan), int(st.kernels_in_last_plan))
    s.free()
    return out


def test_a_pass_with_ring_ordered_rows_has_one_rows_launch_per_layer():
    layers = 6
    # one ring-ordered piece of 8 rows
    rl, rj, rr, bl, bj, gen, k = pass_counts(layers, [(1, 30, 8)])
    print(f"one ring-ordered piece of 8 rows: {k} launches, {rl} rows launches holding {rj} jobs of {rr} rows, {bl} block launches, {gen} generic soft_max / set_rows")
    assert (rl, rj, rr) == (layers, layers, 8 * layers) and bl == 0 and gen == 0
    # one block piece (5 rows before the wrap) and one ring-ordered piece (8 rows) in one pass
    rl, rj, rr, bl, bj, gen, k = pass_counts(layers, [(1, 3, 5), (2, 24, 8)])
    print(f"a block piece and a ring-ordered piece: {k} launches, {rl} rows launches holding {rj} jobs of {rr} rows, {bl} block launches holding {bj} jobs, {gen} generic")
    assert (rl, rj, rr) == (layers, layers, 8 * layers) and (bl, bj) == (2 * layers, layers) and gen == 0
    # two ring-ordered pieces of two slots share a launch per layer
    rl, rj, rr, bl, bj, gen, k = pass_counts(layers, [(1, 40, 5), (2, 24, 8)])
    print(f"two ring-ordered pieces: {k} launches, {rl} rows launches holding {rj} jobs of {rr} rows, {bl} block launches, {gen} generic")
    assert (rl, rj, rr) == (layers, 2 * layers, 13 * layers) and bl == 0 and gen == 0
