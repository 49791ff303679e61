"""-m gpu: slot prefill (moshi_hot_slots_prefill) on the MI355X. One scenario throughout: B = 3 slots over a ring of 24; slot 0 is live from frame 0;
after its second frame slots 1 and 2 are opened and take histories of 13 and 6 frames at chunk 8 - passes 8 | 5 + 3 | 3: a job that spans passes, a
ragged 5 = 4 + 1 group, jobs of at most 4 rows - then all three run 8 live frames. Against the slots oracle, with and without the neighbours'
prefill, one call against one call per job, the plan of a two-job pass, and the fused plan against the generic one.

Bars: token ids equal on the contractive model; transformer_out / text logits and Depth logits against the oracle within the per-type bars of
tests/test_hip_frame.py test_batched_prefill_on_the_device_matches_frame_by_frame_oracle (1e-5 / 1e-4 for F32, 5e-2 / 0.2 for quantised weights);
device against device the bar of that test's last assertion (median relative error < 1e-5 for F32, < 1e-2 for quantised weights)."""
import functools

import numpy as np
import pytest

import hot_util as hu
import slot_prefill_util as pu
import streams_util as su
from ggml_util import F32, Q4_0, Q4_K, Q8_0

pytestmark = pytest.mark.gpu
L = hu.L

B, N_BEFORE, N_LIVE = 3, 2, 8
HIST = {1: 13, 2: 6}
TYPES = [(F32, F32), (Q8_0, Q8_0), (Q4_0, Q4_0), (Q4_K, Q4_0)]
IDS = ["f32", "q8_0", "q4_0", "q4_k"]


def make_cfg(lt, et, layers=2):
    cfg = su.lm_only(hu.hot.tiny(L, linear_type=lt, embed_type=et, layers=layers))   # ring of 24 >= 13 history + 8 live frames
    cfg.update_scale = 1.0 / 256   # (include/moshi_hot.h) rounding flips stay local instead of compounding over free-running frames
    return cfg


def hist(cfg, b):
    return pu.history(cfg, HIST[b], seed=60 + b)


@functools.lru_cache(maxsize=None)
def scenario(kind, lt, et, mode="together", flags=0):
    """mode: "together" (one call, both jobs), "apart" (one call per job), "none" (slots 1 and 2 stay closed)
    -> {"after": transformer_out [B, dim] right after the prefill, "frames": per frame (status, texts, audios, text_logits, transformer_out, Depth logits)}"""
    cfg = make_cfg(lt, et)
    s = pu.Slots(kind, cfg, B)
    if kind == "hip" and flags:
        L.ggml_backend_mi355x_set_flags(s.be, flags)
    codes = su.stream_codes(cfg, B, N_BEFORE + N_LIVE, seed=21)
    assert s.open(0) == 0
    out = {"frames": []}
    for k, fr in enumerate(codes):
        if k == N_BEFORE and mode != "none":
            assert s.open(1) == 0 and s.open(2) == 0
            if mode == "together":
                assert s.prefill([(1, hist(cfg, 1)), (2, hist(cfg, 2))], 8) == HIST[1] + HIST[2]
            else:
                assert s.prefill_one(1, hist(cfg, 1), 8) == HIST[1] and s.prefill_one(2, hist(cfg, 2), 8) == HIST[2]
            assert [s.position(b) for b in range(B)] == [N_BEFORE, HIST[1], HIST[2]]
            out["after"] = s.read("transformer_out", cfg.dim)
        r = s.step(fr)
        out["frames"].append(r[1:] + (s.read("text_logits", cfg.text_card), s.read("transformer_out", cfg.dim), s.read(f"dep_logits{cfg.dep_q - 1}", cfg.card)))
    s.free()
    return out


def live_slots(k, mode="together"):
    return range(B) if k >= N_BEFORE and mode != "none" else range(1)


@pytest.mark.parametrize("lt,et", TYPES, ids=IDS)
def test_prefilled_slots_beside_a_live_one_match_the_slots_oracle(lt, et):
    ref, got = scenario("oracle", lt, et), scenario("hip", lt, et)
    text_tol, dep_tol = (1e-5, 1e-4) if lt == F32 else (5e-2, 0.2)
    for b in (1, 2):
        e = hu.rel_err(ref["after"][b], got["after"][b])
        print(f"slot {b}: transformer_out after the prefill: rel err {e:.2e}")
        assert e < text_tol, f"slot {b}: transformer_out after the prefill: rel err {e:.2e}"
    for k, (a, g) in enumerate(zip(ref["frames"], got["frames"])):
        assert a[:3] == g[:3], f"frame {k}: tokens differ: oracle {a[:3]} vs hip {g[:3]}"
        for b in live_slots(k):
            e_out, e_txt, e_dep = hu.rel_err(a[4][b], g[4][b]), hu.rel_err(a[3][b], g[3][b]), hu.rel_err(a[5][b], g[5][b])
            print(f"frame {k} slot {b}: transformer_out {e_out:.2e} text logits {e_txt:.2e} Depth logits {e_dep:.2e}")
            assert e_out < text_tol and e_txt < text_tol and e_dep < dep_tol, (k, b, e_out, e_txt, e_dep)
    assert any(st == [1, 1, 1] for st, _, _, _, _, _ in ref["frames"])


def test_live_neighbour_is_bit_identical_with_and_without_the_prefill():
    a, b = scenario("hip", Q4_K, Q4_0, "none"), scenario("hip", Q4_K, Q4_0)
    for k, (x, y) in enumerate(zip(a["frames"], b["frames"])):
        assert x[0][0] == y[0][0] and x[1][0] == y[1][0] and x[2][0] == y[2][0], f"frame {k}: slot 0's tokens differ"
        assert np.array_equal(x[3][0], y[3][0]), f"frame {k}: slot 0's text logits differ"
    assert any(x[0][0] == 1 for x in a["frames"])


def device_pair_agrees(lt, x, y, what):
    errs = []
    for k, (a, g) in enumerate(zip(x["frames"], y["frames"])):
        assert a[:3] == g[:3], f"{what} frame {k}: tokens differ: {a[:3]} vs {g[:3]}"
        errs += [hu.rel_err(a[3][b], g[3][b]) for b in live_slots(k)]
    print(f"{what}: text logit errors, sorted: {np.array2string(np.sort(errs), precision=2)}")
    assert np.median(errs) < (1e-5 if lt == F32 else 1e-2), f"{what}: median text logit error {np.median(errs):.2e}"


@pytest.mark.parametrize("lt,et", TYPES, ids=IDS)
def test_one_call_for_both_jobs_against_one_call_per_job(lt, et):
    device_pair_agrees(lt, scenario("hip", lt, et, "apart"), scenario("hip", lt, et), "two jobs per pass vs one")


@pytest.mark.parametrize("lt,et", TYPES, ids=IDS)
def test_fused_plan_against_generic_nodes(lt, et):
    # backend flag 1: no fusion at all - the pass graphs run node by node (column views of the rings, row-range views, copies into row ranges)
    device_pair_agrees(lt, scenario("hip", lt, et, "together", 1), scenario("hip", lt, et), "generic vs fused")
    ref, got = scenario("oracle", lt, et), scenario("hip", lt, et, "together", 1)
    text_tol = 1e-5 if lt == F32 else 5e-2
    for k, (a, g) in enumerate(zip(ref["frames"], got["frames"])):
        assert a[:3] == g[:3], f"generic, frame {k}: tokens differ from the oracle's"
        for b in live_slots(k):
            assert hu.rel_err(a[3][b], g[3][b]) < text_tol, (k, b)


def test_a_pass_of_two_jobs_has_one_launch_pair_per_layer():
    layers = 6
    cfg = make_cfg(Q4_K, Q4_0, layers=layers)
    plans = {}
    for name, jobs in (("two jobs", [(1, 5), (2, 3)]), ("one job", [(1, 8)]), ("three small jobs", [(0, 1), (1, 4), (2, 2)])):
        s = pu.Slots("hip", cfg, B)
        for b, _ in jobs:
            assert s.open(b) == 0
        n = sum(t for _, t in jobs)
        assert s.prefill([(b, pu.history(cfg, t, seed=b)) for b, t in jobs], 8) == n     # one pass
        plans[name] = s.stats()
        s.free()
    for name, n_jobs in (("two jobs", 2), ("one job", 1), ("three small jobs", 3)):
        st = plans[name]
        print(f"{name}: {st.kernels_in_last_plan} launches, {st.attn_block_launches_in_last_plan} attention launches holding "
              f"{st.attn_block_jobs_in_last_plan} blocks, {st.generic_attention_nodes_in_last_plan} generic soft_max / set_rows")
        # per Temporal layer two attention launches (write, attend) whatever the number of jobs - not two per job - and nothing generic
        assert st.attn_block_launches_in_last_plan == 2 * layers, name
        assert st.attn_block_jobs_in_last_plan == n_jobs * layers, name
        assert st.generic_attention_nodes_in_last_plan == 0, name
    # what a second job adds to a pass is per pass, not per layer: its RoPE rows (add, timestep_embedding) and its row of transformer_out (rms_norm,
    # mul, cpy) - at most 5 launches, where one more launch per layer would be 6
    extra = plans["two jobs"].kernels_in_last_plan - plans["one job"].kernels_in_last_plan
    assert 0 <= extra <= 5, f"{extra} more launches for a second job over {layers} layers"
