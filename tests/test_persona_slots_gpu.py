"""-m gpu: PersonaPlex streams and slots on the MI355X. The pass-input launch on its own (a [96, 5] input of token rows, voice rows and a token row
against the oracle, bit for bit, fused and generic); one scenario of B = 3 slots over a ring of 24 - slot 1 is live from frame 0, after its second
frame slots 0 and 2 are opened and take two personas (5 voice rows + 2 silence + 3 text + 2 silence each, one voice F32 with a ring image, one BF16
without) in one call at chunk 7, then all three run 8 live frames - against the slots oracle and with and without the admission; the plan of a
two-job pass; and B = 2 lockstep streams against the batched oracle.

Bars: those of tests/test_slot_prefill_gpu.py - token ids equal on the contractive model; transformer_out / text logits and Depth logits against the
oracle within 1e-5 / 1e-4 for F32 weights and 5e-2 / 0.2 for Q4_K."""
import functools

import numpy as np
import pytest

import ggml_util as gu
import hot_util as hu
import persona_util as pp
from ggml_util import BF16, F32, I32, Q4_0, Q4_K

pytestmark = pytest.mark.gpu
L = hu.L

B, N_BEFORE, N_LIVE = 3, 2, 8
TYPES = [(F32, F32), (Q4_K, Q4_0)]
IDS = ["f32", "q4_k"]


# ---- the kernel ----------------------------------------------------------------------------------------------------------------------------------
def pass_input_graph(table_type, voice_type):
    """-> build(g): token piece (rows 0-1, 17 tables) | voice piece (2 rows) | token piece (row 4) of a [96, 5] input, built as moshi_hot.cpp builds it:
    one index and one scale tensor per table for the whole pass, the pieces take views. 96 columns: the last workgroup of a row has 32 live lanes."""
    K, T, n_tab, n_rows = 96, 5, 17, 40
    rng = np.random.default_rng(3)
    raw = [gu.random_q4_0(rng, n_rows, K) if table_type == Q4_0 else rng.standard_normal((n_rows, K)).astype(np.float32) for _ in range(n_tab)]
    ids = rng.integers(0, n_rows, (n_tab, T)).astype(np.int32)
    scales = np.ones((n_tab, T), np.float32)
    scales[3, 1] = scales[16, 4] = 0.0                      # a -1 token (lm.h:586-607)
    voice = rng.standard_normal((3, K)).astype(np.float32)

    def build(g):
        tabs = [g.input_raw(r, Q4_0, K, n_rows) if table_type == Q4_0 else g.input(r, F32) for r in raw]
        idx = [g.input(ids[i], I32) for i in range(n_tab)]
        sc = [g.input(scales[i].reshape(T, 1), F32) for i in range(n_tab)]

        def tokens(row0, n):
            x = None
            for i in range(n_tab):
                e = g.mul(g.get_rows(tabs[i], g.view_1d(idx[i], n, row0 * 4)), g.view_2d(sc[i], 1, n, 4, row0 * 4))
                x = e if x is None else g.add(x, e)
            return x
        v = g.get_rows(g.input(voice, voice_type), g.input(np.array([2, 0], np.int32), I32))
        return [g.concat(g.concat(tokens(0, 2), v, 1), tokens(4, 1), 1)]
    return build


@pytest.mark.parametrize("table_type,voice_type", [(Q4_0, BF16), (F32, F32)], ids=["q4_0-bf16", "f32-f32"])
def test_pass_input_launch_equals_the_oracle_bit_for_bit(table_type, voice_type):
    build = pass_input_graph(table_type, voice_type)
    (ref,), _ = gu.run_graph("oracle", build)
    (got,), st = gu.run_graph("hip", build)
    (gen,), st_gen = gu.run_graph("hip", build, flags=1)
    assert ref.shape[-2:] == (5, 96) and np.all(np.isfinite(ref)) and np.abs(ref).max() > 0
    assert np.array_equal(ref, got), f"fused: {np.count_nonzero(ref != got)} of {ref.size} values differ, max {np.abs(ref - got).max():.3e}"
    assert np.array_equal(ref, gen), "generic plan"
    assert st.pass_input_launches_in_last_plan == 1 and st.pass_input_rows_in_last_plan == 5
    assert st_gen.pass_input_launches_in_last_plan == 0 and st_gen.pass_input_rows_in_last_plan == 0
    assert st.kernels_in_last_plan < st_gen.kernels_in_last_plan
    # flag 4096: this matcher alone is off - the two embedding sums stay launches of their own, beside the row gather and the two concat copies
    (own,), st_own = gu.run_graph("hip", build, flags=4096)
    assert np.array_equal(ref, own) and st_own.pass_input_launches_in_last_plan == 0
    assert st.kernels_in_last_plan == 1 and st_own.kernels_in_last_plan == 5, (st.kernels_in_last_plan, st_own.kernels_in_last_plan)


# ---- persona slots ---------------------------------------------------------------------------------------------------------------------------------
def make_cfg(lt, et, layers=2):
    cfg = pp.make_cfg(layers=layers, linear_type=lt, embed_type=et)
    cfg.update_scale = 1.0 / 256   # (include/moshi_hot.h) rounding flips stay local instead of compounding over free-running frames
    return cfg


def personas(cfg):
    return pp.Persona(cfg, 11, vtype=F32, cache=True), pp.Persona(cfg, 12, vtype=BF16, cache=False)


@functools.lru_cache(maxsize=None)
def scenario(kind, lt, et, admit=True, flags=0):
    """-> {"after": transformer_out [B, dim] right after the admission, "frames": per frame (status, texts, audios, text_logits, transformer_out, Depth logits)}"""
    cfg = make_cfg(lt, et)
    s = pp.Slots(kind, cfg, B)
    if kind == "hip" and flags:
        L.ggml_backend_mi355x_set_flags(s.be, flags)
    codes = np.random.default_rng(21).integers(0, cfg.card, (N_BEFORE + N_LIVE, B, cfg.io_dep_q)).tolist()
    assert s.open(1) == 0
    out = {"frames": []}
    for k, fr in enumerate(codes):
        if k == N_BEFORE and admit:
            A, Bp = personas(cfg)
            assert s.open(0) == 0 and s.open(2) == 0
            assert s.persona([(0, A), (2, Bp)], 7) == 24
            assert [s.position(b) for b in range(B)] == [12, N_BEFORE, 12]
            out["after"] = s.read("transformer_out", cfg.dim)
        r = s.step(fr)
        out["frames"].append(r[1:] + (s.read("text_logits", cfg.text_card), s.read("transformer_out", cfg.dim), s.read(f"dep_logits{cfg.dep_q - 1}", cfg.card)))
    s.free()
    return out


def live_slots(k, admit=True):
    return range(B) if k >= N_BEFORE and admit else range(1, 2)


@pytest.mark.parametrize("lt,et", TYPES, ids=IDS)
def test_admitted_slots_beside_a_live_one_match_the_slots_oracle(lt, et):
    ref, got = scenario("oracle", lt, et), scenario("hip", lt, et)
    text_tol, dep_tol = (1e-5, 1e-4) if lt == F32 else (5e-2, 0.2)
    for b in (0, 2):
        e = hu.rel_err(ref["after"][b], got["after"][b])
        print(f"slot {b}: transformer_out after the admission: rel err {e:.2e}")
        assert e < text_tol, f"slot {b}: transformer_out after the admission: rel err {e:.2e}"
    for k, (a, g) in enumerate(zip(ref["frames"], got["frames"])):
        assert a[:3] == g[:3], f"frame {k}: tokens differ: oracle {a[:3]} vs hip {g[:3]}"
        for b in live_slots(k):
            e_out, e_txt, e_dep = hu.rel_err(a[4][b], g[4][b]), hu.rel_err(a[3][b], g[3][b]), hu.rel_err(a[5][b], g[5][b])
            print(f"frame {k} slot {b}: transformer_out {e_out:.2e} text logits {e_txt:.2e} Depth logits {e_dep:.2e}")
            assert e_out < text_tol and e_txt < text_tol and e_dep < dep_tol, (k, b, e_out, e_txt, e_dep)
    assert any(st == [1, 1, 1] for st, _, _, _, _, _ in ref["frames"])


def test_live_neighbour_is_bit_identical_with_and_without_the_admission():
    a, b = scenario("hip", Q4_K, Q4_0, False), scenario("hip", Q4_K, Q4_0)
    for k, (x, y) in enumerate(zip(a["frames"], b["frames"])):
        assert x[0][1] == y[0][1] and x[1][1] == y[1][1] and x[2][1] == y[2][1], f"frame {k}: slot 1's tokens differ"
        assert np.array_equal(x[3][1], y[3][1]), f"frame {k}: slot 1's text logits differ"
    assert any(x[0][1] == 1 for x in a["frames"])


def test_generic_plan_agrees_with_the_fused_one():
    # backend flag 1: the pass input runs as its plain nodes (embedding sums, row gathers, concat copies)
    x, y = scenario("hip", Q4_K, Q4_0, True, 1), scenario("hip", Q4_K, Q4_0)
    errs = []
    for k, (a, g) in enumerate(zip(x["frames"], y["frames"])):
        assert a[:3] == g[:3], f"frame {k}: tokens differ: {a[:3]} vs {g[:3]}"
        errs += [hu.rel_err(a[3][b], g[3][b]) for b in live_slots(k)]
    assert np.median(errs) < 1e-2, f"median text logit error {np.median(errs):.2e}"   # (the device-against-device bar of tests/test_slot_prefill_gpu.py)


def test_a_pass_of_two_jobs_has_one_input_launch_and_one_attention_pair_per_layer():
    layers = 4
    cfg = make_cfg(Q4_K, Q4_0, layers=layers)
    A, Bp = personas(cfg)
    s = pp.Slots("hip", cfg, B)
    assert s.open(0) == 0 and s.open(2) == 0
    assert s.persona([(0, A), (2, Bp)], 0) == 24          # one pass: voice | tokens | voice | tokens
    st = s.stats()
    s.free()
    print(f"{st.kernels_in_last_plan} launches, {st.pass_input_launches_in_last_plan} input launch writing {st.pass_input_rows_in_last_plan} rows, "
          f"{st.attn_block_launches_in_last_plan} attention launches holding {st.attn_block_jobs_in_last_plan} blocks")
    assert st.pass_input_launches_in_last_plan == 1 and st.pass_input_rows_in_last_plan == 24
    assert st.attn_block_launches_in_last_plan == 2 * layers and st.attn_block_jobs_in_last_plan == 2 * layers
    assert st.generic_attention_nodes_in_last_plan == 0


def test_lockstep_streams_match_the_batched_oracle():
    cfg, n = make_cfg(Q4_K, Q4_0), 30                      # 16 Depth steps over a ring of 8: the Depth ring wraps in every frame
    codes = np.random.default_rng(9).integers(0, cfg.card, (n, 2, cfg.io_dep_q)).tolist()
    runs = {}
    for kind in ("oracle", "hip"):
        s = pp.Streams(kind, cfg, 2)
        runs[kind] = [s.step(fr) for fr in codes]
        s.free()
    for k, (a, g) in enumerate(zip(runs["oracle"], runs["hip"])):
        assert a == g, f"frame {k}: oracle {a} vs hip {g}"
    assert sum(r[0] for r in runs["oracle"]) >= n - 2
