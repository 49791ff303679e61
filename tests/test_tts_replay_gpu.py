"""-m gpu: replay and full snapshots of tts-shaped slots on the MI355X.

Op level: the cross-attention jobs of one layer of a replay pass - q [D * H, T], K / V [D, Tc, H, B], jobs of (column, first row, rows), each the node
sequence of cross_attention_jobs ending in a copy into its rows of one [D, H, T] tensor - as ONE k_cross_attn_blocks launch (two for 17 jobs). Every
row is bit-equal to the existing single-column launch on that row (it is the same device function) and within the F32 bar of tests/test_slots_gpu.py
of the oracle; with MI355X_NO_CROSS_ATTN_FUSION (a fresh process: the switch is read once) the plain nodes meet the same bar.

Model level (contractive tiny_tts, 2 layers, as tests/test_tts_slots_gpu.py): B = 3, slot 0 live, slots 1 and 2 replayed with 13 and 6 frames at chunk
8, then 8 live frames. Bars as tests/test_slot_prefill_gpu.py: tokens equal the oracle's, transformer_out / text logits and Depth logits within
1e-5 / 1e-4 (F32) or 5e-2 / 0.2 (quantised weights); device against device that file's median bar (1e-5 / 1e-2)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import ggml_util as gu
import hot_util as hu
import tts_replay_util as ru
import tts_slots_util as tu
from ggml_util import F32, Q4_0, Q4_K, Q8_0
from test_slots_gpu import TYPE_TOL
from test_tts_slots_gpu import run_xattn, xattn_inputs

pytestmark = pytest.mark.gpu
L = hu.L
TOL = TYPE_TOL[F32]
KEEP = tu.KEEP
U64 = 1 << 64

# D, Tc, H (B = 3 columns): the shapes of tests/test_tts_slots_gpu.py
SHAPES = [(128, 5, 4), (128, 1, 4), (64, 17, 4), (256, 7, 2), (128, 64, 16)]
JOBS3 = [(2, 0, 1), (0, 1, 4), (1, 5, 5)]                 # (column, first row, rows): a non-identity column order; 1, 4 and a ragged 5 rows
JOBS17 = [(i % 3, i, 1) for i in range(17)]               # one more job than a launch's table holds
JOBS13 = [(1, 0, 13)]


def block_inputs(D, Tc, H, jobs, big_column=None):
    B = 3
    K, V, _ = xattn_inputs(D, Tc, H, B, big_column)
    T = sum(n for _, _, n in jobs)
    q = np.random.default_rng(D + 7 * Tc + T).standard_normal((T, D * H)).astype(np.float32)
    return K, V, q


def run_blocks(kind, K, V, q, jobs):
    """-> (x [T, D * H], stats or None): the node sequence of cross_attention_jobs (moshi_hot.cpp) up to the [D * H, T] view that cross_out takes"""
    H, Tc, D = K.shape[1], K.shape[2], K.shape[3]
    T = q.shape[0]
    g = gu.Graph(kind)
    try:
        ctx = g.ctx
        Kt, Vt, qt = g.input(K), g.input(V), g.input(q)
        row = D * H * 4
        out = g.new(F32, D, H, T)
        out_at = 0
        for col, r0, n in jobs:
            qj = L.ggml_permute(ctx, L.ggml_view_3d(ctx, qt, D, H, n, D * 4, row, r0 * row), 0, 2, 1, 3)
            kc, vc = Kt.contents, Vt.contents
            k = L.ggml_view_3d(ctx, Kt, D, Tc, H, kc.nb[1], kc.nb[2], col * kc.nb[3])
            v = L.ggml_view_3d(ctx, Vt, D, Tc, H, vc.nb[1], vc.nb[2], col * vc.nb[3])
            w = L.ggml_soft_max_ext(ctx, L.ggml_mul_mat(ctx, k, qj), None, 1.0 / np.sqrt(D), 0.0)
            o = L.ggml_mul_mat(ctx, L.ggml_cont(ctx, L.ggml_transpose(ctx, v)), w)
            dst = L.ggml_view_3d(ctx, out, D, H, n, D * 4, row, ((r0 - out_at) * row) % U64)
            out = L.ggml_cpy(ctx, L.ggml_permute(ctx, o, 0, 2, 1, 3), dst)
            out_at = r0
        x = L.ggml_view_3d(ctx, out, D * H, T, 1, row, row * T, (-out_at * row) % U64)
        g.build([x])
        g.alloc()
        g.compute()
        return g.get(x).reshape(T, D * H), (g.stats() if kind == "hip" else None)
    finally:
        g.free()


def check_blocks(D, Tc, H, jobs, launches, big_column=None):
    K, V, q = block_inputs(D, Tc, H, jobs, big_column)
    ref, _ = run_blocks("oracle", K, V, q, jobs)
    got, st = run_blocks("hip", K, V, q, jobs)
    assert st.cross_block_launches_in_last_plan == launches and st.cross_block_jobs_in_last_plan == len(jobs), (st.cross_block_launches_in_last_plan, st.cross_block_jobs_in_last_plan)
    assert st.kernels_in_last_plan == launches and st.generic_attention_nodes_in_last_plan == 0, st.kernels_in_last_plan
    worst = 0.0
    for col, r0, n in jobs:
        for t in range(r0, r0 + n):
            one, n1 = run_xattn("hip", K[col:col + 1], V[col:col + 1], q[t].reshape(1, 1, D * H))
            assert n1 == 1
            assert np.array_equal(one.reshape(-1), got[t]), f"row {t} (column {col}) differs from the single-column launch on that row"
            err = hu.rel_err(ref[t], got[t])
            worst = max(worst, err)
            assert np.all(np.isfinite(got[t])) and err < TOL, (t, col, err)
    print(f"cross-attention blocks D {D} Tc {Tc} H {H} jobs {len(jobs)}: worst rel err {worst:.2e}")


@pytest.mark.parametrize("D,Tc,H", SHAPES)
def test_cross_attention_jobs_are_one_launch_bit_equal_to_single_column_launches(D, Tc, H):
    check_blocks(D, Tc, H, JOBS3, 1)


def test_seventeen_jobs_take_a_second_launch():
    check_blocks(128, 5, 4, JOBS17, 2)


def test_one_job_of_thirteen_rows():
    check_blocks(128, 5, 4, JOBS13, 1)


@pytest.mark.parametrize("D,Tc,H,big", [(128, 5, 4, 1), (64, 17, 4, 2)])
def test_cross_attention_jobs_with_one_large_column(D, Tc, H, big):
    check_blocks(D, Tc, H, JOBS3, 1, big_column=big)


PLAIN_CHILD = r'''
import numpy as np
import hot_util as hu
import test_tts_replay_gpu as t
for (D, Tc, H), jobs in [(s, t.JOBS3) for s in t.SHAPES] + [((128, 5, 4), t.JOBS17), ((128, 5, 4), t.JOBS13)]:
    K, V, q = t.block_inputs(D, Tc, H, jobs)
    ref, _ = t.run_blocks("oracle", K, V, q, jobs)
    got, st = t.run_blocks("hip", K, V, q, jobs)
    assert st.cross_block_launches_in_last_plan == 0 and st.kernels_in_last_plan > len(jobs), st.kernels_in_last_plan
    for r in range(q.shape[0]):
        err = hu.rel_err(ref[r], got[r])
        assert np.all(np.isfinite(got[r])) and err < t.TOL, (D, Tc, H, r, err)
print("OK")
'''


def test_plain_nodes_meet_the_bar_with_the_fusion_switched_off():
    env = dict(os.environ, PYTHONPATH=os.path.dirname(os.path.abspath(__file__)), MI355X_NO_CROSS_ATTN_FUSION="1")
    r = subprocess.run([sys.executable, "-c", PLAIN_CHILD], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and "OK" in r.stdout, (r.stdout + r.stderr)[-2000:]


# ---- model level --------------------------------------------------------------------------------------------------------------------------------
B, N_BEFORE, N_LIVE = 3, 2, 8
HIST = {1: 13, 2: 6}
TYPES = [(F32, F32), (Q8_0, Q8_0), (Q4_K, Q4_0)]
IDS = ["f32", "q8_0", "q4_k"]


def make_cfg(lt, et, layers=2, ring=24):
    cfg = tu.tts_cfg(linear_type=lt, embed_type=et, layers=layers, cross_len=5)
    cfg.context = ring
    cfg.update_scale = 1.0 / 256   # (include/moshi_hot.h) rounding flips stay local instead of compounding over free-running frames
    return cfg


def hist(cfg, b):
    return ru.history(cfg, HIST[b], seed=60 + b)


@functools.lru_cache(maxsize=None)
def scenario(kind, lt, et, mode="together", flags=0, ring=24):
    """slot b: conditions 4 + b, text stream b. mode: "together" (one call, both jobs), "apart" (one call per job), "none" (slots 1 and 2 stay closed)
    -> {"after": transformer_out [B, dim] right after the replay, "frames": per frame (status, texts, audios, text_logits, transformer_out, Depth logits)}"""
    cfg = make_cfg(lt, et, ring=ring)
    s = ru.Slots(kind, cfg, B, flags=flags)
    for b in range(B):
        assert s.set_conditions(b, 4 + b) == 0
    texts = [tu.text_stream(cfg, b, N_BEFORE + N_LIVE) for b in range(B)]
    assert s.open(0) == 0
    out = {"frames": []}
    for k in range(N_BEFORE + N_LIVE):
        if k == N_BEFORE and mode != "none":
            assert s.open(1) == 0 and s.open(2) == 0
            if mode == "together":
                assert s.replay([(1, hist(cfg, 1)), (2, hist(cfg, 2))], 8) == HIST[1] + HIST[2]
            else:
                assert s.replay_one(1, hist(cfg, 1), 8) == HIST[1] and s.replay_one(2, hist(cfg, 2), 8) == HIST[2]
            assert [s.position(b) for b in range(B)] == [N_BEFORE, HIST[1], HIST[2]]
            out["after"] = s.read("transformer_out", cfg.dim)
        live = k >= N_BEFORE and mode != "none"
        r = s.step([texts[0][k]] + [texts[b][k - N_BEFORE] if live else KEEP for b in (1, 2)])
        out["frames"].append(r[1:] + (s.read("text_logits", cfg.text_card), s.read("transformer_out", cfg.dim),
                                      s.read(f"dep_logits{cfg.dep_q - 1}", cfg.card) if k >= cfg.delay_steps else None))
    s.free()
    return out


def live_slots(k, mode="together"):
    return range(B) if k >= N_BEFORE and mode != "none" else range(1)


def against_the_oracle(lt, ref, got, what):
    text_tol, dep_tol = (1e-5, 1e-4) if lt == F32 else (5e-2, 0.2)
    for b in (1, 2):
        e = hu.rel_err(ref["after"][b], got["after"][b])
        print(f"{what} slot {b}: transformer_out after the replay: rel err {e:.2e}")
        assert e < text_tol, f"{what} slot {b}: transformer_out after the replay: rel err {e:.2e}"
    for k, (a, g) in enumerate(zip(ref["frames"], got["frames"])):
        assert a[:3] == g[:3], f"{what} frame {k}: status or tokens differ: oracle {a[:3]} vs hip {g[:3]}"
        for b in live_slots(k):
            e_out, e_txt = hu.rel_err(a[4][b], g[4][b]), hu.rel_err(a[3][b], g[3][b])
            e_dep = hu.rel_err(a[5][b], g[5][b]) if a[5] is not None else 0.0
            print(f"{what} frame {k} slot {b}: transformer_out {e_out:.2e} text logits {e_txt:.2e} Depth logits {e_dep:.2e}")
            assert e_out < text_tol and e_txt < text_tol and e_dep < dep_tol, (k, b, e_out, e_txt, e_dep)
    assert any(st == [1, 1, 1] for st, *_ in ref["frames"])


@pytest.mark.parametrize("lt,et", TYPES, ids=IDS)
def test_replayed_slots_beside_a_live_one_match_the_slots_oracle(lt, et):
    against_the_oracle(lt, scenario("oracle", lt, et), scenario("hip", lt, et), "ring 24")


def test_replay_across_the_rings_end_matches_the_slots_oracle():
    # a ring of 8: slot 1's 13 frames are a block piece of 8 rows and a ring-ordered piece of 5, slot 0 wraps while it lives
    against_the_oracle(F32, scenario("oracle", F32, F32, ring=8), scenario("hip", F32, F32, ring=8), "ring 8")


def test_live_neighbour_is_bit_identical_with_and_without_the_replay():
    a, b = scenario("hip", Q4_K, Q4_0, "none"), scenario("hip", Q4_K, Q4_0)
    for k, (x, y) in enumerate(zip(a["frames"], b["frames"])):
        assert x[0][0] == y[0][0] and x[1][0] == y[1][0] and x[2][0] == y[2][0], f"frame {k}: slot 0's tokens differ"
        assert np.array_equal(x[3][0], y[3][0]) and np.array_equal(x[4][0], y[4][0]), f"frame {k}: slot 0's text logits or transformer_out differ"
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
    device_pair_agrees(lt, scenario("hip", lt, et, "together", 1), scenario("hip", lt, et), "generic vs fused")


def test_a_pass_has_one_cross_attention_launch_per_layer():
    layers = 6
    cfg = make_cfg(Q4_K, Q4_0, layers=layers)
    for name, jobs in (("one job", [(1, 8)]), ("two jobs", [(1, 5), (2, 3)]), ("three small jobs", [(0, 1), (1, 4), (2, 2)])):
        s = ru.Slots("hip", cfg, B)
        for b, _ in jobs:
            assert s.set_conditions(b, 4 + b) == 0 and s.open(b) == 0
        n = sum(t for _, t in jobs)
        assert s.replay([(b, ru.history(cfg, t, seed=b)) for b, t in jobs], 8) == n     # one pass
        st = s.stats()
        s.free()
        print(f"{name}: {st.kernels_in_last_plan} launches, {st.cross_block_launches_in_last_plan} cross-attention launches holding "
              f"{st.cross_block_jobs_in_last_plan} jobs, {st.attn_block_launches_in_last_plan} attention launches holding {st.attn_block_jobs_in_last_plan} blocks, "
              f"{st.generic_attention_nodes_in_last_plan} generic soft_max / set_rows")
        assert st.cross_block_launches_in_last_plan == layers and st.cross_block_jobs_in_last_plan == len(jobs) * layers, name
        assert st.attn_block_launches_in_last_plan == 2 * layers and st.attn_block_jobs_in_last_plan == len(jobs) * layers, name
        assert st.generic_attention_nodes_in_last_plan == 0, name


# ---- snapshots ----------------------------------------------------------------------------------------------------------------------------------
N_SNAP, N_AFTER = 7, 8


def continued(s, cfg, cols, first, n):
    """the listed columns run frames first .. first + n of text stream 0 -> per frame (status, texts, audios, text logits, transformer_out) of those columns"""
    texts = tu.text_stream(cfg, 0, first + n)
    out = []
    for i in range(first, first + n):
        r = s.step([texts[i] if b in cols else KEEP for b in range(s.B)])
        tl, to = s.read("text_logits", cfg.text_card), s.read("transformer_out", cfg.dim)
        out.append([(r[1][b], r[2][b], r[3][b], tl[b].copy(), to[b].copy()) for b in cols])
    return out


def same_conversation(frames, what):
    """every listed column of every frame equals the first one bit for bit"""
    worst = 0.0
    for k, cols in enumerate(frames):
        for c in cols[1:]:
            worst = max(worst, hu.rel_err(cols[0][3], c[3]))
    print(f"{what}: largest text logit difference between the copies {worst:.2e}")
    for k, cols in enumerate(frames):
        for c in cols[1:]:
            assert c[:3] == cols[0][:3], f"{what} frame {k}: status or tokens differ: {c[:3]} vs {cols[0][:3]}"
            assert np.array_equal(c[3], cols[0][3]) and np.array_equal(c[4], cols[0][4]), f"{what} frame {k}: text logits or transformer_out differ"
    assert any(cols[0][0] == 1 for cols in frames)


@pytest.mark.parametrize("lt,et", [(F32, F32), (Q4_K, Q4_0)], ids=["f32", "q4_k"])
def test_fork_full_and_save_load_full_continue_like_their_source(lt, et):
    cfg = make_cfg(lt, et)
    s = ru.Slots("hip", cfg, 3)
    assert s.set_conditions(0, 4) == 0 and s.set_conditions(2, 9) == 0 and s.open(0) == 0
    continued(s, cfg, [0], 0, N_SNAP)
    blob = s.save_full(0)
    assert s.fork_full(0, 2) == 0 and s.position(2) == N_SNAP
    st = s.stats()
    assert st.ring_copy_launches_in_last_plan == 2 and st.ring_copy_jobs_in_last_plan == 8, (st.ring_copy_launches_in_last_plan, st.ring_copy_jobs_in_last_plan)
    again = s.save_full(2)
    assert np.array_equal(blob, again), f"the fork's blob differs from its source's in {int(np.sum(blob != again))} bytes"
    forked = continued(s, cfg, [0, 2], N_SNAP, N_AFTER)
    s.free()
    same_conversation(forked, "source against fork")
    t = ru.Slots("hip", cfg, 3)
    assert t.set_conditions(0, 11) == 0 and t.load_full(0, blob) == 0 and t.position(0) == N_SNAP
    assert np.array_equal(t.save_full(0), blob)
    loaded = continued(t, cfg, [0], N_SNAP, N_AFTER)
    t.free()
    same_conversation([[a[0], b[0]] for a, b in zip(forked, loaded)], "source against a reloaded blob")


def test_oracle_blob_continues_on_the_device():
    cfg = make_cfg(Q4_K, Q4_0)
    o = ru.Slots("oracle", cfg, 2)
    assert o.set_conditions(1, 4) == 0 and o.open(1) == 0
    continued(o, cfg, [1], 0, N_SNAP)
    blob = o.save_full(1)
    ref = [f[0][:3] for f in continued(o, cfg, [1], N_SNAP, N_AFTER)]
    o.free()
    t = ru.Slots("hip", cfg, 3)
    assert t.load_full(2, blob) == 0 and t.position(2) == N_SNAP
    got = [f[0][:3] for f in continued(t, cfg, [2], N_SNAP, N_AFTER)]
    t.free()
    assert got == ref, f"tokens after loading the oracle's blob differ: oracle {ref} vs hip {got}"
    assert any(st == 1 for st, _, _ in ref)
