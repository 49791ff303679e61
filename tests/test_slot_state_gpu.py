"""-m gpu: slot snapshots (moshi_hot_slot_fork / _save / _load) on the MI355X. The tiny contractive model over a ring of 24. The copies are exact
(blobs compared byte for byte: fork against source, reload against blob, the one-launch plan against the generic nodes, neighbours before and after),
the continuation of a fork matches the slots oracle, an oracle blob continues on the device, and the plan of each call holds one ring-copy launch.

Bars: token ids equal on the contractive model; text logits / transformer_out and Depth logits against the oracle within the per-type bars that
tests/test_slot_prefill_gpu.py quotes from tests/test_hip_frame.py (1e-5 / 1e-4 for F32, 5e-2 / 0.2 for quantised weights); source against fork on
the device that file's device-against-device bar (median relative error < 1e-5 for F32, < 1e-2 for quantised weights)."""
import functools

import numpy as np
import pytest

import hot_util as hu
import slot_state_util as ss
import streams_util as su
from ggml_util import F32, Q4_0, Q4_K, Q8_0

pytestmark = pytest.mark.gpu
L = hu.L

N_BEFORE, N_AFTER = 7, 8
TYPES = [(F32, F32), (Q8_0, Q8_0), (Q4_0, Q4_0), (Q4_K, Q4_0)]
IDS = ["f32", "q8_0", "q4_0", "q4_k"]


def make_cfg(lt=Q4_K, et=Q4_0, layers=2):
    cfg = su.lm_only(hu.hot.tiny(L, linear_type=lt, embed_type=et, layers=layers))   # ring of 24
    cfg.update_scale = 1.0 / 256   # (include/moshi_hot.h) rounding flips stay local instead of compounding over free-running frames
    return cfg


def codes(n, seed=81):
    return ss.live_codes(make_cfg(), n, seed=seed)


# frames before the fork -> live rows n = 1, 13 and 24 (30 frames wrap the 24-slot ring); src < dst and src > dst; B = 2 and column 15 of B = 16
@pytest.mark.parametrize("B,src,dst,frames", [(2, 0, 1, 1), (2, 1, 0, 13), (2, 0, 1, 30), (16, 2, 15, 13), (16, 15, 3, 30), (16, 15, 14, 1)])
def test_fork_and_reload_copy_the_state_exactly(B, src, dst, frames):
    cfg = make_cfg()
    s = ss.Slots("hip", cfg, B)
    assert s.open(src) == 0
    ss.run(s, {src: codes(frames)}, frames)
    assert s.fork(src, dst) == 0
    a, b = s.save(src), s.save(dst)
    s.free()
    assert 0 < a.nbytes - ss.ring_bytes(cfg, frames) < 4096
    assert np.any(a[-ss.ring_bytes(cfg, frames):] != 0)
    assert np.array_equal(a, b), f"fork {src} -> {dst} of {B} after {frames} frames: {int(np.sum(a != b))} bytes differ"
    t = ss.Slots("hip", cfg, 2)
    assert t.load(1, a) == 0 and t.position(1) == frames
    c = t.save(1)
    t.free()
    assert np.array_equal(a, c), f"reload: {int(np.sum(a != c))} bytes differ"


@functools.lru_cache(maxsize=None)
def source_blob(kind, frames, lt=Q4_K, et=Q4_0):
    """slot 1 of a B = 3 model after `frames` frames -> (blob, per frame of the 8 that follow (status, text, audio) of slot 1)"""
    s = ss.Slots(kind, make_cfg(lt, et), 3)
    assert s.open(1) == 0
    fr = codes(frames + N_AFTER)
    ss.run(s, {1: fr}, frames)
    blob = s.save(1)
    after = [(r[1][1], r[2][1], r[3][1]) for r in ss.run(s, {1: fr[frames:]}, N_AFTER)]
    s.free()
    return blob, after


@pytest.mark.parametrize("frames", [13, 30])
def test_one_launch_plan_against_generic_nodes(frames):
    blob = source_blob("hip", frames)[0]
    for flags in (0, 1):                       # 1: no fusion - every cpy of the same graphs runs as the generic strided copy
        s = ss.Slots("hip", make_cfg(), 3, flags=flags)
        assert s.load(0, blob) == 0
        launches = s.stats().ring_copy_launches_in_last_plan
        assert s.fork(0, 2) == 0
        launches += s.stats().ring_copy_launches_in_last_plan
        got = [s.save(0), s.save(2)]
        launches += s.stats().ring_copy_launches_in_last_plan
        s.free()
        assert launches == (0 if flags else 3), (flags, launches)
        for what, g in zip(("load then save", "load, fork, save"), got):
            assert np.array_equal(g, blob), f"flags {flags}, {what}: {int(np.sum(g != blob))} bytes differ"


def test_neighbour_column_is_untouched():
    s = ss.Slots("hip", make_cfg(), 3)
    assert s.open(0) == 0 and s.open(1) == 0
    fr = codes(30)
    ss.run(s, {0: fr, 1: codes(30, seed=82)}, 30)
    before = s.save(1)
    assert s.fork(0, 2) == 0
    after_fork = s.save(1)
    assert s.close(2) == 0 and s.load(2, source_blob("hip", 13)[0]) == 0
    after_load = s.save(1)
    s.free()
    assert np.array_equal(before, after_fork) and np.array_equal(before, after_load)


@functools.lru_cache(maxsize=None)
def fork_scenario(kind, lt, et):
    """slot 0 runs 7 frames and is forked into slot 2; both take the same codes for 8 frames
    -> per frame after the fork (status, texts, audios, text_logits, transformer_out, Depth logits)"""
    cfg = make_cfg(lt, et)
    s = ss.Slots(kind, cfg, 3)
    assert s.open(0) == 0
    fr = codes(N_BEFORE + N_AFTER)
    ss.run(s, {0: fr}, N_BEFORE)
    assert s.fork(0, 2) == 0
    out = []
    for k in range(N_AFTER):
        r = ss.step_all(s, {0: fr[N_BEFORE + k], 2: fr[N_BEFORE + k]})
        out.append(r[1:4] + (r[4], s.read("transformer_out", cfg.dim), s.read(f"dep_logits{cfg.dep_q - 1}", cfg.card)))
    s.free()
    return out


@pytest.mark.parametrize("lt,et", TYPES, ids=IDS)
def test_source_and_fork_continue_like_the_slots_oracle(lt, et):
    ref, got = fork_scenario("oracle", lt, et), fork_scenario("hip", lt, et)
    text_tol, dep_tol = (1e-5, 1e-4) if lt == F32 else (5e-2, 0.2)
    pair, identical = [], True
    for k, (a, g) in enumerate(zip(ref, got)):
        assert a[:3] == g[:3], f"frame {k}: tokens differ: oracle {a[:3]} vs hip {g[:3]}"
        assert g[0][0] == g[0][2] and g[1][0] == g[1][2] and g[2][0] == g[2][2], f"frame {k}: source and fork differ on the device"
        for b in (0, 2):
            e_out, e_txt, e_dep = hu.rel_err(a[4][b], g[4][b]), hu.rel_err(a[3][b], g[3][b]), hu.rel_err(a[5][b], g[5][b])
            print(f"frame {k} slot {b}: transformer_out {e_out:.2e} text logits {e_txt:.2e} Depth logits {e_dep:.2e}")
            assert e_out < text_tol and e_txt < text_tol and e_dep < dep_tol, (k, b, e_out, e_txt, e_dep)
        pair.append(hu.rel_err(g[3][0], g[3][2]))
        identical = identical and np.array_equal(g[3][0], g[3][2]) and np.array_equal(g[5][0], g[5][2])
    print(f"source against fork on the device: text logit errors {np.array2string(np.array(pair), precision=2)}; columns 0 and 2 bit-identical: {identical}")
    assert np.median(pair) < (1e-5 if lt == F32 else 1e-2), f"source against fork: median text logit error {np.median(pair):.2e}"
    assert any(st == [1, -1, 1] for st, *_ in ref)


@pytest.mark.parametrize("frames", [13, 30])
def test_oracle_blob_continues_on_the_device(frames):
    blob, ref = source_blob("oracle", frames)
    t = ss.Slots("hip", make_cfg(), 2)
    assert t.load(0, blob) == 0 and t.position(0) == frames
    got = [(r[1][0], r[2][0], r[3][0]) for r in ss.run(t, {0: codes(frames + N_AFTER)[frames:]}, N_AFTER)]
    t.free()
    assert got == ref, f"tokens after loading the oracle's blob differ: oracle {ref} vs hip {got}"
    assert any(st == 1 for st, _, _ in ref)


def test_each_call_plans_one_ring_copy_launch_for_all_layers():
    layers = 6
    cfg = make_cfg(layers=layers)
    s = ss.Slots("hip", cfg, 3)
    assert s.open(0) == 0
    ss.run(s, {0: codes(5)}, 5)
    plans = {}
    assert s.fork(0, 1) == 0
    plans["fork"] = s.stats()
    blob = s.save(0)
    plans["save"] = s.stats()
    assert s.load(2, blob) == 0
    plans["load"] = s.stats()
    s.free()
    for name, st in plans.items():
        print(f"{name}: {st.kernels_in_last_plan} launches, {st.ring_copy_launches_in_last_plan} ring-copy launches holding {st.ring_copy_jobs_in_last_plan} jobs")
        assert st.ring_copy_launches_in_last_plan == 1 and st.ring_copy_jobs_in_last_plan == 2 * layers, name
        # the only other launch is the row copy of transformer_out: no cpy of a ring view runs as a generic launch
        assert st.kernels_in_last_plan == 2 and st.fused_nodes_in_last_plan == 2 * layers, name
