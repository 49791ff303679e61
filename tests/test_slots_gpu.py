"""-m gpu: stream slots (moshi_hot_create_slots) on the MI355X - conversations admitted and retired mid-batch, each slot at a stream position of its
own, against the oracle's slots model, against the device lockstep model, against single-stream device models at the moshika width, and the plans
(one attention launch per layer with per-slot mask rows / RoPE rows / ring slots, one launch for the B mask rows).

Bars as tests/test_streams_gpu.py: token ids bit-exact against the oracle (contractive tiny model), logits per weight type in the statistical form
that module uses (median within the bar and below summation noise, 90 % of slot-frames within the bar, every one below 0.1)."""
import ctypes as C

import numpy as np
import pytest

import ggml_util as gu
import hot_util as hu
import slots_util as sl
import streams_util as su
from ggml_util import BF16, F32, Q4_0, Q4_K, Q8_0

pytestmark = pytest.mark.gpu
L = hu.L
libc = C.CDLL(None)

LOGIT_TOL = 1e-2
TYPE_TOL = {BF16: 1e-6, F32: 1e-5, Q8_0: 1e-5, Q4_K: LOGIT_TOL, Q4_0: LOGIT_TOL}
RING = 8


def tiny_slots(lt, et, contractive=True, context=RING):
    cfg = su.lm_only(hu.hot.tiny(L, linear_type=lt, embed_type=et, context=context))
    if contractive:
        cfg.update_scale = 1.0 / 256   # (include/moshi_hot.h) rounding flips stay local instead of compounding over free-running frames
    return cfg


def staggered_events(B):
    """slot b opens at frame b (B - 1 stays closed at B = 8); slot 0 is reopened after its conversation ran past the 8-slot ring's wrap, and slot 1
    (B = 3) / slot 3 (B = 8) is closed before its ring filled and reopened later"""
    ev = {}
    n_open = B if B <= 3 else B - 1
    for b in range(n_open):
        ev.setdefault(b, []).append(("open", b))
    ev.setdefault(RING + 2, []).extend([("close", 0), ("open", 0)])
    short = 1 if B <= 3 else 3
    ev.setdefault(short + 5, []).append(("close", short))
    ev.setdefault(short + 8, []).append(("open", short))
    return ev


def run(kind, cfg, B, codes, events, srand=False, fills=None):
    s = sl.Slots(kind, cfg, B, seed=0)
    for b, f in (fills or {}).items():
        s.open(b)
        s.set_fill(b, f)

    def noise(i):
        if srand:
            libc.srand(1000 + i)   # the sampler's exponential noise is drawn from rand() on the host: both executors see the same draws
    rec = sl.run_slots(s, codes, events, logits=True, dep_logits=True, before_step=noise)
    st = s.stats() if kind == "hip" else None
    s.free()
    return rec, st


@pytest.mark.parametrize("B", [3, 8])
@pytest.mark.parametrize("lt,et", [(Q4_K, Q4_0), (Q8_0, Q8_0), (BF16, BF16), (F32, F32)])
def test_staggered_and_reopened_slots_match_oracle(lt, et, B):
    cfg = tiny_slots(lt, et)
    n = 2 * RING + 2
    codes = sl.slot_codes(cfg, B, n, seed=B)
    events = staggered_events(B)
    ref, _ = run("oracle", cfg, B, codes, events)
    got, _ = run("hip", cfg, B, codes, events)
    errs = []
    for i, (a, b) in enumerate(zip(ref, got)):
        assert a[:4] == b[:4], f"frame {i}: tokens differ: oracle {a[:4]} vs hip {b[:4]}"
        for s in range(B):
            if a[1][s] != -1:
                errs.append(max(hu.rel_err(a[4][s], b[4][s]), hu.rel_err(a[5][s], b[5][s])))
    assert any(r[0] > 0 for r in ref)
    errs = np.array(errs)
    tol = TYPE_TOL[lt]
    assert np.median(errs) < min(tol, 1e-5), f"median logit error {np.median(errs):.2e}"
    assert np.mean(errs < tol) >= 0.9 and errs.max() < 0.1, f"logit errors over the bar {tol:.0e}: {np.sort(errs)[-8:]}"


def test_sampled_slots_match_oracle_with_the_same_noise():
    cfg = tiny_slots(Q4_K, Q4_0)
    cfg.temp, cfg.temp_text, cfg.top_k, cfg.top_k_text = 0.8, 0.7, 20, 25
    n = 2 * RING + 2
    codes = sl.slot_codes(cfg, 3, n, seed=9)
    events = staggered_events(3)
    ref, _ = run("oracle", cfg, 3, codes, events, srand=True)
    got, _ = run("hip", cfg, 3, codes, events, srand=True)
    for i, (a, b) in enumerate(zip(ref, got)):
        assert a[:4] == b[:4], f"frame {i}: sampled tokens differ: oracle {a[:4]} vs hip {b[:4]}"
    assert len({t for r in ref for t in r[2] if t >= 0}) > 1


@pytest.mark.parametrize("B", [3, 8])
def test_all_slots_open_at_frame_zero_equal_device_lockstep(B):
    # the per-slot strides, the per-slot RoPE table and the grouped mask rows change no arithmetic: bit for bit the lockstep model
    cfg = tiny_slots(Q4_K, Q4_0, contractive=False)
    n = RING + 4
    codes = sl.slot_codes(cfg, B, n, seed=30 + B)
    ref = su.run_streams("hip", cfg, codes, logits=True)
    s = sl.Slots("hip", cfg, B)
    got = sl.run_slots(s, codes, {0: [("open", b) for b in range(B)]}, logits=True)
    s.free()
    for k, (g, r) in enumerate(zip(got, ref)):
        assert g[1] == [r[0]] * B, k
        if r[0]:
            assert g[2] == r[1] and g[3] == r[2], k
        assert np.array_equal(g[4], r[3]), k


def test_slots_temporal_plan_has_no_generic_attention():
    cfg = tiny_slots(Q4_K, Q4_0)
    B = 8
    s = sl.Slots("hip", cfg, B)
    codes = sl.slot_codes(cfg, B, 6, seed=2)
    for i, fr in enumerate(codes):   # slots at positions 5, 4, .. 0 and two closed
        if i < B - 2:
            s.open(i)
        s.step(fr)
    assert [s.position(b) for b in range(B)] == [6, 5, 4, 3, 2, 1, -1, -1]
    # the Temporal graph once more on its own (same inputs, same ring slots): its plan is the last one
    assert L.ggml_backend_graph_compute(s.be, L.moshi_hot_graph(s.m, 0)) == 0
    st = s.stats()
    s.free()
    bound = 6 * cfg.num_layers + 8     # as tests/test_streams_gpu.py test_batched_temporal_plan_has_no_generic_attention
    assert st.kernels_in_last_plan <= bound, f"{st.kernels_in_last_plan} launches in the slots Temporal plan (bound {bound})"


@pytest.mark.parametrize("B", [1, 2, 3, 8, 16])
def test_mask_rows_of_the_slots_step_are_one_launch(B):
    # the scratch graph of the slots step (moshi_hot.cpp transformer_graph_step_slots): B windows of the bias table, each at its own column, into
    # the B rows of the mask input - one launch for any B (B = 1: the single-stream step's fold, also one)
    C_ = 24
    width = 3 * C_ - 1
    pattern = np.where(np.arange(width) < 2 * C_, 0.0, -np.inf).astype(np.float32)
    positions = [(7 * b + 3 * (b % 2) * C_) for b in range(B)]
    cols = [2 * C_ - 1 - p if p <= C_ else C_ - p % C_ for p in positions]

    def build(g):
        pat = g.input(pattern)
        dst = g.new(F32, C_, 1, 1, B)
        outs = []
        for b in range(B):
            row = g.cont(g.view_2d(pat, C_, 1, width * 4, cols[b] * 4))
            outs.append(g.cpy(row, g.view_1d(dst, C_, b * C_ * 4)))
        return outs, [dst]
    res, st = gu.run_graph("hip", build)
    want = np.stack([pattern[c:c + C_] for c in cols]).reshape(B, 1, 1, C_)
    assert np.array_equal(res[-1], want)
    assert st.kernels_in_last_plan == 1, f"{st.kernels_in_last_plan} launches for {B} mask rows"


def test_long_and_short_fills_side_by_side_match_oracle():
    # one slot at fill 2 800 of a 3 000-slot ring beside slots at fill 0 .. 3: each (head, slot) workgroup scans its own slot's mask row
    cfg = tiny_slots(Q4_K, Q4_0, context=3000)
    B, n = 4, 8
    codes = sl.slot_codes(cfg, B, n, seed=17)
    events = {0: [("open", 1)], 1: [("open", 2)], 3: [("open", 3)]}
    ref, _ = run("oracle", cfg, B, codes, events, fills={0: 2800})
    got, _ = run("hip", cfg, B, codes, events, fills={0: 2800})
    for i, (a, b) in enumerate(zip(ref, got)):
        assert a[:4] == b[:4], f"frame {i}: tokens differ: oracle {a[:4]} vs hip {b[:4]}"
    assert ref[-1][1][0] == 1 and any(r[0] > 1 for r in ref)


def near_tie(logits, tok_ref, tok_got, err):
    return tok_ref == tok_got or float(logits[tok_ref] - logits[tok_got]) <= 2.0 * err * float(np.abs(logits).max()) + 1e-6


def test_contractive_moshika_width_staggered_slots_equal_single_stream_device_models():
    # every conversation against a single-stream device model fed that conversation's codes from its own first frame, up to the first near-tie pick
    # (the B-column int8-MFMA mat-muls and the single-column mat-vecs sum in different orders: tests/test_streams_gpu.py)
    cfg = su.lm_only(hu.hot.moshika(L))
    cfg.update_scale = 1.0 / 256
    B, n, dq = 3, 12, cfg.dep_q
    QSTEP_TOL = 2e-3
    codes = sl.slot_codes(cfg, B, n, seed=23)
    start = [0, 2, 5]
    s = sl.Slots("hip", cfg, B)
    got = []
    for i, fr in enumerate(codes):
        for b in range(B):
            if start[b] == i:
                s.open(b)
        r = s.step(fr)
        got.append(r + (s.read("text_logits", cfg.text_card), [s.read(f"dep_logits{k}", cfg.card) for k in range(dq)]))
    s.free()
    compared, total, errs = 0, 0, []
    for b in range(B):
        m = hu.Model("hip", cfg, seed=0)
        total += n - start[b]
        for i in range(start[b], n):
            r = m.lm_step(codes[i][b])
            lt = m.read("text_logits", cfg.text_card)
            dl = [m.read(f"dep_logits{k}", cfg.card) for k in range(dq)]
            txt_raw, aud_raw = m.last_raw()
            g = got[i]
            e = hu.rel_err(lt, g[4][b])
            assert e < QSTEP_TOL, f"slot {b} frame {i}: text logits rel err {e:.2e}"
            errs.append(e)
            assert g[1][b] == r[0], (b, i)
            gt = int(np.argmax(g[4][b]))
            assert near_tie(lt, txt_raw, gt, e), f"slot {b} frame {i}: text pick {gt} vs {txt_raw} is not a near-tie"
            diverged = gt != txt_raw
            for k in range(dq):
                if diverged:
                    break
                ek = hu.rel_err(dl[k], g[5][k][b])
                gk = int(np.argmax(g[5][k][b]))
                assert near_tie(dl[k], aud_raw[k], gk, ek), f"slot {b} frame {i} depth {k}: pick {gk} vs {aud_raw[k]} is not a near-tie (err {ek:.2e})"
                diverged = gk != aud_raw[k]
            if diverged:
                break
            compared += 1
            if r[0]:
                assert g[2][b] == r[1] and g[3][b] == r[2], f"slot {b} frame {i}"
        m.free()
    assert compared >= total // 2, f"only {compared} of {total} slot-frames compared before a near-tie divergence"
    # a frame either agrees to summation noise or sits one activation quantiser step away (a Q8_K value rounded the other way): no systematic error
    errs = np.array(errs)
    print("text logit errors:", np.array2string(np.sort(errs), precision=2))
    assert np.median(errs) < QSTEP_TOL and np.mean(errs < 1e-5) >= 0.25, f"text logit errors {np.sort(errs)}"
