"""-m gpu: lockstep streams (moshi_hot_create_streams) on the MI355X - B conversations per frame step against the oracle's batched model, against
single-stream device models at the moshika width, and the plan of the batched Temporal graph (one attention launch per layer for all streams).

Bars: greedy and sampled token ids bit-exact against the oracle (on the contractive variant of the tiny model). Logits: these runs hold B x 12 stream-frames (up to 96) instead of the single-stream frame
test's 8, so a discontinuous activation rounding (a Q8_K / Q8_0 quantiser step, or a BF16 ring store) that the per-type bar of that test excludes on
8 steps turns up on some frame here, moving that frame's logits by ~1e-3 .. 5e-2 (measured: Q4_K 7.6e-2 once, F32 1.0e-3 once - the B-column F32
mat-muls run on the generic float mul_mat, whose summation order is not the mat-vec's). So the per-type bars of tests/test_hip_frame.py are asserted
as that module asserts its long runs: median within the bar and below summation noise, 90 % of stream-frames within the bar, every one below 0.1."""
import ctypes as C

import numpy as np
import pytest

import hot_util as hu
import streams_util as su
from ggml_util import BF16, F32, Q4_0, Q4_K, Q8_0

pytestmark = pytest.mark.gpu
L = hu.L
libc = C.CDLL(None)

# the per-type logit bars of the single-stream frame (tests/test_hip_frame.py TYPE_TOL)
LOGIT_TOL = 1e-2
TYPE_TOL = {BF16: 1e-6, F32: 1e-5, Q8_0: 1e-5, Q4_K: LOGIT_TOL, Q4_0: LOGIT_TOL}


def tiny_streams(lt, et, contractive=False):
    # a Temporal ring of 8 slots: 12 frames run across the wrap (and the Depth ring of dep_q slots wraps every frame)
    cfg = su.lm_only(hu.hot.tiny(L, linear_type=lt, embed_type=et, context=8))
    if contractive:
        cfg.update_scale = 1.0 / 256   # (include/moshi_hot.h) rounding flips stay local instead of compounding over 12 free-running frames
    return cfg


def near_tie(logits, tok_ref, tok_got, err):
    """tok_got is an acceptable greedy pick iff, in the reference logits, it sits within the observed logit disagreement of the reference pick
    (tests/test_hip_frame.py near_tie)"""
    return tok_ref == tok_got or float(logits[tok_ref] - logits[tok_got]) <= 2.0 * err * float(np.abs(logits).max()) + 1e-6


def run(kind, cfg, codes, srand=False):
    s = su.Streams(kind, cfg, len(codes[0]), seed=0)
    rec = []
    for i, fr in enumerate(codes):
        if srand:
            libc.srand(1000 + i)       # the sampler's exponential noise is drawn from rand() on the host: both executors see the same draws
        r, txt, aud = s.step(fr)
        rec.append((r, txt, aud, s.read("text_logits", cfg.text_card), s.read(f"dep_logits{cfg.dep_q - 1}", cfg.card)))
    st = s.stats() if kind == "hip" else None
    s.free()
    return rec, st


@pytest.mark.parametrize("B", [2, 3, 8])
@pytest.mark.parametrize("lt,et", [(Q4_K, Q4_0), (Q8_0, Q8_0), (BF16, BF16), (F32, F32)])
def test_streams_match_oracle_across_the_ring_wrap(lt, et, B):
    cfg = tiny_streams(lt, et, contractive=True)
    codes = su.stream_codes(cfg, B, 12, seed=B)
    ref, _ = run("oracle", cfg, codes)
    got, _ = run("hip", cfg, codes)
    errs = []
    for i, (a, b) in enumerate(zip(ref, got)):
        assert a[:3] == b[:3], f"frame {i}: tokens differ: oracle {a[:3]} vs hip {b[:3]}"
        for s in range(B):
            errs.append(max(hu.rel_err(a[3][s], b[3][s]), hu.rel_err(a[4][s], b[4][s])))
    errs = np.array(errs)
    tol = TYPE_TOL[lt]
    assert np.median(errs) < min(tol, 1e-5), f"median logit error {np.median(errs):.2e}"
    assert np.mean(errs < tol) >= 0.9 and errs.max() < 0.1, f"logit errors over the bar {tol:.0e}: {np.sort(errs)[-8:]}"


def test_sampled_streams_match_oracle_with_the_same_noise():
    cfg = tiny_streams(Q4_K, Q4_0, contractive=True)
    cfg.temp, cfg.temp_text, cfg.top_k, cfg.top_k_text = 0.8, 0.7, 20, 25
    codes = su.stream_codes(cfg, 3, 12, seed=9)
    ref, _ = run("oracle", cfg, codes, srand=True)
    got, _ = run("hip", cfg, codes, srand=True)
    for i, (a, b) in enumerate(zip(ref, got)):
        assert a[:3] == b[:3], f"frame {i}: sampled tokens differ: oracle {a[:3]} vs hip {b[:3]}"
    assert len({t for r in ref[1:] for t in r[1]}) > 1


def test_contractive_moshika_width_streams_equal_single_stream_device_models():
    # Every stream against a single-stream device model fed that stream's codes. The batched int8-MFMA mat-muls and the single-column mat-vecs
    # sum in different orders, so a Q8_K activation value may round the other way (one quantiser step, QSTEP_TOL of the text logits); where that
    # tips a greedy pick it must be a near-tie in the single-stream logits, and that stream's comparison ends there (its later frames are
    # conditioned on the other token). Measured: tokens equal through frame 5 on every stream, one near-tie Depth pick at frame 6.
    cfg = su.lm_only(hu.hot.moshika(L))
    cfg.update_scale = 1.0 / 256                          # contractive stack (include/moshi_hot.h): no chaotic rounding flips at full width
    B, n, dq = 3, 12, cfg.dep_q
    QSTEP_TOL = 2e-3    # one activation quantiser step at this width (tests/test_full_width_parity.py)
    codes = su.stream_codes(cfg, B, n, seed=21)

    st = su.Streams("hip", cfg, B)
    got = []
    for fr in codes:
        r = st.step(fr)
        got.append(r + (st.read("text_logits", cfg.text_card), [st.read(f"dep_logits{k}", cfg.card) for k in range(dq)]))
    st.free()
    compared, errs = 0, []
    for b in range(B):
        m = hu.Model("hip", cfg, seed=0)
        for i, fr in enumerate(codes):
            r = m.lm_step(fr[b])
            lt = m.read("text_logits", cfg.text_card)
            dl = [m.read(f"dep_logits{k}", cfg.card) for k in range(dq)]
            txt_raw, aud_raw = m.last_raw()
            g = got[i]
            e = hu.rel_err(lt, g[3][b])
            assert e < QSTEP_TOL, f"stream {b} frame {i}: text logits rel err {e:.2e}"
            errs.append(e)
            assert g[0] == r[0], (b, i)
            # the raw picks of this frame (before the delay ring) come from the logits just read: text, then the Depth chain
            gt = int(np.argmax(g[3][b]))
            assert near_tie(lt, txt_raw, gt, e), f"stream {b} frame {i}: text pick {gt} vs {txt_raw} is not a near-tie"
            diverged = gt != txt_raw
            for k in range(dq):
                if diverged:
                    break
                ek = hu.rel_err(dl[k], g[4][k][b])
                gk = int(np.argmax(g[4][k][b]))
                assert near_tie(dl[k], aud_raw[k], gk, ek), f"stream {b} frame {i} depth {k}: pick {gk} vs {aud_raw[k]} is not a near-tie (err {ek:.2e})"
                diverged = gk != aud_raw[k]
            if diverged:
                break
            compared += 1
            if r[0]:
                assert g[1][b] == r[1] and g[2][b] == r[2], f"stream {b} frame {i}"
        m.free()
    assert compared >= B * n // 2, f"only {compared} of {B * n} stream-frames compared before a near-tie divergence"
    assert np.median(errs) < 1e-3, f"median text logit error {np.median(errs):.2e}"


def test_batched_temporal_plan_has_no_generic_attention():
    cfg = tiny_streams(Q4_K, Q4_0)
    s = su.Streams("hip", cfg, 8)
    s.step(su.stream_codes(cfg, 8, 1)[0])
    # the Temporal graph once more on its own (same inputs, same ring slot): its plan is the last one
    assert L.ggml_backend_graph_compute(s.be, L.moshi_hot_graph(s.m, 0)) == 0
    st = s.stats()
    s.free()
    # per layer: in_proj, attention, out_proj, linear_in, linear_out (+ one spare); 8 for the embedding sum, the RoPE row and the text head
    bound = 6 * cfg.num_layers + 8
    assert st.kernels_in_last_plan <= bound, f"{st.kernels_in_last_plan} launches in the batched Temporal plan (bound {bound})"


def test_one_stream_on_the_device_is_the_single_stream_model():
    cfg = tiny_streams(Q4_K, Q4_0)
    codes = su.stream_codes(cfg, 1, 10, seed=4)
    got = su.run_streams("hip", cfg, codes, logits=True)
    ref = su.run_single("hip", cfg, [fr[0] for fr in codes], logits=True)
    for g, r in zip(got, ref):
        assert g[0] == r[0] and (not r[0] or (g[1][0] == r[1] and g[2][0] == r[2]))
        assert np.array_equal(g[3][0], r[3])
