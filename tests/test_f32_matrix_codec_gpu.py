"""GPU: decoder and encoder slots with f32_matrix = 1 (include/moshi_hot.h): the F32 linears of the codec transformers run on the f64-MFMA mat-mul
(k_mm_f32_batched). References, schedules, rules and helpers are those of tests/test_codec_slots_gpu.py and tests/test_encoder_slots_gpu.py
(imported, not changed; their cached oracle runs are shared): the reference is the oracle, the tolerance 2 x the single-stream device decode's /
encode's own max-abs deviation from it on the same inputs. Both figures are printed."""
import numpy as np
import pytest

import codec_slots_util as cu
import encoder_slots_util as eu
import test_codec_slots_gpu as dec
import test_encoder_slots_gpu as enc

pytestmark = pytest.mark.gpu
SEED = dec.SEED
N_LINEARS = 32      # in_proj, out_proj, linear1, linear2 of the 8 layers of the decoder transformer


def on(cfg):
    cfg.f32_matrix = 1
    return cfg


def test_decoder_slots_staggered_against_the_oracle():
    spans, ref = cu.schedule(late=1), dec.oracle_schedule(2)
    s = cu.CodecSlots("hip", on(cu.cfg_of()), 2, seed=SEED)
    got = cu.run_schedule(s, spans)
    n_mms = s.stats().f32_matrix_mms_in_last_plan
    s.free()
    assert all(g[0] == r[0] and list(g[2]) == list(r[2]) for g, r in zip(got, ref))
    single = max(dec.single_stream_deviation(900, 4), dec.single_stream_deviation(902, 4), dec.single_stream_deviation(904, 2))
    dev = dec.span_deviation(got, ref, spans)
    print(f"B = 2, f32_matrix: decoder-slots PCM against the oracle: max abs deviation {dev:.3e} (single-stream device: {single:.3e}); {n_mms} f64-MFMA linears")
    assert n_mms == N_LINEARS and dev <= 2 * single, (n_mms, dev, single)
    s = cu.CodecSlots("hip", cu.cfg_of(), 2, seed=SEED)      # a fresh handle and a model without the field
    assert s.open(0) == 0 and s.decode([cu.codes(900)[0], None])[0] == 1 and s.stats().f32_matrix_mms_in_last_plan == 0
    s.free()


def test_a_conversation_gets_the_same_bits_in_any_column_of_any_batch():
    seq = cu.codes(910)
    a = cu.CodecSlots("hip", on(cu.cfg_of()), 2, seed=SEED)
    assert a.open(0) == 0                                            # slot 1 stays closed: a silent neighbour
    pcm_a = np.stack([a.decode([seq[k], None])[1][0] for k in range(cu.N_FRAMES)])
    a.free()
    b = cu.CodecSlots("hip", on(cu.cfg_of()), 3, seed=SEED)
    assert all(b.open(slot) == 0 for slot in range(3))
    b.set_fill(0, 57)                                                # busy neighbours, at other positions
    others = [cu.codes(911), cu.codes(912)]
    pcm_b = np.stack([b.decode([others[0][k], others[1][k], seq[k]])[1][2] for k in range(cu.N_FRAMES)])
    assert b.stats().f32_matrix_mms_in_last_plan == N_LINEARS
    b.free()
    assert np.array_equal(pcm_a, pcm_b)


def test_encoder_slots_staggered_against_the_oracle():
    spans, ref = eu.schedule(late=1), enc.oracle_schedule(2)
    s = eu.EncoderSlots("hip", on(eu.cfg_of()), 2, seed=SEED)
    got = eu.run_schedule(s, spans)
    n_mms = s.stats().f32_matrix_mms_in_last_plan
    s.free()
    assert all(g[0] == r[0] and list(g[2]) == list(r[2]) for g, r in zip(got, ref))
    check, dev = eu.CodeCheck(enc.book), 0.0
    for b, first, seq in spans:
        for k in range(first, first + len(seq)):
            lg, lr = [a[b] for a in got[k][4]], [a[b] for a in ref[k][4]]
            dev = max(dev, float(np.abs(lg[0] - lr[0]).max()), float(np.abs(lg[1] - lr[1]).max()))
            check.add(f"slot {b} frame {k}", ref[k][1][b], got[k][1][b], lr, lg)
    single = enc.single_stream([(900, 4, 0), (902, 4, 0), (904, 2, 0)])
    print(f"B = 2, f32_matrix: encoder-slots latents against the oracle: max abs deviation {dev:.3e} (single-stream device: {single:.3e}); {n_mms} f64-MFMA linears")
    assert n_mms > 0 and dev <= 2 * single, (n_mms, dev, single)
    check.assert_caps("B = 2 encoder slots, f32_matrix")
