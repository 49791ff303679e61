"""GPU: decoder slots with f32_matrix = 3 / 2 (include/moshi_hot.h): the four streaming transposed convolutions run as one k_convtr_cols_mfma launch
each. References, schedules, rules and helpers are those of tests/test_codec_slots_gpu.py (imported, not changed; its cached oracle
runs are shared): the reference is the oracle, the tolerance 2 x the single-stream device decode's own max-abs deviation from it on the same codes.
Both figures are printed."""
import numpy as np
import pytest

import codec_slots_util as cu
import test_codec_slots_gpu as dec

pytestmark = pytest.mark.gpu
SEED = dec.SEED


def cfg_of(value):
    cfg = cu.cfg_of()
    cfg.f32_matrix = value
    return cfg


def test_decoder_slots_staggered_against_the_oracle():
    spans, ref = cu.schedule(late=1), dec.oracle_schedule(2)
    s = cu.CodecSlots("hip", cfg_of(3), 2, seed=SEED)
    got = cu.run_schedule(s, spans)
    st = s.stats()
    s.free()
    assert all(g[0] == r[0] and list(g[2]) == list(r[2]) for g, r in zip(got, ref))
    single = max(dec.single_stream_deviation(900, 4), dec.single_stream_deviation(902, 4), dec.single_stream_deviation(904, 2))
    dev = dec.span_deviation(got, ref, spans)
    print(f"B = 2, f32_matrix = 3: decoder-slots PCM against the oracle: max abs deviation {dev:.3e} (single-stream device: {single:.3e})")
    assert (st.convtr_matrix_groups_in_last_plan, st.convtr_column_groups_in_last_plan, st.f32_matrix_mms_in_last_plan, st.kernels_in_last_plan) == (4, 4, 32, 224)
    assert dev <= 2 * single, (dev, single)


def test_a_conversation_gets_the_same_bits_in_any_column_of_any_batch():
    seq = cu.codes(910)
    a = cu.CodecSlots("hip", cfg_of(3), 2, seed=SEED)
    assert a.open(0) == 0                                            # slot 1 stays closed: a silent neighbour
    pcm_a = np.stack([a.decode([seq[k], None])[1][0] for k in range(cu.N_FRAMES)])
    a.free()
    b = cu.CodecSlots("hip", cfg_of(3), 3, seed=SEED)
    assert all(b.open(slot) == 0 for slot in range(3))
    b.set_fill(0, 57)                                                # busy neighbours, at other positions
    others = [cu.codes(911), cu.codes(912)]
    pcm_b = np.stack([b.decode([others[0][k], others[1][k], seq[k]])[1][2] for k in range(cu.N_FRAMES)])
    assert b.stats().convtr_matrix_groups_in_last_plan == 4
    b.free()
    assert np.array_equal(pcm_a, pcm_b)


def test_bit_1_alone_leaves_the_linears_where_they_were():
    s = cu.CodecSlots("hip", cfg_of(2), 2, seed=SEED)
    assert s.open(0) == 0 and s.decode([cu.codes(900)[0], None])[0] == 1
    st = s.stats()
    s.free()
    assert (st.convtr_matrix_groups_in_last_plan, st.f32_matrix_mms_in_last_plan, st.kernels_in_last_plan) == (4, 0, 224)
