"""GPU: decoder and encoder slots with bit 2 of f32_matrix (include/moshi_hot.h): every B-column convolution group of the Mimi graphs is one
k_conv_cols_mfma launch. References, schedules, rules and helpers are those of tests/test_codec_slots_gpu.py and
tests/test_encoder_slots_gpu.py (imported, not changed; their cached oracle and single-stream runs are shared): the reference is the oracle, the
tolerance 2 x the single-stream device's own max-abs deviation from it on the same inputs, the encoder's codes under the caps of eu.CodeCheck.

The group counts are the conv_1d_bias calls of moshi_hot.cpp at B columns. build_decode_graph: the output projection of each RVQ stack (2), dec_convs[0]
and dec_convs[1] (2), two per resnet_block x 4 (8) = 12. build_encode_graph: enc_convs[0] and enc_convs[5] (2), per stage two in the resnet_block and
the strided convolution x 4 (12), the downsampler (1), the input projection of each RVQ stack (2) = 17."""
import numpy as np
import pytest

import codec_slot_state_util as su
import codec_slots_util as cu
import encoder_slots_util as eu
import test_codec_slots_gpu as dec
import test_encoder_slots_gpu as enc

pytestmark = pytest.mark.gpu
SEED = dec.SEED
GROUPS = {"decoder": 12, "encoder": 17}


def make(half, value, B):
    cfg = half.cfg()
    cfg.f32_matrix = value
    return (cu.CodecSlots if half.dec else eu.EncoderSlots)("hip", cfg, B, seed=SEED)


@pytest.mark.parametrize("B", [2, 3])
@pytest.mark.parametrize("value", [4, 7])
def test_decoder_slots_staggered_against_the_oracle(value, B):
    spans, ref = cu.schedule(late=B - 1), dec.oracle_schedule(B)
    s = make(su.HALVES[0], value, B)
    got = cu.run_schedule(s, spans)
    n = s.stats().conv_matrix_groups_in_last_plan
    s.free()
    assert all(g[0] == r[0] and list(g[2]) == list(r[2]) for g, r in zip(got, ref))
    single = max(dec.single_stream_deviation(900, 4), dec.single_stream_deviation(902, 4), dec.single_stream_deviation(904, 2))
    dev = dec.span_deviation(got, ref, spans)
    print(f"B = {B}, f32_matrix = {value}: decoder-slots PCM against the oracle: max abs deviation {dev:.3e} (single-stream device: {single:.3e})")
    assert n == GROUPS["decoder"] and dev <= 2 * single, (n, dev, single)


@pytest.mark.parametrize("B", [2, 3])
@pytest.mark.parametrize("value", [4, 7])
def test_encoder_slots_staggered_against_the_oracle(value, B):
    spans, ref = eu.schedule(late=B - 1), enc.oracle_schedule(B)
    s = make(su.HALVES[1], value, B)
    got = eu.run_schedule(s, spans)
    n = s.stats().conv_matrix_groups_in_last_plan
    s.free()
    assert all(g[0] == r[0] and list(g[2]) == list(r[2]) for g, r in zip(got, ref))
    check, dev = eu.CodeCheck(enc.book), 0.0
    for b, first, seq in spans:
        for k in range(first, first + len(seq)):
            lg, lr = [a[b] for a in got[k][4]], [a[b] for a in ref[k][4]]
            dev = max(dev, float(np.abs(lg[0] - lr[0]).max()), float(np.abs(lg[1] - lr[1]).max()))
            check.add(f"slot {b} frame {k}", ref[k][1][b], got[k][1][b], lr, lg)
    single = enc.single_stream([(900, 4, 0), (902, 4, 0), (904, 2, 0)])
    print(f"B = {B}, f32_matrix = {value}: encoder-slots latents against the oracle: max abs deviation {dev:.3e} (single-stream device: {single:.3e})")
    assert n == GROUPS["encoder"] and dev <= 2 * single, (n, dev, single)
    check.assert_caps(f"B = {B} encoder slots, f32_matrix = {value}")


@pytest.mark.parametrize("half", su.HALVES, ids=repr)
def test_a_conversation_gets_the_same_bits_in_any_column_of_any_batch(half):
    seq, others = half.frames(910, 6), [half.frames(911, 6), half.frames(912, 6)]
    a = make(half, 7, 2)
    assert a.open(0) == 0                                            # slot 1 stays closed: a silent neighbour
    got_a = su.run(half, a, 0, seq)
    a.free()
    b = make(half, 7, 3)
    assert all(b.open(slot) == 0 for slot in range(3))
    b.set_fill(0, 57)                                                # busy neighbours, at other positions
    got_b = [half.step(b, {0: others[0][k], 1: others[1][k], 2: seq[k]})[2] for k in range(6)]
    assert b.stats().conv_matrix_groups_in_last_plan == GROUPS[half.name]
    b.free()
    assert all(su.same(x, y) for x, y in zip(got_a, got_b))


@pytest.mark.parametrize("half", su.HALVES, ids=repr)
def test_the_plan_is_shorter_than_without_the_bit_and_does_not_grow_with_the_batch(half):
    launches = {}
    for value, B in ((3, 2), (7, 2), (7, 5)):
        s = make(half, value, B)
        assert all(s.open(b) == 0 for b in range(B))
        for k in range(2):
            half.step(s, {b: half.frames(920 + b, 2)[k] for b in range(B)})
        st = s.stats()
        launches[value, B] = st.kernels_in_last_plan
        assert st.conv_matrix_groups_in_last_plan == (GROUPS[half.name] if value & 4 else 0)
        s.free()
    print(f"{half}: launches in the plan {launches}")
    assert launches[7, 2] == launches[7, 5] < launches[3, 2], launches


@pytest.mark.parametrize("half", su.HALVES, ids=repr)
def test_snapshots_round_trip_with_the_bit_set(half):
    frames = half.frames(930, 5)
    s = make(half, 7, 3)
    su.dirty(half, s, 2)
    assert s.open(0) == 0
    su.run(half, s, 0, frames[:3])
    blob = su.save(s, 0)
    rest = su.run(half, s, 0, frames[3:])
    assert s.close(0) == 0 and su.load(s, 2, blob) == 0 and su.fork(s, 2, 1) == 0
    for k, f in enumerate(frames[3:]):
        got = half.step(s, {1: f, 2: f})
        assert su.same(got[1], rest[k]) and su.same(got[2], rest[k]), k
    s.free()
