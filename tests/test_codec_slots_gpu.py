"""GPU: decoder slots (moshi_hot_create_codec_slots) on the MI355X against the oracle, at Mimi's own size.

The tolerance is measured, not written down: every test takes the max-abs deviation of the EXISTING single-stream device decode (flags 16: plain
launches, the sums nearest in order) from the oracle on the same code sequences, and the B-column PCM must stay within 2x that figure (the orders
of the split sums differ, the precision does not). Both figures are printed. References are computed once and shared.

The oracle side of a slot is a fresh single-stream oracle model fed the slot's codes: tests/test_codec_slots_cpu.py asserts that the oracle
decoder-slots model equals it bit for bit, so the staggered and wrap tests compare with the oracle decoder-slots model itself and the wide test
(33 columns, of which 31 closed ones would cost the oracle 31 frozen decodes per frame) with the two single-stream references."""
import functools

import numpy as np
import pytest

import codec_slots_util as cu

pytestmark = pytest.mark.gpu
SEED = 3


@functools.lru_cache(maxsize=None)
def oracle_single(seed, n):
    out = cu.single_reference("oracle", cu.cfg_of(), cu.codes(seed)[:n], seed=SEED)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def single_stream_deviation(seed, n):
    """max |single-stream device decode (flags 16) - oracle| over n frames of one code sequence"""
    dev = cu.single_reference("hip", cu.cfg_of(), cu.codes(seed)[:n], seed=SEED, flags=16)
    d = float(np.abs(dev - oracle_single(seed, n)).max())
    print(f"single-stream device decode against the oracle, codes {seed} x {n} frames: max abs deviation {d:.3e}")
    return d


@functools.lru_cache(maxsize=None)
def oracle_schedule(B):
    s = cu.CodecSlots("oracle", cu.cfg_of(), B, seed=SEED)
    got = cu.run_schedule(s, cu.schedule(late=B - 1))
    s.free()
    return got


def span_deviation(got, ref, spans):
    worst = 0.0
    for b, first, seq in spans:
        for i in range(len(seq)):
            worst = max(worst, float(np.abs(got[first + i][1][b] - ref[first + i][1][b]).max()))
    return worst


@pytest.mark.parametrize("B", [2, 3])
def test_staggered_slots_against_the_oracle_decoder_slots_model(B):
    spans = cu.schedule(late=B - 1)
    ref = oracle_schedule(B)
    s = cu.CodecSlots("hip", cu.cfg_of(), B, seed=SEED)
    got = cu.run_schedule(s, spans)
    s.free()
    for g, r in zip(got, ref):
        assert g[0] == r[0] and list(g[2]) == list(r[2])
        for b in range(B):
            if b not in g[3]:
                assert np.all(g[1][b] == 0)
    single = max(single_stream_deviation(900, 4), single_stream_deviation(902, 4), single_stream_deviation(904, 2))
    dev = span_deviation(got, ref, spans)
    print(f"B = {B}: decoder-slots device PCM against the oracle decoder-slots model: max abs deviation {dev:.3e} (single-stream device: {single:.3e})")
    assert dev <= 2 * single, (dev, single)


def test_a_conversation_gets_the_same_bits_in_any_column_of_any_batch():
    seq = cu.codes(910)
    a = cu.CodecSlots("hip", cu.cfg_of(), 2, seed=SEED)
    assert a.open(0) == 0                                            # slot 1 stays closed: a silent neighbour
    pcm_a = np.stack([a.decode([seq[k], None])[1][0] for k in range(cu.N_FRAMES)])
    a.free()
    b = cu.CodecSlots("hip", cu.cfg_of(), 3, seed=SEED)
    for slot in range(3):
        assert b.open(slot) == 0
    b.set_fill(0, 57)                                                # busy neighbours, at other positions
    others = [cu.codes(911), cu.codes(912)]
    pcm_b = np.stack([b.decode([others[0][k], others[1][k], seq[k]])[1][2] for k in range(cu.N_FRAMES)])
    b.free()
    assert np.array_equal(pcm_a, pcm_b)


def test_ring_wrap_in_one_column_while_another_starts():
    def run(kind):
        s = cu.CodecSlots(kind, cu.cfg_of(), 2, seed=SEED)
        assert s.open(0) == 0 and s.open(1) == 0
        s.set_fill(1, 122)                                           # rows 244, 245: three frames before the 250-row ring wraps
        out = [s.decode([cu.codes(900)[k], cu.codes(902)[k]]) for k in range(cu.N_FRAMES)]
        assert [s.position(0), s.position(1)] == [cu.N_FRAMES, 122 + cu.N_FRAMES]
        s.free()
        assert all(r == 2 for r, _, _ in out)
        return np.stack([pcm for _, pcm, _ in out])
    ref, got = run("oracle"), run("hip")
    single = max(single_stream_deviation(900, cu.N_FRAMES), single_stream_deviation(902, cu.N_FRAMES))
    dev = [float(np.abs(got[:, b] - ref[:, b]).max()) for b in range(2)]
    print(f"ring wrap: slot 0 (from 0) {dev[0]:.3e}, slot 1 (across the wrap) {dev[1]:.3e}; single-stream device {single:.3e}")
    assert max(dev) <= 2 * single, (dev, single)


def test_the_decode_plan_does_not_grow_with_the_batch():
    launches = {}
    for B in (2, 5):
        s = cu.CodecSlots("hip", cu.cfg_of(), B, seed=SEED)
        for b in range(B):
            assert s.open(b) == 0
        for k in range(2):
            assert s.decode([cu.codes(920 + b)[k] for b in range(B)])[0] == B
        st = s.stats()
        launches[B] = st.kernels_in_last_plan
        print(f"B = {B}: {st.kernels_in_last_plan} launches in the decode plan, {st.convtr_column_groups_in_last_plan} B-column convtr groups, "
              f"{st.codec_attn_launches_in_last_plan} codec attention launches, {st.generic_attention_nodes_in_last_plan} generic attention nodes")
        assert st.convtr_column_groups_in_last_plan == 4
        assert st.codec_attn_launches_in_last_plan == 8
        assert st.generic_attention_nodes_in_last_plan == 0
        s.free()
    assert launches[2] == launches[5], launches


def test_wide_batch_of_33_with_the_first_and_the_last_slot_open():
    n = 2
    s = cu.CodecSlots("hip", cu.cfg_of(wide=True), 33, seed=SEED)
    assert s.open(0) == 0 and s.open(32) == 0
    seqs = {0: cu.codes(900), 32: cu.codes(902)}
    got = []
    for k in range(n):
        rows = [None] * 33
        rows[0], rows[32] = seqs[0][k], seqs[32][k]
        r, pcm, status = s.decode(rows)
        assert r == 2 and list(status) == [1] + [-1] * 31 + [1] and np.all(pcm[1:32] == 0)
        got.append(pcm)
    s.free()
    single = max(single_stream_deviation(900, n), single_stream_deviation(902, n))
    dev = max(float(np.abs(np.stack([g[0] for g in got]) - oracle_single(900, n)).max()),
              float(np.abs(np.stack([g[32] for g in got]) - oracle_single(902, n)).max()))
    print(f"B = 33: slots 0 and 32 against the oracle: max abs deviation {dev:.3e} (single-stream device: {single:.3e})")
    assert dev <= 2 * single, (dev, single)
