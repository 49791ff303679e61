"""GPU: encoder slots (moshi_hot_create_encoder_slots) on the MI355X against the oracle, at Mimi's own size.

Latents: the tolerance is measured, not written down. Every test takes the max-abs deviation of the EXISTING single-stream device encode (flags 16:
plain launches) from the oracle on the same frames, and the B-column latents must stay within 2x that figure (the orders of the split sums differ,
the precision does not). Both figures are printed.

Codes are integers: per stack they must equal the oracle's level by level up to the first parting, and a parting must be explained by the latent
difference (encoder_slots_util.CodeCheck). So that partings cannot hide a failure at least half of the (slot, frame) pairs must be fully exact and
0.8 of all level codes counted exact - the same two caps the single-stream device encode is held to on the same frames, in the same test.

References are computed once and shared. tests/test_encoder_slots_cpu.py asserts that the oracle encoder-slots model equals fresh single-stream
oracle models bit for bit; the staggered and wrap tests compare with the oracle encoder-slots model itself and the wide test (33 columns, of which
31 closed ones would cost the oracle 31 frozen encodes per frame) with two single-stream references."""
import functools

import numpy as np
import pytest

import encoder_slots_util as eu
import hot_util as hu

pytestmark = pytest.mark.gpu
SEED = 3


@functools.lru_cache(maxsize=None)
def oracle_single(seed, fill=0):
    out = eu.single_reference("oracle", eu.cfg_of(), eu.pcm(seed), seed=SEED, fill=fill)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def device_single(seed, fill=0):
    out = eu.single_reference("hip", eu.cfg_of(), eu.pcm(seed), seed=SEED, flags=16, fill=fill)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def books():
    m = hu.Model("oracle", eu.cfg_of(), seed=SEED)
    out = {("first", 0): eu.codebook(m.m, "first", 0)}
    for j in range(eu.N_Q - 1):
        out[("rest", j)] = eu.codebook(m.m, "rest", j)
    m.free()
    return out


def book(stack, level):
    return books()[(stack, level)]


def single_stream(spans):
    """the single-stream device encode (flags 16) against the oracle on spans of (seed, n frames, fill): its max-abs latent deviation, and its codes
    held to the caps the slots are held to"""
    check = eu.CodeCheck(book)
    worst = 0.0
    for seed, n, fill in spans:
        (rc, rf, rr), (dc, df, dr) = oracle_single(seed, fill), device_single(seed, fill)
        for i in range(n):
            worst = max(worst, float(np.abs(df[i] - rf[i]).max()), float(np.abs(dr[i] - rr[i]).max()))
            check.add(f"single-stream {seed} frame {i}", rc[i], dc[i], (rf[i], rr[i]), (df[i], dr[i]))
    check.assert_caps("single-stream device encode")
    return worst


@functools.lru_cache(maxsize=None)
def oracle_schedule(B):
    s = eu.EncoderSlots("oracle", eu.cfg_of(), B, seed=SEED)
    got = eu.run_schedule(s, eu.schedule(late=B - 1))
    s.free()
    return got


@pytest.mark.parametrize("B", [2, 3])
def test_staggered_slots_against_the_oracle_encoder_slots_model(B):
    spans = eu.schedule(late=B - 1)
    ref = oracle_schedule(B)
    s = eu.EncoderSlots("hip", eu.cfg_of(), B, seed=SEED)
    got = eu.run_schedule(s, spans)
    s.free()
    for g, r in zip(got, ref):
        assert g[0] == r[0] and list(g[2]) == list(r[2])
        for b in range(B):
            if b not in g[3]:
                assert np.all(g[1][b] == -1) and g[2][b] == -1
    check = eu.CodeCheck(book)
    dev = 0.0
    for b, first, seq in spans:
        for i in range(len(seq)):
            k = first + i
            lg, lr = [a[b] for a in got[k][4]], [a[b] for a in ref[k][4]]
            dev = max(dev, float(np.abs(lg[0] - lr[0]).max()), float(np.abs(lg[1] - lr[1]).max()))
            check.add(f"slot {b} frame {k}", ref[k][1][b], got[k][1][b], lr, lg)
    single = single_stream([(900, 4, 0), (902, 4, 0), (904, 2, 0)])
    print(f"B = {B}: encoder-slots device latents against the oracle encoder-slots model: max abs deviation {dev:.3e} (single-stream device: {single:.3e})")
    assert dev <= 2 * single, (dev, single)
    check.assert_caps(f"B = {B} encoder slots")


def test_a_conversation_gets_the_same_bits_in_any_column_of_any_batch():
    seq = eu.pcm(910)

    def rows_of(s, slot, frames_of):
        out = []
        for k in range(eu.N_FRAMES):
            r, codes, _ = s.encode(frames_of(k))
            lf, lr = s.latents()
            out.append((codes[slot].copy(), lf[slot].copy(), lr[slot].copy()))
        return out
    a = eu.EncoderSlots("hip", eu.cfg_of(), 2, seed=SEED)
    assert a.open(0) == 0                                            # slot 1 stays closed: a silent neighbour
    got_a = rows_of(a, 0, lambda k: [seq[k], None])
    a.free()
    b = eu.EncoderSlots("hip", eu.cfg_of(), 3, seed=SEED)
    for slot in range(3):
        assert b.open(slot) == 0
    b.set_fill(0, 57)                                                # busy neighbours, at other positions
    others = [eu.pcm(911), eu.pcm(912)]
    got_b = rows_of(b, 2, lambda k: [others[0][k], others[1][k], seq[k]])
    b.free()
    for k, (x, y) in enumerate(zip(got_a, got_b)):
        for u, v, what in zip(x, y, ("codes", "first latent", "rest latent")):
            assert np.array_equal(u, v), (k, what)
    assert len({tuple(x[0]) for x in got_a}) == eu.N_FRAMES, "degenerate input: the codes do not vary"


def test_ring_wrap_in_one_column_while_another_starts():
    def run(kind):
        s = eu.EncoderSlots(kind, eu.cfg_of(), 2, seed=SEED)
        assert s.open(0) == 0 and s.open(1) == 0
        s.set_fill(1, 122)                                           # rows 244, 245: three frames before the 250-row ring wraps
        a, b = eu.pcm(900), eu.pcm(902)
        out = []
        for k in range(eu.N_FRAMES):
            r, codes, status = s.encode([a[k], b[k]])
            assert r == 2 and list(status) == [1, 1]
            out.append((codes, s.latents()))
        assert [s.position(0), s.position(1)] == [eu.N_FRAMES, 122 + eu.N_FRAMES]
        s.free()
        return out
    ref, got = run("oracle"), run("hip")
    check = eu.CodeCheck(book)
    dev = [0.0, 0.0]
    for k in range(eu.N_FRAMES):
        for b in range(2):
            lg, lr = [a[b] for a in got[k][1]], [a[b] for a in ref[k][1]]
            dev[b] = max(dev[b], float(np.abs(lg[0] - lr[0]).max()), float(np.abs(lg[1] - lr[1]).max()))
            check.add(f"slot {b} frame {k}", ref[k][0][b], got[k][0][b], lr, lg)
    single = single_stream([(900, eu.N_FRAMES, 0), (902, eu.N_FRAMES, 122)])
    print(f"ring wrap: slot 0 (from 0) {dev[0]:.3e}, slot 1 (across the wrap) {dev[1]:.3e}; single-stream device {single:.3e}")
    assert max(dev) <= 2 * single, (dev, single)
    check.assert_caps("ring wrap encoder slots")


def test_the_encode_plan_does_not_grow_with_the_batch():
    launches = {}
    for B in (2, 5):
        s = eu.EncoderSlots("hip", eu.cfg_of(), B, seed=SEED)
        for b in range(B):
            assert s.open(b) == 0
        for k in range(2):
            assert s.encode([eu.pcm(920 + b)[k] for b in range(B)])[0] == B
        st = s.stats()
        launches[B] = st.kernels_in_last_plan
        print(f"B = {B}: {st.kernels_in_last_plan} launches in the encode plan, {st.vq_column_levels_in_last_plan} B-column RVQ levels, "
              f"{st.code_gather_columns_in_last_plan} code gather columns, {st.codec_attn_launches_in_last_plan} codec attention launches, "
              f"{st.generic_attention_nodes_in_last_plan} generic attention nodes")
        assert st.vq_column_levels_in_last_plan == s.cfg.mimi_n_q
        assert st.code_gather_columns_in_last_plan == B
        assert st.codec_attn_launches_in_last_plan == 8
        assert st.generic_attention_nodes_in_last_plan == 0
        s.free()
    assert launches[2] == launches[5], launches


def test_wide_batch_of_33_with_the_first_and_the_last_slot_open():
    n = 2
    s = eu.EncoderSlots("hip", eu.cfg_of(wide=True), 33, seed=SEED)
    assert s.open(0) == 0 and s.open(32) == 0
    seqs = {0: (900, eu.pcm(900)), 32: (902, eu.pcm(902))}
    check = eu.CodeCheck(book)
    dev = 0.0
    for k in range(n):
        rows = [None] * 33
        rows[0], rows[32] = seqs[0][1][k], seqs[32][1][k]
        r, codes, status = s.encode(rows)
        assert r == 2 and list(status) == [1] + [-1] * 31 + [1] and np.all(codes[1:32] == -1)
        lf, lr = s.latents()
        for b in (0, 32):
            rc, rf, rr = oracle_single(seqs[b][0])
            dev = max(dev, float(np.abs(lf[b] - rf[k]).max()), float(np.abs(lr[b] - rr[k]).max()))
            check.add(f"slot {b} frame {k}", rc[k], codes[b], (rf[k], rr[k]), (lf[b], lr[b]))
    s.free()
    single = single_stream([(900, n, 0), (902, n, 0)])
    print(f"B = 33: slots 0 and 32 against the oracle: max abs deviation {dev:.3e} (single-stream device: {single:.3e})")
    assert dev <= 2 * single, (dev, single)
    check.assert_caps("B = 33 encoder slots")
