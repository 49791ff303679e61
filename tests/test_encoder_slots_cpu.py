"""CPU: encoder slots (moshi_hot_create_encoder_slots) on the host device with the oracle attached, at Mimi's own size. Every open span of a slot gives,
bit for bit, the codes and both projected latents of a fresh single-stream codec-only model (moshi_hot_create, enable_lm = 0) fed that span's frames
one by one - whatever the other slots do: that covers the carried conv tails, the reset on open, the per-column ring rows, mask rows and RoPE phases,
the residual-VQ search at B columns and the independence of neighbours."""
import ctypes as C
import functools

import numpy as np

import codec_slots_util as du
import encoder_slots_util as eu
import hot_util as hu

L = hu.L
SEED = 3


@functools.lru_cache(maxsize=None)
def full_reference(seed, fill):
    out = eu.single_reference("oracle", eu.cfg_of(), eu.pcm(seed), seed=SEED, fill=fill)
    for a in out:
        a.setflags(write=False)
    return out


def reference(seed, n, fill=0):
    """the first n of N_FRAMES frames through a fresh single-stream model (from transformer position `fill` on) -> (codes, first latents, rest latents).
    Computed once per (seed, fill), shared by the tests and never changed"""
    return tuple(a[:n] for a in full_reference(seed, fill))


def check_schedule(B):
    s = eu.EncoderSlots("oracle", eu.cfg_of(), B, seed=SEED)
    assert L.moshi_hot_n_streams(s.m) == B
    assert [s.position(b) for b in range(B)] == [-1] * B             # all slots start closed
    late = B - 1
    spans = eu.schedule(late)
    got = eu.run_schedule(s, spans)
    refs = {(0, 0): reference(900, 4), (late, 2): reference(902, 4), (0, 4): reference(904, 2)}
    for k, (r, codes, status, open_slots, _) in enumerate(got):
        assert r == len(open_slots), (k, r, open_slots)
        for b in range(B):
            if b in open_slots:
                assert status[b] == 1 and np.all(codes[b] >= 0) and np.all(codes[b] < eu.CARD)
            else:
                assert status[b] == -1 and np.all(codes[b] == -1), (k, b)
    assert all(set(g[3]) <= {0, late} for g in got)                   # the slots between never open
    for b, first, seq in spans:
        rc, rf, rr = refs[(b, first)]
        for i in range(len(seq)):
            _, codes, _, _, (lf, lr) = got[first + i]
            assert np.array_equal(codes[b], rc[i]), (b, first, i)
            assert np.array_equal(lf[b], rf[i]) and np.array_equal(lr[b], rr[i]), (b, first, i)
    assert len({tuple(c) for c in np.concatenate([r[0] for r in refs.values()])}) == 10, "degenerate input: the codes do not vary"
    want = [-1] * B
    want[0], want[late] = 2, 4
    assert [s.position(b) for b in range(B)] == want
    s.free()


def test_staggered_slots_equal_fresh_single_stream_encoders_bit_for_bit_b2():
    check_schedule(2)


def test_staggered_slots_equal_fresh_single_stream_encoders_bit_for_bit_b3():
    check_schedule(3)


def test_ring_wrap_in_one_column_while_another_starts():
    s = eu.EncoderSlots("oracle", eu.cfg_of(), 2, seed=SEED)
    assert s.open(0) == 0 and s.open(1) == 0
    s.set_fill(1, 122)                                               # rows 244, 245: three frames before the 250-row ring wraps
    a, b = eu.pcm(900), eu.pcm(902)
    ref0, ref1 = reference(900, eu.N_FRAMES), reference(902, eu.N_FRAMES, fill=122)   # the single-stream model's position is moved the same way
    for k in range(eu.N_FRAMES):
        r, codes, status = s.encode([a[k], b[k]])
        lf, lr = s.latents()
        assert r == 2 and list(status) == [1, 1]
        for col, ref in ((0, ref0), (1, ref1)):
            assert np.array_equal(codes[col], ref[0][k]), (col, k)
            assert np.array_equal(lf[col], ref[1][k]) and np.array_equal(lr[col], ref[2][k]), (col, k)
    assert [s.position(0), s.position(1)] == [eu.N_FRAMES, 122 + eu.N_FRAMES]
    assert not np.array_equal(ref1[1][:4], reference(902, 4)[1])     # the position matters (RoPE phase, mask row): another latent
    s.free()


def test_nothing_open_does_no_work_and_changes_nothing():
    s = eu.EncoderSlots("oracle", eu.cfg_of(), 2, seed=SEED)
    r, codes, status = s.encode([None, None])
    assert r == 0 and np.all(codes == -1) and list(status) == [-1, -1]
    assert [s.position(b) for b in range(2)] == [-1, -1]
    assert L.moshi_hot_graph(s.m, 2) is None                         # no graph was built: no device work
    for b in (-1, 2):
        assert s.open(b) == -1 and s.close(b) == -1 and s.position(b) == -1
    assert s.open(1) == 0 and s.close(1) == 0
    s.set_fill(1, 9)
    r, codes, status = s.encode([None, None])
    assert r == 0 and np.all(codes == -1) and s.position(1) == -1
    st = np.zeros(2, np.int32)
    x = np.zeros((2, eu.FRAME), np.float32)
    assert L.moshi_hot_mimi_encode_slots(s.m, None, codes.ctypes.data, st.ctypes.data) == -1
    assert L.moshi_hot_mimi_encode_slots(s.m, x.ctypes.data, None, st.ctypes.data) == -1
    assert L.moshi_hot_mimi_encode_slots(s.m, x.ctypes.data, codes.ctypes.data, None) == -1
    s.free()


def test_constructor_refusals():
    be = hu.make_backend("oracle")

    def made(B, **kw):
        cfg = eu.cfg_of(wide=kw.pop("wide", False))
        for k, v in kw.items():
            setattr(cfg, k, v)
        m = L.moshi_hot_create_encoder_slots(be, C.byref(cfg), SEED, B)
        if m:
            L.moshi_hot_free(m)
        return bool(m)

    assert not made(2, enable_lm=1)
    assert not made(2, enable_mimi_encoder=0)
    assert not made(2, enable_mimi_decoder=1)
    assert not made(2, codec_stream=1)
    assert not made(2, mimi_n_q=0)
    assert not made(2, mimi_codebook_size=0)
    assert not made(1)
    assert not made(17)
    assert not made(65, wide=True)
    assert made(2)
    # the decoder-slots constructor keeps refusing an encoder
    assert not L.moshi_hot_create_codec_slots(be, C.byref(eu.cfg_of()), SEED, 2)
    L.ggml_backend_free(be)


def test_other_calls_refuse_on_an_encoder_slots_model_and_the_new_call_on_other_models():
    s = eu.EncoderSlots("oracle", eu.cfg_of(), 2, seed=SEED)
    assert s.open(0) == 0
    before = s.position(0)
    i32 = (C.c_int32 * 64)()
    pcm = np.full(2 * 1920, 5.0, np.float32)
    txt = C.c_int32(-7)
    st = np.zeros(2, np.int32)
    L.moshi_hot_mimi_decode(s.m, i32, pcm.ctypes.data)               # does nothing
    assert np.all(pcm == 5.0)
    L.moshi_hot_mimi_encode(s.m, pcm.ctypes.data, i32)
    assert list(i32) == [0] * 64
    assert L.moshi_hot_mimi_decode_slots(s.m, i32, pcm.ctypes.data, st.ctypes.data) == -1
    assert L.moshi_hot_lm_step(s.m, i32, C.byref(txt), i32) == -1
    assert L.moshi_hot_lm_step_n(s.m, i32, 8, C.byref(txt), i32, None) == -1
    assert L.moshi_hot_lm_step_streams(s.m, i32, C.byref(txt), i32) == -1
    assert L.moshi_hot_lm_step_slots(s.m, i32, C.byref(txt), i32, i32) == -1
    assert L.moshi_hot_sts_frame(s.m, pcm.ctypes.data, C.byref(txt), i32, pcm.ctypes.data) == -1
    assert L.moshi_hot_sts_pipeline_frame(s.m, None, C.byref(txt), i32, pcm.ctypes.data) == -1
    assert L.moshi_hot_slot_open(s.m, 0) == -1 and L.moshi_hot_slot_close(s.m, 0) == -1 and L.moshi_hot_slot_position(s.m, 0) == -1
    assert L.moshi_hot_slot_prefill(s.m, 0, i32, 1, 0) == -1 and L.moshi_hot_slot_fork(s.m, 0, 1) == -1
    assert s.position(0) == before and txt.value == -7 and np.all(pcm == 5.0)
    # the weights are the single-stream model's, under the same names
    one = hu.Model("oracle", eu.cfg_of(), seed=SEED)
    for name in (b"mimi.encoder.model.0.conv.weight", b"mimi.encoder.model.12.conv.bias", b"mimi.encoder_transformer.transformer.layers.7.linear2.weight",
                 b"mimi.downsample.conv.weight", b"mimi.quantizer.rvq_first.input_proj.weight", b"mimi.quantizer.rvq_rest.vq.layers.6._codebook.embedding"):
        a, b = L.moshi_hot_weight(s.m, name), L.moshi_hot_weight(one.m, name)
        assert a and b, name
        a, b = C.cast(a, hu.pkg.TP), C.cast(b, hu.pkg.TP)
        n = L.ggml_nbytes(a)
        assert n == L.ggml_nbytes(b) and n > 0
        ba, bb = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
        L.ggml_backend_tensor_get(a, ba.ctypes.data, 0, n)
        L.ggml_backend_tensor_get(b, bb.ctypes.data, 0, n)
        assert np.array_equal(ba, bb), name
    # the new call on a single-stream codec model ...
    codes = np.full((2, 8), -7, np.int32)
    assert L.moshi_hot_mimi_encode_slots(one.m, pcm.ctypes.data, codes.ctypes.data, st.ctypes.data) == -1
    assert L.moshi_hot_codec_slot_open(one.m, 0) == -1
    assert np.all(codes == -7)
    assert one.mimi_encode(eu.pcm(900)[0]) == reference(900, 4)[0][0].tolist()   # ... and nothing has changed on it
    one.free()
    s.free()
    # ... on a decoder-slots model
    d = du.CodecSlots("oracle", du.cfg_of(), 2, seed=SEED)
    assert d.open(0) == 0
    assert L.moshi_hot_mimi_encode_slots(d.m, pcm.ctypes.data, codes.ctypes.data, st.ctypes.data) == -1
    assert np.all(codes == -7) and d.position(0) == 0
    d.free()
    # ... and on an LM slots model
    cfg = hu.hot.tiny(L)
    cfg.enable_mimi_encoder = cfg.enable_mimi_decoder = 0
    be = hu.make_backend("oracle")
    lm = L.moshi_hot_create_slots(be, C.byref(cfg), SEED, 2)
    assert lm
    assert L.moshi_hot_mimi_encode_slots(lm, pcm.ctypes.data, codes.ctypes.data, st.ctypes.data) == -1
    assert np.all(codes == -7)
    L.moshi_hot_free(lm)
    L.ggml_backend_free(be)
