"""CPU: decoder slots (moshi_hot_create_codec_slots) on the host device with the oracle attached, at Mimi's own size. Every open span of a slot is,
bit for bit, the PCM of a fresh single-stream codec-only model (moshi_hot_create, enable_lm = 0) fed that span's codes frame by frame - whatever the
other slots do: that covers the carried conv tails and transposed-conv partials, the reset on open, the per-column ring rows, mask rows and RoPE
phases, and the independence of neighbours."""
import ctypes as C
import functools

import numpy as np

import codec_slots_util as cu
import hot_util as hu

L = hu.L


@functools.lru_cache(maxsize=None)
def reference(seed, n):
    """a code sequence through a fresh single-stream model. Shared by the tests and never changed"""
    out = cu.single_reference("oracle", cu.cfg_of(), cu.codes(seed)[:n], seed=3)
    out.setflags(write=False)
    return out


def test_staggered_slots_equal_fresh_single_stream_decoders_bit_for_bit():
    s = cu.CodecSlots("oracle", cu.cfg_of(), 3, seed=3)
    assert L.moshi_hot_n_streams(s.m) == 3
    assert [s.position(b) for b in range(3)] == [-1, -1, -1]          # all slots start closed
    spans = cu.schedule(late=2)
    got = cu.run_schedule(s, spans)
    refs = {(0, 0): reference(900, 4), (2, 2): reference(902, 4), (0, 4): reference(904, 2)}
    for k, (r, pcm, status, open_slots) in enumerate(got):
        assert r == len(open_slots), (k, r, open_slots)
        for b in range(3):
            if b in open_slots:
                assert status[b] == 1
            else:
                assert status[b] == -1 and np.all(pcm[b] == 0), (k, b)
    assert all(1 not in g[3] for g in got)                            # slot 1 never opens
    for b, first, seq in spans:
        for i in range(len(seq)):
            assert np.array_equal(got[first + i][1][b], refs[(b, first)][i]), (b, first, i)
    assert [s.position(b) for b in range(3)] == [2, -1, 4]
    s.free()


def test_constructor_refusals():
    be = hu.make_backend("oracle")

    def made(B, **kw):
        cfg = cu.cfg_of(wide=kw.pop("wide", False))
        for k, v in kw.items():
            setattr(cfg, k, v)
        m = L.moshi_hot_create_codec_slots(be, C.byref(cfg), 3, B)
        if m:
            L.moshi_hot_free(m)
        return bool(m)

    assert not made(2, enable_lm=1)
    assert not made(2, enable_mimi_encoder=1)
    assert not made(2, codec_stream=1)
    assert not made(2, enable_mimi_decoder=0)
    assert not made(1)
    assert not made(17)
    assert not made(65, wide=True)
    assert made(2)
    L.ggml_backend_free(be)


def test_bad_indices_and_bad_codes_change_nothing():
    s = cu.CodecSlots("oracle", cu.cfg_of(), 2, seed=3)
    for b in (-1, 2):
        assert s.open(b) == -1 and s.close(b) == -1 and s.position(b) == -1
    r, pcm, status = s.decode([None, None])                          # nothing open: no device work
    assert r == 0 and np.all(pcm == 0) and list(status) == [-1, -1]
    assert s.open(1) == 0
    seq = cu.codes(900)
    ref = reference(900, 4)
    assert np.array_equal(s.decode([None, seq[0]])[1][1], ref[0])
    for bad in (-1, 2048):
        row = seq[1].copy()
        row[5] = bad
        r, pcm, status = s.decode([None, row])
        assert r == -1 and s.position(1) == 1
    r, pcm, status = s.decode([[-5] * 8, seq[1]])                     # a closed slot's codes are ignored
    assert r == 1 and np.array_equal(pcm[1], ref[1]) and np.all(pcm[0] == 0)
    assert np.array_equal(s.decode([None, seq[2]])[1][1], ref[2])
    s.free()


def test_other_calls_refuse_on_a_decoder_slots_model_and_the_new_calls_on_other_models():
    s = cu.CodecSlots("oracle", cu.cfg_of(), 2, seed=3)
    assert s.open(0) == 0
    before = s.position(0)
    i32 = (C.c_int32 * 64)()
    pcm = np.full(1920, 5.0, np.float32)
    txt = C.c_int32(-7)
    L.moshi_hot_mimi_decode(s.m, i32, pcm.ctypes.data)               # does nothing
    assert np.all(pcm == 5.0)
    L.moshi_hot_mimi_encode(s.m, pcm.ctypes.data, i32)
    assert list(i32) == [0] * 64
    assert L.moshi_hot_lm_step(s.m, i32, C.byref(txt), i32) == -1
    assert L.moshi_hot_lm_step_n(s.m, i32, 8, C.byref(txt), i32, None) == -1
    assert L.moshi_hot_lm_step_streams(s.m, i32, C.byref(txt), i32) == -1
    assert L.moshi_hot_lm_step_slots(s.m, i32, C.byref(txt), i32, i32) == -1
    assert L.moshi_hot_sts_frame(s.m, pcm.ctypes.data, C.byref(txt), i32, pcm.ctypes.data) == -1
    assert L.moshi_hot_sts_pipeline_frame(s.m, None, C.byref(txt), i32, pcm.ctypes.data) == -1
    assert L.moshi_hot_slot_open(s.m, 0) == -1 and L.moshi_hot_slot_close(s.m, 0) == -1 and L.moshi_hot_slot_position(s.m, 0) == -1
    assert L.moshi_hot_slot_prefill(s.m, 0, i32, 1, 0) == -1 and L.moshi_hot_slot_fork(s.m, 0, 1) == -1
    assert s.position(0) == before and txt.value == -7
    # the weights are the single-stream model's, under the same names
    one = hu.Model("oracle", cu.cfg_of(), seed=3)
    for name in (b"mimi.decoder.model.2.convtr.weight", b"mimi.decoder_transformer.transformer.layers.7.linear2.weight", b"mimi.quantizer.rvq_rest.vq.layers.6._codebook.embedding"):
        a, b = L.moshi_hot_weight(s.m, name), L.moshi_hot_weight(one.m, name)
        assert a and b
        a, b = C.cast(a, hu.pkg.TP), C.cast(b, hu.pkg.TP)
        n = L.ggml_nbytes(a)
        assert n == L.ggml_nbytes(b) and n > 0
        ba, bb = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
        L.ggml_backend_tensor_get(a, ba.ctypes.data, 0, n)
        L.ggml_backend_tensor_get(b, bb.ctypes.data, 0, n)
        assert np.array_equal(ba, bb), name
    # the new calls on a single-stream codec model
    st = np.zeros(2, np.int32)
    assert L.moshi_hot_codec_slot_open(one.m, 0) == -1 and L.moshi_hot_codec_slot_close(one.m, 0) == -1 and L.moshi_hot_codec_slot_position(one.m, 0) == -1
    assert L.moshi_hot_mimi_decode_slots(one.m, i32, pcm.ctypes.data, st.ctypes.data) == -1
    assert np.array_equal(one.mimi_decode(cu.codes(900)[0].tolist()), reference(900, 4)[0])   # ... and nothing has changed on it
    one.free()
    s.free()
    # ... and on an LM slots model
    cfg = hu.hot.tiny(L)
    cfg.enable_mimi_encoder = cfg.enable_mimi_decoder = 0
    be = hu.make_backend("oracle")
    lm = L.moshi_hot_create_slots(be, C.byref(cfg), 3, 2)
    assert lm
    assert L.moshi_hot_codec_slot_open(lm, 0) == -1 and L.moshi_hot_codec_slot_close(lm, 0) == -1 and L.moshi_hot_codec_slot_position(lm, 0) == -1
    assert L.moshi_hot_mimi_decode_slots(lm, i32, pcm.ctypes.data, st.ctypes.data) == -1
    L.moshi_hot_free(lm)
    L.ggml_backend_free(be)
