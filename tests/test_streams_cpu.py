"""CPU: lockstep streams (moshi_hot_create_streams) on the host device with the oracle attached - B conversations stepped as one batch give each
conversation exactly what a single-stream model gives it, across the Temporal ring's wrap."""
import ctypes as C

import numpy as np
import pytest

import hot_util as hu
import streams_util as su


@pytest.mark.parametrize("B", [2, 3])
def test_streams_equal_single_stream_models_across_the_ring_wrap(B):
    cfg = su.lm_only(hu.hot.tiny(hu.L))
    n = cfg.context + 4                                     # the 24-slot Temporal ring wraps
    codes = su.stream_codes(cfg, B, n, seed=B)
    got = su.run_streams("oracle", cfg, codes, seed=5, logits=True)
    assert got[0][0] == 0 and all(g[0] == 1 for g in got[1:])
    for b in range(B):
        ref = su.run_single("oracle", cfg, [fr[b] for fr in codes], seed=5, logits=True)
        for k, (g, r) in enumerate(zip(got, ref)):
            assert g[0] == r[0], (b, k)
            if r[0]:
                assert g[1][b] == r[1] and g[2][b] == r[2], (b, k)
            # the oracle quantises and dots every column on its own: the batched logits are the single-stream logits, bit for bit
            assert np.array_equal(g[3][b], r[3]), (b, k)
    # the streams really differ (different inputs): not B copies of one conversation
    assert len({tuple(g[1]) for g in got[1:]}) > 1 or any(len(set(g[1])) > 1 for g in got[1:])


def test_streams_read_last_gives_one_row_per_stream():
    cfg = su.lm_only(hu.hot.tiny(hu.L, layers=1))
    s = su.Streams("oracle", cfg, 2)
    codes = su.stream_codes(cfg, 2, 2, seed=1)
    for fr in codes:
        s.step(fr)
    tout = s.read("transformer_out", cfg.dim)
    dl = s.read("dep_logits0", cfg.card)
    s.free()
    assert tout.shape == (2, cfg.dim) and not np.array_equal(tout[0], tout[1])
    assert dl.shape == (2, cfg.card) and np.isfinite(dl).all()


def test_one_stream_is_the_single_stream_model():
    cfg = su.lm_only(hu.hot.tiny(hu.L))
    codes = su.stream_codes(cfg, 1, 6, seed=3)
    got = su.run_streams("oracle", cfg, codes, seed=2, logits=True)
    ref = su.run_single("oracle", cfg, [fr[0] for fr in codes], seed=2, logits=True)
    for g, r in zip(got, ref):
        assert g[0] == r[0]
        if r[0]:
            assert g[1][0] == r[1] and g[2][0] == r[2]
        assert np.array_equal(g[3][0], r[3])


def _refused(cfg, n_streams):
    be = hu.make_backend("oracle")
    m = hu.L.moshi_hot_create_streams(be, C.byref(cfg), 0, n_streams)
    if m:
        hu.L.moshi_hot_free(m)
    hu.L.ggml_backend_free(be)
    return not m


def test_create_streams_refuses_what_it_does_not_batch():
    base = lambda: su.lm_only(hu.hot.tiny(hu.L, layers=1))
    assert not _refused(base(), 2)
    assert _refused(base(), 17) and _refused(base(), 0)
    pp = hu.hot.tiny_personaplex(hu.L, layers=1)
    pp.enable_mimi_encoder = pp.enable_mimi_decoder = 0
    assert _refused(pp, 2)
    tp = base(); tp.tp_world = 1
    assert _refused(tp, 2)
    codec = hu.hot.tiny(hu.L, layers=1)                     # codec halves on
    assert _refused(codec, 2)
    for field in ("chain_depth", "delay_steps", "extra_heads", "codec_stream"):
        c = base(); setattr(c, field, 1)
        assert _refused(c, 3), field


def test_single_stream_calls_refuse_a_streams_model():
    cfg = su.lm_only(hu.hot.tiny(hu.L, layers=1))
    s = su.Streams("oracle", cfg, 2)
    ia = (C.c_int32 * 32)()
    txt = C.c_int32()
    assert hu.L.moshi_hot_lm_step(s.m, ia, C.byref(txt), ia) == -1
    assert hu.L.moshi_hot_ring_bytes(s.m, 0, 0, 0, None, 0, 0) == -1
    assert hu.L.moshi_hot_host_ring(s.m, None, 0) == -1
    assert hu.L.moshi_hot_n_streams(s.m) == 2
    s.free()
