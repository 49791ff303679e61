"""CPU: the f32_matrix field of struct moshi_hot_config (include/moshi_hot.h) - its place in the struct, its default, and the host backend ignoring it."""
import ctypes as C

import numpy as np

import codec_slots_util as cu
import hot_util as hu

L = hu.L


def test_config_has_the_c_structs_size_with_f32_matrix_in_front_of_float_accumulate():
    # moshi_hot_config_moshika clears sizeof(struct moshi_hot_config) bytes before it fills them: the bytes it leaves alone start at the struct's end
    n = C.sizeof(hu.hot.Config)
    buf = (C.c_uint8 * (n + 64))(*([0xAA] * (n + 64)))
    L.moshi_hot_config_moshika(C.cast(buf, C.POINTER(hu.hot.Config)))
    raw = bytes(buf)
    assert raw[n:] == b"\xaa" * 64, "the C struct is larger than hot.Config"
    assert 0xAA not in raw[n - 8:n], "the C struct is smaller than hot.Config"
    assert hu.hot.Config.f32_matrix.offset == n - 8 and hu.hot.Config.float_accumulate.offset == n - 4
    assert all(fill(L).f32_matrix == 0 for fill in (hu.hot.moshika, hu.hot.personaplex, hu.hot.tiny))


def test_host_backend_ignores_f32_matrix():
    pcm = {}
    for on in (0, 1):
        cfg = cu.cfg_of()
        cfg.f32_matrix = on
        s = cu.CodecSlots("oracle", cfg, 2, seed=3)
        assert s.open(0) == 0 and s.open(1) == 0
        pcm[on] = np.stack([s.decode([cu.codes(900)[k], cu.codes(902)[k]])[1] for k in range(2)])
        s.free()
    assert np.isfinite(pcm[0]).all() and np.abs(pcm[0]).max() > 0 and np.array_equal(pcm[0], pcm[1])
