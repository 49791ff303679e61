"""CPU: the host backend ignores bit 1 of f32_matrix (include/moshi_hot.h): decoder slots decode to the same bytes with 0, 2 and 3."""
import numpy as np

import codec_slots_util as cu


def test_host_backend_ignores_the_convtr_bit():
    pcm = {}
    for value in (0, 2, 3):
        cfg = cu.cfg_of()
        cfg.f32_matrix = value
        s = cu.CodecSlots("oracle", cfg, 2, seed=3)
        assert s.open(0) == 0 and s.open(1) == 0
        pcm[value] = np.stack([s.decode([cu.codes(900)[k], cu.codes(902)[k]])[1] for k in range(2)])
        s.free()
    assert np.isfinite(pcm[0]).all() and np.abs(pcm[0]).max() > 0 and np.array_equal(pcm[0], pcm[2]) and np.array_equal(pcm[0], pcm[3])
