"""CPU: bit 2 of f32_matrix (include/moshi_hot.h) is a device plan, not a graph change - on the host backend decoder and encoder slots give the same
bytes with 0, 4 and 7 - and pkg.Stats lists the fields of struct ggml_mi355x_stats in the header's order, the new counter last. (The setter's mask and
MI355X_MMF32 need a device handle: tests/test_conv_matrix_gpu.py.)"""
import os
import re

import numpy as np

import codec_slots_util as cu
import encoder_slots_util as eu
import hot_util as hu


def test_stats_mirror_has_the_headers_fields_in_order():
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "ggml-backend.h")).read()
    body = re.search(r"struct ggml_mi355x_stats \{(.*?)\n\};", header, re.S).group(1)
    names = re.findall(r"^\s*int64_t\s+(\w+);", body, re.M)
    assert names == [n for n, _ in hu.pkg.Stats._fields_] and names[-1] == "conv_matrix_groups_in_last_plan"


def test_host_backend_ignores_the_conv_bit():
    pcm, codes = {}, {}
    for value in (0, 4, 7):
        cfg = cu.cfg_of()
        cfg.f32_matrix = value
        s = cu.CodecSlots("oracle", cfg, 2, seed=3)
        assert s.open(0) == 0 and s.open(1) == 0
        pcm[value] = np.stack([s.decode([cu.codes(900)[k], cu.codes(902)[k]])[1] for k in range(2)])
        s.free()
        cfg = eu.cfg_of()
        cfg.f32_matrix = value
        s = eu.EncoderSlots("oracle", cfg, 2, seed=3)
        assert s.open(0) == 0 and s.open(1) == 0
        codes[value] = np.stack([np.concatenate([s.encode([eu.pcm(900)[k], eu.pcm(902)[k]])[1].ravel(), *[a.ravel() for a in s.latents()]]) for k in range(2)])
        s.free()
    assert np.isfinite(pcm[0]).all() and np.abs(pcm[0]).max() > 0
    assert all(np.array_equal(pcm[0], pcm[v]) and np.array_equal(codes[0], codes[v]) for v in (4, 7))
