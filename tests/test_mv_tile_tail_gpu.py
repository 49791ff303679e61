"""The tile loops of the block mat-vec (matvec_q4k_kernel, WS == 0) and of the merged in_proj + attention launch (inproj_attn_kernel),
moshi.cpp_amd/csrc/hip_kernels_fused.hip: a wave runs STEADY rounds (stage its tile, request the next one, dot) while it has a tile after the current one,
then a TAIL (stage, dot, no request). The shapes below are the smallest that put each combination on the device - waves with no tile, tail-only waves,
one and two steady rounds in front of the tail, a partial last tile, a short last workgroup, the paired gate's source switch, the merged launch's three
segment sources - for every weight format that shares the loop. launch_shape() restates k_matvec's dispatch (default switches); each case asserts the
tiles per workgroup it is meant to have, so a later change of the dispatch cannot silently empty it.

Every mat-vec case goes through ggml_util.compare against the oracle at the mat-vec bar of tests/test_hip_ops.py (atol_rel = 2e-6); the merged launch is
compared bit for bit with the two launches it replaces, as tests/test_attn_fold.py does.

Merged launch: a model's in_proj has K = dim = H x 128 rows per segment, so a workgroup of the 256 holds 3 x (dim / 256)^2 / 64 tiles - 3 at dim 2048,
12 at dim 4096; no model has 6 (that needs K = 4096 over 16 heads of 128, which is a head width of 256 in a model and keeps the attention a launch of
its own). The K = 4096 case therefore runs at 32 heads: 12 tiles, waves 0-3 one steady round and the tail, waves 4-7 the tail only."""
import numpy as np
import pytest

import ggml_util as gu
from ggml_util import Q4_K, Q8_0, Q4_0

pytestmark = pytest.mark.gpu

XBLK_BYTES = 304
RANDOM = {Q4_K: gu.random_q4_K, Q8_0: gu.random_q8_0, Q4_0: gu.random_q4_0}


def launch_shape(K, M, wtype, pair_F=0):
    """(waves, rows per workgroup, workgroups) of k_matvec for a tile-loop (WS == 0) launch; asserts that the launch is one."""
    nb = K // 256
    tile_bytes = 64 * 272 if wtype == Q8_0 else 64 * 144
    tiles_total = (M * nb + 63) // 64
    nw = 4
    if tiles_total >= 256 * 6:
        nw = 8
        rows = (M + 255) // 256
        while rows * nb > 4096:
            rows = (rows + 1) // 2
    else:
        tpw = max(4, nb // 4)
        rows = (tpw * 64 + nb - 1) // nb
        if rows * nb > 4096:
            rows = 4096 // nb
        while rows > 1 and (M + rows - 1) // rows < 128 and (rows // 2) * nb >= 64:
            rows >>= 1
    if wtype == Q8_0 and nw > 4:
        assert nb * XBLK_BYTES + 8 * tile_bytes + rows * nb * 4 <= 158 * 1024
    if pair_F:
        assert M == 2 * pair_F and wtype != Q8_0
        h = (pair_F + 255) // 256
        while (h * nb) % 64:
            h += 1
        assert pair_F % h == 0 and 2 * h * nb <= 4096 and pair_F // h >= 128 and pair_F > 4096
        nw, rows = 8, 2 * h
    direct = not pair_F and wtype == Q4_K and nw == 4 and tiles_total <= 512 and nb <= nw * 8 * 4
    assert not direct, "the register form (WS == 1) has no tile loop"
    grid = pair_F // (rows // 2) if pair_F else (M + rows - 1) // rows
    return nw, rows, grid


def tiles(rows, nb):
    return (rows * nb + 63) // 64


def rounds(nw, ntiles):
    """Per wave: (steady rounds, has a tail)."""
    out = []
    for w in range(nw):
        mine = len(range(w, ntiles, nw))
        out.append((max(mine - 1, 0), mine > 0))
    return out


def norm_residual(K, M, wtype, seed):
    r = np.random.default_rng(seed)
    x = r.standard_normal((1, K)).astype(np.float32)
    alpha = (1.0 + 0.1 * r.standard_normal((1, K))).astype(np.float32)
    res = r.standard_normal((1, M)).astype(np.float32)
    wraw = RANDOM[wtype](r, M, K)

    def build(g):
        w = g.input_raw(wraw, wtype, K, M)
        xn = g.mul(g.input(alpha), g.rms_norm(g.input(x), 1e-8))
        return [g.add(g.input(res), g.mul_mat(w, xn))]
    return build


def plain_residual(K, M, wtype, seed):
    r = np.random.default_rng(seed)
    x = r.standard_normal((1, K)).astype(np.float32)
    res = r.standard_normal((1, M)).astype(np.float32)
    wraw = RANDOM[wtype](r, M, K)

    def build(g):
        return [g.add(g.input(res), g.mul_mat(g.input_raw(wraw, wtype, K, M), g.input(x)))]
    return build


@pytest.mark.parametrize("wtype", [Q4_K, Q8_0, Q4_0])
def test_eight_waves_tail_only_two_waves_without_a_tile(wtype):
    K, M = 4096, 6144
    nw, rows, grid = launch_shape(K, M, wtype)
    assert (nw, rows, grid, tiles(rows, 16)) == (8, 24, 256, 6)
    assert rounds(8, 6) == [(0, True)] * 6 + [(0, False)] * 2
    gu.compare(norm_residual(K, M, wtype, 61), atol_rel=2e-6)


@pytest.mark.parametrize("wtype", [Q4_K, Q8_0, Q4_0])
def test_eight_waves_two_rounds_partial_last_tile_short_last_workgroup(wtype):
    K, M = 4096, 9467
    nw, rows, grid = launch_shape(K, M, wtype)
    assert (nw, rows, grid) == (8, 37, 256)
    assert tiles(rows, 16) == 10 and rows * 16 - 9 * 64 == 16            # the last tile holds 16 super-blocks
    last_rows = M - (grid - 1) * rows
    assert last_rows == 32 and last_rows * 16 == 8 * 64                  # the last workgroup: exactly 8 tiles, every wave the tail only
    assert rounds(8, 10) == [(1, True)] * 2 + [(0, True)] * 6
    gu.compare(norm_residual(K, M, wtype, 62), atol_rel=2e-6)


def test_eight_waves_three_rounds():
    K, M = 4096, 17408
    nw, rows, grid = launch_shape(K, M, Q4_K)
    assert (nw, rows, grid, tiles(rows, 16)) == (8, 68, 256, 17)
    assert rounds(8, 17) == [(2, True)] + [(1, True)] * 7                # wave 0: steady, steady, tail
    gu.compare(norm_residual(K, M, Q4_K, 63), atol_rel=2e-6)


def test_four_waves_short_last_workgroup_one_wave_idle():
    K, M = 4096, 4090
    nw, rows, grid = launch_shape(K, M, Q4_K)
    assert (nw, rows, grid, tiles(rows, 16)) == (4, 16, 256, 4)
    last_blocks = (M - (grid - 1) * rows) * 16
    assert last_blocks == 160 and tiles(M - (grid - 1) * rows, 16) == 3  # 2.5 tiles: wave 3 has none, wave 2 half a tile
    gu.compare(plain_residual(K, M, Q4_K, 64), atol_rel=2e-6)


def test_four_waves_q8_0_short_last_workgroup():
    K, M = 1024, 1000
    nw, rows, grid = launch_shape(K, M, Q8_0)
    assert (nw, rows, grid, tiles(rows, 4)) == (4, 16, 63, 1)
    assert (M - (grid - 1) * rows) * 4 == 32                             # the last workgroup: half a tile
    gu.compare(plain_residual(K, M, Q8_0, 65), atol_rel=2e-6)


def test_paired_gate_five_tiles_per_half_feeding_five_tiles_on_four_waves():
    # the graph of test_hip_ops.py::test_paired_gate_ffn_matches_oracle_and_can_be_switched_off at F = 5120: linear_in in the paired form (8 waves, 10 tiles,
    # the source switches from W_l to W_r at tile 5: waves 0 and 1 request a W_r tile from a W_l round), linear_out on 4 waves with 5 tiles (wave 0: steady, tail)
    K, F = 4096, 5120
    nw, rows, grid = launch_shape(K, 2 * F, Q4_K, pair_F=F)
    assert (nw, rows, grid, tiles(rows, 16), tiles(rows // 2, 16)) == (8, 40, 256, 10, 5)
    assert rounds(8, 10) == [(1, True)] * 2 + [(0, True)] * 6
    nw, rows, grid = launch_shape(F, K, Q4_K)
    assert (nw, rows, grid, tiles(rows, 20)) == (4, 16, 256, 5)
    assert rounds(4, 5) == [(1, True)] + [(0, True)] * 3
    r = np.random.default_rng(66)
    x = r.standard_normal((1, K)).astype(np.float32)
    alpha = (1.0 + 0.1 * r.standard_normal((1, K))).astype(np.float32)
    res = r.standard_normal((1, K)).astype(np.float32)
    w_in = gu.random_q4_K(r, 2 * F, K)
    w_out = gu.random_q4_K(r, K, F)

    def build(g):
        xn = g.mul(g.input(alpha), g.rms_norm(g.input(x), 1e-8))
        h = g.mul_mat(g.input_raw(w_in, Q4_K, K, 2 * F), xn)
        hh = h.contents
        left = g.view_4d(h, hh.ne[0] // 2, 1, hh.ne[1], hh.ne[2], hh.nb[1] // 2, hh.nb[1], hh.nb[2], 0)
        right = g.view_4d(h, hh.ne[0] // 2, 1, hh.ne[1], hh.ne[2], hh.nb[1] // 2, hh.nb[1], hh.nb[2], hh.nb[1] // 2)
        y = g.mul_mat(g.input_raw(w_out, Q4_K, F, K), g.mul(g.silu(left), right))
        return [g.add(g.input(res), y)]
    ref, got, st = gu.compare(build, atol_rel=2e-6)
    assert st.fused_nodes_in_last_plan >= 6, "linear_in did not take the paired form"


@pytest.mark.parametrize("dim,heads,ntiles", [(2048, 16, 3), (4096, 32, 12)])
def test_merged_launch_small_ring_equals_separate_launches_bit_for_bit(dim, heads, ntiles):
    import test_attn_fold as taf
    nb, seg_rows = dim // 256, dim // 256                                # 256 workgroups: rows per (workgroup, segment) = heads x 128 / 256
    assert dim // heads == 128 and (seg_rows * nb) % 64 == 0 and 3 * seg_rows * nb // 64 == ntiles
    assert rounds(8, ntiles) == {3: [(0, True)] * 3 + [(0, False)] * 5, 12: [(1, True)] * 4 + [(0, True)] * 4}[ntiles]
    cfg = taf.temporal_cfg(64, dim=dim, heads=heads)
    tail, st = taf.run("hip", cfg, 4, fill=40)
    assert st.attention_folds_planned >= cfg.num_layers, f"the attention was not merged ({st.attention_folds_planned})"
    plain, st0 = taf.run("hip", cfg, 4, flags=512, fill=40)
    assert st0.attention_folds_planned == 0
    taf.assert_same(plain, tail, f"dim {dim}, ring of 64, 40 live slots")
