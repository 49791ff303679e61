"""GPU: one residual-VQ level at B columns (k_vq_level_cols) through the C-ABI alone. The graph is built node for node as moshi_hot.cpp builds it for an
encoder-slots model (codebook_encode over the B residuals as its rows, vq_decode at B columns, the residual subtraction): two levels, the second
without a next residual, as the last level of a stack is. The device's codes and new residuals must be the oracle's bit for bit - the search is exact
wherever the best two scores of a column differ, which the inputs guarantee - and a column's result must not depend on its place or on B."""
import functools

import numpy as np
import pytest

import ggml_util as gu

pytestmark = pytest.mark.gpu

D = 256
NO_COLUMN_GROUPS = 8192
CASES = [(B, NC) for NC in (2048, 40) for B in (2, 5, 64)]      # NC = 40: 2 full workgroups of 16 centroids and one of 8 (no multiple of 16)


def level(g, emb, resid, ones, one, NC, B, last):
    """codebook_encode + vq_decode + sub of rvq_encode_columns -> (codes I32 [B], codes F32 [B], next residual [1, D, B] or None)"""
    a = g.cont(g.reshape_2d(resid, D, B))
    a = g.reshape_3d(a, D, 1, B)
    a = g.repeat_4d(a, D, NC, B, 1)
    a = g.reshape_3d(a, D, NC * B, 1)
    b = g.repeat_4d(emb, D, NC * B, 1, 1)
    d = g.sub(b, a)
    d = g.mul(d, d)
    d = g.sum_rows(d)
    d = g.reshape_3d(d, NC, B, 1)
    d = g.add(d, one)
    d = g.div(ones, d)
    idx = g.argmax(d)
    idf = g.cast(idx, gu.F32)
    if last:
        return idx, idf, None
    q = g.get_rows(emb, g.reshape_1d(g.cont(g.reshape_2d(idx, 1, B)), B))
    q = g.cont(g.permute(g.reshape_3d(q, D, 1, B), 1, 0, 2, 3))
    return idx, idf, g.sub(resid, q)


def run(kind, embs, resid, flags=0):
    """two levels over resid [B, D] with codebooks embs = (E0, E1) [NC, D] -> (codes0 [B], codes1 [B], residual after level 0 [B, D]), stats"""
    B, NC = resid.shape[0], embs[0].shape[0]

    def build(g):
        e0, e1 = g.input(embs[0]), g.input(embs[1])
        r = g.input(resid.reshape(B, D, 1))
        one = g.input(np.ones(1, np.float32))
        i0, f0, r1 = level(g, e0, r, g.input(np.ones((B, NC), np.float32)), one, NC, B, False)
        i1, f1, _ = level(g, e1, r1, g.input(np.ones((B, NC), np.float32)), one, NC, B, True)
        return [f0, f1], [i0, i1, r1]
    outs, stats = gu.run_graph(kind, build, flags=flags)
    f0, f1, i0, i1 = (a.reshape(-1) for a in outs[:4])
    r1 = outs[4]
    assert np.array_equal(f0, i0.astype(np.float32)) and np.array_equal(f1, i1.astype(np.float32))
    return (i0, i1, r1.reshape(B, D)), stats


def scores(E, x):
    """the level's scores of one residual as the graph computes them: float differences and squares, summed in double from element 0 up, 1 / (float + 1)"""
    d = E - x[None, :]
    acc = np.cumsum((d * d).astype(np.float64), axis=1)[:, -1]
    return np.float32(1) / (acc.astype(np.float32) + np.float32(1))


def clear_winner(v, tie=None):
    """the best two scores differ by more than a few float steps (so another summation order cannot swap them); `tie`: an index pair whose scores are
    equal on purpose - then the pair leads and the third score is clear of it"""
    order = np.argsort(v, kind="stable")
    top = v[order[-1]]
    if tie is not None:
        if not (v[tie[0]] == v[tie[1]] == top):
            return False
        rest = np.delete(v, list(tie))
        return top - rest.max() > 8 * np.spacing(top)
    return top - v[order[-2]] > 8 * np.spacing(top)


@functools.lru_cache(maxsize=None)
def case(B, NC):
    """Inputs with the planted columns, drawn again (next seed) until every column of both levels has a clear winner; the oracle's results for them.
    Column 0: centroids DUP = (3, NC - 2) are bit-identical and nearest - first against last workgroup, the later index must win. Column 1: the
    residual IS centroid 5, in the first workgroup's slice. Computed once per case and never changed."""
    dup = (3, NC - 2)
    for seed in range(100, 140):
        rng = np.random.default_rng(seed * 1000 + B * 7 + NC)
        E0 = rng.standard_normal((NC, D)).astype(np.float32)
        E1 = rng.standard_normal((NC, D)).astype(np.float32)
        E0[dup[1]] = E0[dup[0]]
        x = rng.standard_normal((B, D)).astype(np.float32)
        x[0] = E0[dup[0]] + (0.05 * rng.standard_normal(D)).astype(np.float32)
        x[1] = E0[5]
        if not all(clear_winner(scores(E0, x[b]), dup if b == 0 else None) for b in range(B)):
            continue
        (i0, i1, r1), _ = run("oracle", (E0, E1), x)
        if all(clear_winner(scores(E1, r1[b])) for b in range(B)):
            break
    else:
        raise AssertionError("no seed gave clear winners")
    # the oracle did what the planted cases say, and the score restatement above is the oracle's arithmetic
    assert i0[0] == dup[1] and i0[1] == 5 and np.all(r1[1] == 0)
    for b in range(B):
        v = scores(E0, x[b])
        assert i0[b] == np.flatnonzero(v == v.max())[-1]
    for a in (E0, E1, x, i0, i1, r1):
        a.setflags(write=False)
    return (E0, E1), x, (i0, i1, r1)


@pytest.mark.parametrize("B,NC", CASES)
def test_codes_and_residuals_equal_the_oracle_bit_for_bit(B, NC):
    embs, x, ref = case(B, NC)
    got, stats = run("hip", embs, x)
    assert stats.vq_column_levels_in_last_plan == 2, "the levels did not take the B-column launch"
    for r, g, what in zip(ref, got, ("level 0 codes", "level 1 codes", "residuals")):
        assert np.array_equal(r, g), (what, np.argwhere(r != g)[:5])
    plain, stats = run("hip", embs, x, flags=NO_COLUMN_GROUPS)
    assert stats.vq_column_levels_in_last_plan == 0
    for r, g in zip(ref, plain):
        assert np.array_equal(r, g)


@pytest.mark.parametrize("B,NC", CASES)
def test_a_column_is_a_function_of_its_residual_alone(B, NC):
    embs, x, _ = case(B, NC)
    got, _ = run("hip", embs, x)
    for b in sorted({0, 1, B // 2, B - 1}):
        pair = np.stack([x[b], x[(b + 1) % B]])
        alone, stats = run("hip", embs, pair)
        assert stats.vq_column_levels_in_last_plan == 2
        assert alone[0][0] == got[0][b] and alone[1][0] == got[1][b], (b, alone[0][0], got[0][b])
        assert np.array_equal(alone[2][0], got[2][b]), b
