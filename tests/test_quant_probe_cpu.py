"""CPU: the activation-rounding probe (tests/quant_probe_util.py) against the oracle, and against itself.

(a) the oracle's run of every selector graph equals the numpy reference on every input family, weight type and K in {256, 512, 2560}: as values
    for the selector rows, inside the bar of roundings for the heavy Q4_K row. This holds the oracle to a statement of ggml's quantisers that shares
    no code with it, and shows the selector construction reads what it claims to read. The RMS-norm and gate prologues with their exact inputs too.
(b) every deliberately wrong quantiser is rejected by assert_probe on the committed inputs, in the family built for it.
(c) two changes are NOT rejected, and the tests say why:
      last_tie   taking the last instead of the first +-amax element flips the sign of iscale and of d together: d q and d bsum keep their values
                 (hip_mv_device.h takes the sign from one ballot and calls the choice immaterial - this is the proof);
      no_clamp   min(127, .) never binds on an input ggml defines: iscale = fl(-127 / max) and |x| <= |max| give |fl(iscale x)| <= 127 (1 + 2^-23)^2
                 < 127.5, so 128 is never reached before the clamp. test_the_clamp_never_binds asserts the margin on every family; a family cannot
                 contain a value that "rounds to 128" without |x| > amax, which contradicts amax.
(d) every family contains the case it was written for (counted)."""
import numpy as np
import pytest

import ggml_util as gu
import quant_probe_util as qp
from ggml_util import BF16, F16, Q4_0, Q4_K, Q8_0

f32 = np.float32
KS = [256, 512, 2560]
ROWS = 3
ALL = [(wt, fam) for wt in qp.QUANT + qp.FLOAT for fam in qp.families(wt)]
IDS = [f"{qp.NAMES[wt]}-{fam}" for wt, fam in ALL]


def oracle(build, T, M):
    outs, _ = gu.run_graph("oracle", build)
    return qp.collect(outs, T, M)


# ---- (a) --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("wt,fam", ALL, ids=IDS)
def test_oracle_equals_the_reference(wt, fam, K):
    sel = qp.Selectors(wt, K)
    v = qp.family(wt, fam, K, ROWS)
    ref = qp.reference(wt, v)
    what = f"{qp.NAMES[wt]} {fam} K={K}"
    qp.assert_probe(oracle(qp.probe_graph(sel, v), ROWS, sel.M0), ref, what + " mat-mul", who="oracle", lanes=True)
    qp.assert_probe(oracle(qp.probe_graph(sel, v, per_row=True), ROWS, sel.M0), ref, what + " mat-vecs", who="oracle", lanes=True)


@pytest.mark.parametrize("wt", qp.QUANT + qp.FLOAT, ids=lambda t: qp.NAMES[t])
@pytest.mark.parametrize("K", [512, 2560])
def test_oracle_equals_the_reference_behind_an_rms_norm(wt, K):
    sel = qp.Selectors(wt, K)
    x, alpha = qp.norm_inputs(K, 4, seed=K)
    ref = qp.reference(wt, qp.norm_values(x, alpha))
    qp.assert_probe(oracle(qp.probe_graph(sel, x, "norm", alpha), 4, sel.M0), ref, f"{qp.NAMES[wt]} norm K={K}", who="oracle", lanes=True)


@pytest.mark.parametrize("wt", qp.QUANT + qp.FLOAT, ids=lambda t: qp.NAMES[t])
@pytest.mark.parametrize("random_l", [False, True], ids=["l_32", "l_20_60"])
def test_oracle_equals_the_reference_behind_a_gate(wt, random_l):
    K = 512
    sel = qp.Selectors(wt, K)
    v = qp.family(wt, "random", K, 6) if random_l else qp.stacked(wt, K, 3)      # (60 x the range families would overflow an F16 scale)
    h, seen = qp.gate_inputs(v, seed=5, random_l=random_l)
    if not random_l:
        live = np.abs(v) >= 1e-36                                 # (a denormal over 32 loses bits; the reference sees what the quantiser sees)
        live[:, 11::37] = False
        assert np.array_equal(seen[live], v[live])                # l = 32 hands the family through unchanged
        assert (seen[:, 11::37] == 0).all()
    T = v.shape[0]
    qp.assert_probe(oracle(qp.probe_graph(sel, h, "gate"), T, sel.M0), qp.reference(wt, seen), f"{qp.NAMES[wt]} gate", who="oracle", lanes=True)


def test_cyclic_rows_and_residual_are_read_back():
    K, M = 256, 700
    sel = qp.Selectors(Q4_K, K)
    v = qp.family(Q4_K, "random", K, ROWS)
    ref = qp.reference(Q4_K, v)
    res = np.zeros((ROWS, M), f32)
    got = oracle(qp.probe_graph(sel, v, residual=res, M=M), ROWS, M)
    qp.assert_probe(got, ref, "cyclic", who="oracle", lanes=True)
    assert np.array_equal(got[:, :sel.M0 - 1], got[:, sel.M0:2 * sel.M0 - 1])


def test_restated_quantisers_are_block_arith():
    # the loops the mutations are written into, unmutated, against tests/golden/block_arith.py
    for K in KS:
        for fam in qp.FAMILIES_Q8K:
            v = qp.family(Q4_K, fam, K, ROWS)
            for a, b in zip(qp.q8k_blocks(v), qp.q8k_blocks(v, "restated")):
                assert np.array_equal(a, b), (K, fam)
        for fam in qp.FAMILIES_Q80:
            v = qp.family(Q8_0, fam, K, ROWS)
            for a, b in zip(qp.q80_blocks(v), qp.q80_blocks(v, "restated")):
                assert np.array_equal(a, b), (K, fam)


# ---- (b) --------------------------------------------------------------------------------------------------------------------------------------
REJECTED = [(Q4_K, "half_away", "halves"), (Q4_K, "recip", "random"), (Q4_K, "trunc", "random"), (Q4_K, "neighbour_amax", "random"),
            (Q4_K, "bsum16", "random"), (Q4_K, "bs_hi_div", "const"), (Q4_K, "zero_nan", "zero"),
            (Q8_0, "half_even", "halves"), (Q8_0, "trunc", "random"), (Q8_0, "d_unrounded", "random"), (Q8_0, "d_unrounded", "f16scale"),
            (Q8_0, "d_toward_zero", "f16scale"), (Q8_0, "neighbour_amax", "random"), (Q8_0, "bsum16", "random"), (Q8_0, "zero_nan", "zero"),
            (Q4_0, "half_even", "halves"), (Q4_0, "d_toward_zero", "random"), (Q4_0, "bsum16", "const"),
            (BF16, "bf16_trunc", "edges"), (BF16, "bf16_trunc", "random")]


@pytest.mark.parametrize("wt,mutation,fam", REJECTED, ids=[f"{qp.NAMES[w]}-{m}-{f}" for w, m, f in REJECTED])
def test_mutation_is_rejected(wt, mutation, fam):
    K = 512
    v = qp.family(wt, fam, K, ROWS)
    ref = qp.reference(wt, v)
    qp.assert_probe(qp.as_output(ref), ref, "unmutated")
    with pytest.raises(AssertionError):
        qp.assert_probe(qp.as_output(qp.reference(wt, v, mutation)), ref, mutation)


def test_every_listed_mutation_has_a_rejecting_family():
    seen = {(wt, m) for wt, m, _ in REJECTED}
    assert {m for wt, m in seen if wt == Q4_K} == set(qp.Q8K_MUTATIONS) - {"no_clamp", "last_tie"}
    assert {m for wt, m in seen if wt in (Q8_0, Q4_0)} == set(qp.Q80_MUTATIONS)
    assert {m for wt, m in seen if wt == BF16} == set(qp.FLOAT_MUTATIONS)


# ---- (c) --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", KS)
def test_the_last_of_tied_extremes_gives_the_same_outputs(K):
    flipped = 0
    for fam in qp.FAMILIES_Q8K:
        v = qp.family(Q4_K, fam, K, ROWS)
        ref = qp.reference(Q4_K, v)
        qp.assert_probe(qp.as_output(qp.reference(Q4_K, v, "last_tie")), ref, f"last_tie {fam}")
        flipped += int((np.sign(qp.q8k_blocks(v, "last_tie")[1]) != np.sign(qp.q8k_blocks(v)[1])).sum())
    assert flipped >= 4, "no block in which the first and the last extreme differ in sign: the families lost their ties"


@pytest.mark.parametrize("K", KS)
def test_the_clamp_never_binds(K):
    worst = 0.0
    for fam in qp.FAMILIES_Q8K:
        v = qp.family(Q4_K, fam, K, ROWS)
        q, d, _ = qp.q8k_blocks(v)
        xb = v.reshape(ROWS, -1, 256)
        for t in range(ROWS):
            for b in range(xb.shape[1]):
                j = int(np.argmax(np.abs(xb[t, b])))
                if xb[t, b, j] == 0:
                    continue
                p = np.abs((f32(-127.0) / xb[t, b, j] * xb[t, b]).astype(f32))
                worst = max(worst, float(p.max()))
        ref = qp.reference(Q4_K, v)
        qp.assert_probe(qp.as_output(qp.reference(Q4_K, v, "no_clamp")), ref, f"no_clamp {fam}")     # the same outputs: nothing to clamp
        assert np.abs(q).max() <= 127
    assert 127.0 <= worst <= 127.0 * (1 + 2.0 ** -23) ** 2 < 127.5, worst


# ---- (d) --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", KS)
def test_families_contain_their_cases(K):
    nb = K // 256
    # zero
    v = qp.family(Q4_K, "zero", K, ROWS)
    q, d, _ = qp.q8k_blocks(v)
    assert (v[ROWS - 1] == 0).all() and (d[ROWS - 1] == 0).all()
    if nb >= 2:
        assert ((d[:ROWS - 1] == 0).sum(1) == 1).all()                                 # one zero block in a live row
    if nb >= 3:
        z = np.argwhere(d[:ROWS - 1] == 0)[:, 1]
        assert ((z > 0) & (z < nb - 1)).all()                                          # between live blocks
    _, d80, _ = qp.q80_blocks(v)
    assert ((d80[:ROWS - 1] == 0).sum(1) >= 1).all() and (d80[:ROWS - 1] != 0).any()
    # sign: extreme negative (d > 0 since iscale = -127 / max), ties in both orders
    v = qp.family(Q4_K, "sign", K, ROWS)
    q, d, _ = qp.q8k_blocks(v)
    assert (d[0] > 0).all() and (d[1] < 0).all() and (d[2] > 0).all()
    for t in (1, 2):
        blk = v[t].reshape(nb, 256)
        a = np.abs(blk).max(1, keepdims=True)
        assert ((blk == a).sum(1) == 1).all() and ((blk == -a).sum(1) == 1).all()
    # halves: iscale a power of two, products exact halves, both +-126.5 present
    v = qp.family(Q4_K, "halves", K, ROWS)
    q, d, _ = qp.q8k_blocks(v)
    m, _ = np.frexp(d)
    assert (np.abs(m) == 0.5).all()
    p = v.reshape(ROWS, nb, 256) / d[..., None].astype(np.float64)
    halves = np.abs(p - np.trunc(p)) == 0.5
    assert halves.sum() >= 0.9 * 0.9 * p.size
    assert (np.abs(p) == 126.5).sum() >= 2 * 8 * nb * ROWS and (np.abs(p) == 127).sum() >= 2 * 8 * nb * ROWS
    assert (np.abs(q) == 127).sum() == (np.abs(p) == 127).sum() and (np.abs(q[np.abs(p) == 126.5]) == 126).all()      # to even: 126
    q80, d80, _ = qp.q80_blocks(qp.family(Q8_0, "halves", K, ROWS))
    m, _ = np.frexp(d80)
    assert (m == 0.5).all()
    assert (np.abs(q80) == 127).sum() >= 4 * (K // 32) * ROWS                                                          # away from zero: 126.5 -> 127
    # const: block sums of +-4064
    _, _, bs = qp.q8k_blocks(qp.family(Q4_K, "const", K, ROWS))
    assert (bs == 4064).sum() >= ROWS and (bs == -4064).sum() >= ROWS
    assert ((bs >> 6) == -64).any() and ((bs >> 6) == 63).any()
    _, _, bs = qp.q80_blocks(qp.family(Q8_0, "const", K, ROWS))
    assert (np.abs(bs) == 4064).sum() >= 2 * ROWS
    # f16scale: subnormal scales, scales that round to zero under non-zero values, ties rounding each way
    v = qp.family(Q8_0, "f16scale", K, ROWS)
    q80, d80, _ = qp.q80_blocks(v)
    raw = (np.abs(v.reshape(ROWS, -1, 32)).max(-1) / f32(127.0)).astype(f32)
    assert ((d80 > 0) & (d80 < 2.0 ** -14)).sum() >= ROWS
    assert ((d80 == 0) & (raw > 0)).sum() >= ROWS
    # (a tie: the unrounded scale lies exactly half an F16 step from the rounded one)
    tie = np.abs(d80.astype(np.float64) - raw) * 2 == np.spacing(np.minimum(d80, raw).astype(np.float16)).astype(np.float64)
    tie &= raw >= 2.0 ** -14
    assert (tie & (d80 > raw)).sum() >= 1 and (tie & (d80 < raw)).sum() >= 1, (int((tie & (d80 > raw)).sum()), int((tie & (d80 < raw)).sum()))
    # range: 1e-30 and 1e30 blocks in one row, denormal single elements that are not the extreme
    v = qp.family(Q4_K, "range", K, ROWS)
    _, d, _ = qp.q8k_blocks(v)
    assert (np.abs(d) < 1e-30).any() and (np.abs(d) > 1e26).any() and np.isfinite(d).all()
    if nb >= 2:
        assert ((np.abs(d) < 1e-30).any(1) & (np.abs(d) > 1e26).any(1)).all()
    den = (v != 0) & (np.abs(v) < np.finfo(f32).tiny)
    assert den.sum() == 2 * ROWS
    v = qp.family(Q8_0, "range", K, ROWS)
    _, d80, _ = qp.q80_blocks(v)
    assert np.isfinite(d80).all() and (d80 > 1000).any() and ((v != 0) & (np.abs(v) < np.finfo(f32).tiny)).sum() == 2 * ROWS
    # float edges: ties, carries into the next binade, -0, F16 subnormal results
    for wt in (BF16, F16):
        v = qp.family(wt, "edges", K, ROWS)
        r = qp.round_to_type(v, wt)
        assert np.isfinite(r).all() and np.signbit(v[:, 1]).all() and (v[:, 1] == 0).all()
        drop = 16 if wt == BF16 else 13
        low = v.view(np.uint32) & np.uint32((1 << drop) - 1)
        normal = np.abs(r) >= (2.0 ** -14 if wt == F16 else 0)
        ties = (low == (1 << (drop - 1))) & normal
        assert (ties & (np.abs(r) > np.abs(v))).sum() >= K // 8 and (ties & (np.abs(r) < np.abs(v))).sum() >= K // 8
        assert (np.frexp(r)[1] > np.frexp(v)[1]).sum() >= ROWS                         # rounded up into the next binade
        if wt == F16:
            assert ((r != 0) & (np.abs(r) < 2.0 ** -14)).sum() >= ROWS


# ---- paired gate and general gate values on the oracle ----------------------------------------------------------------------------------------
def test_oracle_equals_the_reference_through_the_exact_gated_pair():
    sel = qp.Selectors(Q4_K, 4352)
    build, seen = qp.paired_gate_case(sel)
    qp.assert_probe(oracle(build, 1, sel.M0), qp.reference(Q4_K, seen), "gated pair", who="oracle", lanes=True)


GENERAL = [(512, 8), (512, 17), (4352, 6)]      # the shapes tests/test_quant_probe_gpu.py runs, with its seeds


@pytest.mark.parametrize("wt", qp.QUANT, ids=lambda t: qp.NAMES[t])
@pytest.mark.parametrize("K,T", GENERAL)
def test_general_gate_values_under_the_tolerant_form(wt, K, T):
    h, v = qp.gate_general(K, T, seed=K + T)
    share = float(qp.near_boundary(wt, v).mean())
    assert 0 < share <= 0.01, share                           # the cap on what the tolerant form does not hold exactly, met by the reference alone
    sel = qp.Selectors(wt, K)
    got = oracle(qp.probe_graph(sel, h, "gate"), T, sel.M0)
    near, moved = qp.assert_probe_tolerant(got, wt, v, f"{qp.NAMES[wt]} K={K} T={T}")
    print(f"{qp.NAMES[wt]} K={K} T={T}: {near:.4%} of the elements near a boundary, {moved} blocks with a neighbouring scale (oracle)")
    # and the tolerant form is no blanket: a quantiser that truncates, sums 16 values, looks at the wrong block or keeps a float32 scale is still rejected
    # (round-half-away and the reciprocal form are not: random values hold no exact halves, and the reciprocal moves the scale by the ulp allowed)
    for wrong in (("trunc", "bsum16", "neighbour_amax") if wt == Q4_K else ("trunc", "bsum16", "d_unrounded")):
        with pytest.raises(AssertionError):
            qp.assert_probe_tolerant(qp.as_output(qp.reference(wt, v, wrong)), wt, v, wrong)
