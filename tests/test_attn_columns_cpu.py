"""The self-attention block at the op level, without a GPU: the CPU oracle against the float64 restatement of tests/attn_ref_util.py over the whole case
table (lockstep, slots, blocks, rows, single column), the caps that keep the near-tie slack from hiding a failure, and the proof that the comparison
discriminates: starting from the oracle's output, every mutation of the reference's inputs or of its semantics must be REJECTED by assert_matches.

This validates the reference and pins the oracle's attention at these shapes; tests/test_attn_columns_gpu.py holds the device to the same reference."""
import numpy as np
import pytest

import attn_ref_util as au

GEOS = list(au.GEOMETRIES.values())
IDS = [g.name for g in GEOS]


def run_table(geo):
    """every case of one geometry on the oracle -> [(form, case, reference, oracle output rows, oracle ring bits)]"""
    res = []

    def streams(form, cases, B, rope, per_stream):
        h = au.StreamsGraph("oracle", geo, B, rope, per_stream)
        for c in cases:
            out, rings = h.run(c)
            res.append((form, c, au.streams_reference(c), out, rings))
        h.free()

    for rope in (True, False):
        streams("lockstep", au.lockstep_cases(geo, 3, rope), 3, rope, False)
    streams("slots", au.slots_cases(geo), 3, True, True)
    streams("single", au.single_cases(geo), 1, True, False)
    jobs = [("rows", c) for c in au.rows_cases(geo)]
    if 4 * geo.D <= 512:
        jobs += [("blocks", c) for c in au.blocks_cases(geo)]
    for form, c in jobs:
        h = au.JobsGraph("oracle", c)
        out, rings = h.run()
        h.free()
        res.append((form, c, au.jobs_reference(c), out, rings))
    return res


@pytest.fixture(scope="module")
def tables():
    t = {g.name: run_table(g) for g in GEOS}
    h = au.StreamsGraph("oracle", au.LONG, 1, True, False)
    t[au.LONG.name] = []
    for c in au.single_cases(au.LONG):
        out, rings = h.run(c)
        t[au.LONG.name].append(("single", c, au.streams_reference(c), out, rings))
    h.free()
    return t


def test_block_mask_of_the_lookup_table_is_the_causal_block():
    # create_bias_pattern / bias_pattern_index against causal_mask_block, for blocks that end at or before the ring's end
    for C, n, pos in [(300, 1, 0), (300, 13, 60), (300, 64, 236), (100, 5, 95), (40, 1, 39), (600, 4, 253)]:
        assert np.array_equal(au.bias_pattern_block(C, n, pos), au.causal_block(C, pos, n)), (C, n, pos)


@pytest.mark.parametrize("name", IDS + [au.LONG.name])
def test_oracle_matches_the_float64_reference(tables, name):
    worst = {}
    for form, case, ref, out, rings in tables[name]:
        w = au.assert_matches(out, rings, ref, case.name)
        worst[form] = max(worst.get(form, 0.0), w)
    print(f"{name}: {len(tables[name])} cases; worst |oracle - reference| / max|reference| over rows without a near tie, per form: "
          + ", ".join(f"{k} {v:.3e}" for k, v in worst.items()))
    # (assert_matches above is the check; this one keeps the recorded figure honest - 2 % for another libm's expf)
    assert max(worst.values()) <= 1.02 * au.ORACLE_WORST, (worst, "the measured worst in attn_ref_util.py is stale: BAR is 4 x that figure")
    assert au.BAR == 4 * au.ORACLE_WORST and au.BAR < 2e-6


def test_every_form_is_in_the_table(tables):
    for g in GEOS:
        forms = {f for f, *_ in tables[g.name]}
        assert forms == ({"lockstep", "slots", "single", "rows", "blocks"} if 4 * g.D <= 512 else {"lockstep", "slots", "single", "rows"}), (g.name, forms)
        ends = {int(np.isfinite(c.masks[0]).nonzero()[0][-1]) + 1 for f, c, *_ in tables[g.name] if f == "lockstep"}
        assert ends == set(g.n_ends), (g.name, ends)


def test_near_tie_caps_hold_for_the_inputs(tables):
    # conditions on the INPUTS, checked on the reference alone: a violated cap is a bad seed, not a kernel failure. Expectation: about 2 tau / 2^-8.
    live = ties = row = 0
    for name, t in tables.items():
        for form, case, ref, _, _ in t:
            live += ref.n_live
            ties += ref.n_ties
            row = max(row, ref.max_row_ties)
            assert ref.max_row_ties <= 8, (case.name, ref.max_row_ties)
    print(f"near ties: {ties} of {live} live probabilities ({100.0 * ties / live:.3f} %), at most {row} in one (column, head, row)")
    assert ties <= 0.002 * live, (ties, live)


# ---- the comparison discriminates ----------------------------------------------------------------------------------------------------------------
def rejected(out, rings, ref, what):
    try:
        au.assert_matches(out, rings, ref, what)
    except AssertionError:
        return True
    return False


def n_end_of(case):
    return int(np.isfinite(case.masks[0]).nonzero()[0][-1]) + 1


def pick(table, form, n_end=None):
    """a RoPE case of a form whose first column ends at n_end and attends to the slot it writes; n_end None: the last case of the form"""
    rows = [r for r in table if r[0] == form]
    if n_end is not None:
        rows = [r for r in rows if r[1].rope and n_end_of(r[1]) == n_end and np.isfinite(r[1].masks[0, r[1].slots[0]]) and "n_end" in r[1].name]
    assert rows, (form, n_end)
    return rows[0] if n_end is not None else rows[-1]


def with_masks(case, masks):
    return case._replace(masks=masks)


def streams_mutations(case):
    """-> {mutation: reference}"""
    C = case.geo.C
    n_end = n_end_of(case)
    muts = {}
    m = case.masks.copy()
    m[0, n_end - 1] = -np.inf
    if n_end > 1:
        muts["the last live slot dropped"] = au.streams_reference(with_masks(case, m))
    m = case.masks.copy()
    mid = n_end // 2 if n_end // 2 != case.slots[0] or n_end < 3 else n_end // 2 - 1
    if n_end > 2:
        m[0, mid] = -np.inf
        muts["one live slot dropped"] = au.streams_reference(with_masks(case, m))
    muts["p not rounded to BF16"] = au.streams_reference(case, "p_unrounded")
    muts["q not rounded to BF16"] = au.streams_reference(case, "q_unrounded")
    if np.isfinite(case.masks[0, case.slots[0]]):
        muts["the written slot read from the old ring"] = au.streams_reference(case, "stale_written")
    if case.rope:
        muts["the RoPE position off by one"] = au.streams_reference(case, position_of=lambda b: case.positions[0 if case.shared else b] + 1)
    if not case.shared:
        muts["column b given column b + 1's mask row"] = au.streams_reference(case, mask_of=lambda b: (b + 1) % case.B)
    assert C == case.masks.shape[1]
    return muts


@pytest.mark.parametrize("name", IDS + [au.LONG.name])
def test_mutations_of_a_streams_step_are_rejected(tables, name):
    table = tables[name]
    geo = au.GEOMETRIES.get(name, au.LONG)
    seen = set()
    for form in (["lockstep", "slots", "single"] if name in au.GEOMETRIES else ["single"]):
        for n_end in (geo.n_ends[1], geo.n_ends[-1]):   # (a single live slot has p = 1 whatever is rounded: the second length of the table, and the longest)
            _, case, ref, out, rings = pick(table, form, n_end)
            assert not rejected(out, rings, ref, case.name)
            for what, mref in streams_mutations(case).items():
                if rejected(out, rings, mref, case.name):
                    seen.add(what)
                else:   # (over two or three live slots the BF16 rounding of p can absorb a rounding left out; over the longest range nothing may pass)
                    assert n_end != geo.n_ends[-1], f"{case.name}: not rejected: {what}"
    must = {"one live slot dropped", "the last live slot dropped", "p not rounded to BF16", "q not rounded to BF16", "the written slot read from the old ring",
            "the RoPE position off by one"} | ({"column b given column b + 1's mask row"} if name in au.GEOMETRIES else set())
    assert must <= seen, must - seen


@pytest.mark.parametrize("name", IDS)
def test_a_row_that_misses_the_previous_rows_store_is_rejected(tables, name):
    for _, case, ref, out, rings in [r for r in tables[name] if r[0] == "rows"]:
        assert not rejected(out, rings, ref, case.name)
        assert rejected(out, rings, au.jobs_reference(case, "stale_rows"), case.name), f"{case.name}: a stale read was not rejected"
        assert rejected(out, rings, au.jobs_reference(case, "p_unrounded"), case.name)
    for _, case, ref, out, rings in [r for r in tables[name] if r[0] == "blocks"]:
        assert rejected(out, rings, au.jobs_reference(case, "stale_written"), case.name), f"{case.name}: a block that attends before its rows are written was not rejected"


@pytest.mark.parametrize("name", IDS)
def test_one_byte_in_an_untouched_ring_column_is_rejected(tables, name):
    # the lowest mantissa bit of one value in a column (rows: one that takes part in no job) and slot the step must not touch
    for form in ("lockstep", "slots", "rows"):
        _, case, ref, out, rings = pick(tables[name], form)
        touched = set(case.slots) if form != "rows" else set()
        b = case.B - 1 if form != "rows" else 2 if all(j.b != 2 for j in case.jobs) else 1
        if form == "rows":
            assert all(j.b != b for j in case.jobs), case.name
        slot = next(c for c in range(case.geo.C - 1, -1, -1) if c not in touched)
        for which in ("kbits", "vbits"):
            bits = getattr(ref, which).copy()
            bits[b, 0, slot, 5] ^= 1   # the lowest mantissa bit of one value
            assert rejected(out, rings, ref._replace(**{which: bits}), case.name), f"{case.name}: a changed {which} value in column {b} slot {slot} was not rejected"
