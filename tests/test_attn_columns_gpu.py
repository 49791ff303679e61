"""-m gpu: the self-attention body behind its launch forms, op by op, against the float64 reference of tests/attn_ref_util.py.

Every form and case of the table (tests/test_attn_columns_cpu.py runs the same table on the oracle): the device under default flags, with the backend's
counters proving that the intended launch ran - k_attn_streams (lockstep, slots), k_attn_blocks, k_attn_rows, k_attn_decode (single column) - and the
device with backend flag 1 (plain nodes, no attention launch), both through assert_matches: |got - ref| <= BAR * max|ref| + near-tie slack, the same
finite pattern, the K / V ring bytes equal in every slot of every column. The stated bit-identities are asserted as such: a column of a streams launch is
the single-column launch of that column's inputs (where that launch runs the same body), slots at one position are lockstep, a rows job is its rows as
consecutive one-row graphs.

One device handle is live at a time (tests/test_attn_short_tail_gpu.py, run_steps); a handle per geometry and form, inputs rewritten between computes,
so that the second and later computes replay the captured graph. D 256 has no blocks case (k_attn_blocks asserts 4 D <= 512) and no rows case on the
device: a run of rows the planner declined would go to k_attn_blocks."""
import numpy as np
import pytest

import attn_ref_util as au

pytestmark = pytest.mark.gpu

FLAG_GENERIC = 1
GEOS = list(au.GEOMETRIES.values())
IDS = [g.name for g in GEOS]
JOB_GEOS = [g for g in GEOS if 4 * g.D <= 512]
JOB_IDS = [g.name for g in JOB_GEOS]
MODES = [(0, "fused"), (FLAG_GENERIC, "generic")]
_refs = {}


def ref_of(case):
    """the reference of a case, computed once"""
    if case.name not in _refs:
        _refs[case.name] = au.jobs_reference(case) if isinstance(case, au.JobsCase) else au.streams_reference(case)
    return _refs[case.name]


def no_attention_launch_counted(st, what):
    assert st.attn_block_launches_in_last_plan == 0 and st.attn_row_launches_in_last_plan == 0 and st.attention_folds_planned == 0, what


def run_streams(geo, cases, B, rope, per_stream, flags, form):
    """all cases on one handle, each checked against the reference -> {case name: (output rows, ring bits)}"""
    h = au.StreamsGraph("hip", geo, B, rope, per_stream, flags)
    got, worst = {}, 0.0
    try:
        for c in cases:
            out, rings = h.run(c)
            worst = max(worst, au.assert_matches(out, rings, ref_of(c), f"{c.name} flags {flags}"))
            got[c.name] = (out, rings)
        st = h.stats()
    finally:
        h.free()
    what = (f"{geo.name} {form} flags {flags}: {st.kernels_in_last_plan} launches, {st.generic_attention_nodes_in_last_plan} generic soft_max / set_rows, "
            f"{st.graph_replays} replays")
    print(f"{what}; worst |device - reference| / max|reference| over rows without a near tie {worst:.3e}")
    no_attention_launch_counted(st, what)
    if flags & FLAG_GENERIC:
        assert st.generic_attention_nodes_in_last_plan == 3 and st.kernels_in_last_plan > 3, what
    else:   # the whole graph is the one launch: k_attn_streams (B > 1) or k_attn_decode (B = 1)
        assert st.generic_attention_nodes_in_last_plan == 0 and st.kernels_in_last_plan == 1, what
        assert not rope or len(cases) < 3 or st.graph_replays > 0, what   # (a graph of fewer than 32 nodes - no RoPE - is planned afresh every time)
    return got


def run_jobs(case, flags, expect):
    h = au.JobsGraph("hip", case, flags)
    try:
        out, rings = h.run()
        st = h.stats()
    finally:
        h.free()
    worst = au.assert_matches(out, rings, ref_of(case), f"{case.name} flags {flags}")
    got = (st.attn_block_launches_in_last_plan, st.attn_block_jobs_in_last_plan, st.attn_row_launches_in_last_plan, st.attn_row_jobs_in_last_plan, st.attn_row_rows_in_last_plan)
    what = (f"{case.name} flags {flags}: {st.kernels_in_last_plan} launches, block launches / jobs, row launches / jobs / rows {got}, "
            f"{st.generic_attention_nodes_in_last_plan} generic soft_max / set_rows")
    print(f"{what}; worst |device - reference| / max|reference| over rows without a near tie {worst:.3e}")
    n_seq = sum(len(au.job_sequences(j)) for j in case.jobs)
    if flags & FLAG_GENERIC:
        assert got == (0, 0, 0, 0, 0) and st.generic_attention_nodes_in_last_plan == 3 * n_seq, what
    else:
        assert got == expect and st.generic_attention_nodes_in_last_plan == 0, what
        assert st.kernels_in_last_plan == got[0] + got[2], what   # nothing but the attention launches
    return out, rings


def same_bits(a, b, what):
    assert a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32)), f"{what}: output bits differ at {np.argwhere(a != b)[:4].tolist()}"


# ---- lockstep and slots: k_attn_streams --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags,mode", MODES, ids=[m for _, m in MODES])
@pytest.mark.parametrize("geo", GEOS, ids=IDS)
def test_lockstep_streams_match_the_reference(geo, flags, mode):
    for rope in (True, False):
        run_streams(geo, au.lockstep_cases(geo, 3, rope), 3, rope, False, flags, "lockstep")


@pytest.mark.parametrize("flags,mode", MODES, ids=[m for _, m in MODES])
@pytest.mark.parametrize("geo", GEOS, ids=IDS)
def test_slots_match_the_reference(geo, flags, mode):
    run_streams(geo, au.slots_cases(geo), 3, True, True, flags, "slots")


@pytest.mark.parametrize("flags,mode", MODES, ids=[m for _, m in MODES])
@pytest.mark.parametrize("geo", GEOS + [au.LONG], ids=IDS + [au.LONG.name])
def test_single_column_matches_the_reference(geo, flags, mode):
    run_streams(geo, au.single_cases(geo), 1, True, False, flags, "single")


# the single-column launch of these geometries runs attn_decode_body as one workgroup per head, the call k_attn_streams makes; D 64 on a ring of 100 goes
# to attn_ring256_kernel, another kernel, and is held to the reference only (above)
BODY_GEOS = [g for g in GEOS if not (g.D == 64 and g.C <= 256)]


@pytest.mark.parametrize("geo", BODY_GEOS, ids=[g.name for g in BODY_GEOS])
def test_a_column_of_a_streams_launch_is_the_single_column_launch_bit_for_bit(geo):
    lock, slots = au.lockstep_cases(geo, 3, True), au.slots_cases(geo)
    got = run_streams(geo, lock, 3, True, False, 0, "lockstep")
    got.update(run_streams(geo, slots, 3, True, True, 0, "slots"))
    singles = [au.column_case(c, b) for c in lock + slots for b in range(3)]
    one = run_streams(geo, singles, 1, True, False, 0, "single")
    for c in lock + slots:
        out, (kb, vb) = got[c.name]
        for b in range(3):
            o1, (k1, v1) = one[au.column_case(c, b).name]
            same_bits(out[b], o1[0], f"{c.name} column {b} against its single-column launch")
            assert np.array_equal(kb[b], k1[0]) and np.array_equal(vb[b], v1[0]), f"{c.name} column {b}: ring bytes differ from the single-column launch"


@pytest.mark.parametrize("geo", GEOS, ids=IDS)
def test_slots_at_one_position_are_lockstep_bit_for_bit(geo):
    cases = [au.same_position_case(geo, n) for n in geo.n_ends]
    lock = run_streams(geo, cases, 3, True, False, 0, "lockstep")
    slots = run_streams(geo, cases, 3, True, True, 0, "slots")
    for c in cases:
        for b in range(3):
            same_bits(lock[c.name][0][b], slots[c.name][0][b], f"{c.name} column {b}: slots against lockstep")
        assert np.array_equal(lock[c.name][1][0], slots[c.name][1][0]) and np.array_equal(lock[c.name][1][1], slots[c.name][1][1]), c.name


# ---- slot prefill: k_attn_blocks and k_attn_rows ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags,mode", MODES, ids=[m for _, m in MODES])
@pytest.mark.parametrize("geo", JOB_GEOS, ids=JOB_IDS)
def test_block_jobs_match_the_reference(geo, flags, mode):
    for c in au.blocks_cases(geo):
        launches, jobs = au.blocks_expect(c)
        run_jobs(c, flags, (launches, jobs, 0, 0, 0))


@pytest.mark.parametrize("flags,mode", MODES, ids=[m for _, m in MODES])
@pytest.mark.parametrize("geo", JOB_GEOS, ids=JOB_IDS)
def test_ring_ordered_rows_match_the_reference(geo, flags, mode):
    for c in au.rows_cases(geo):
        run_jobs(c, flags, au.rows_expect(c))


@pytest.mark.parametrize("geo", JOB_GEOS, ids=JOB_IDS)
def test_a_rows_job_is_its_rows_as_consecutive_one_row_graphs_bit_for_bit(geo):
    case = au.rows_cases(geo)[0]
    out, (kb, vb) = run_jobs(case, 0, au.rows_expect(case))
    seqs, _ = au.jobs_sequences(case)
    at = 0
    for job in case.jobs:
        rows = au.job_sequences(job)
        # one handle per ring column: a graph of one one-row sequence, whose row, mask row, ring slot and RoPE row are rewritten between computes; the
        # rings stay on the device from row to row
        one = au.jobs_case(geo, case.B, [au.Job(job.b, 0, 1, job.pos, False)], True, 0, f"{case.name}: column {job.b} row by row")
        one = one._replace(kbits=case.kbits, vbits=case.vbits, proj=case.proj[job.row:job.row + 1])
        h = au.JobsGraph("hip", one)
        try:
            for t, r in enumerate(rows):
                h.set_sequence(0, seqs[at + t])
                o1, (k1, v1) = h.run(proj=case.proj[r.row:r.row + 1])
                same_bits(out[at + t], o1[0], f"{case.name} column {job.b} row {t} against a graph of that row alone")
            st = h.stats()
        finally:
            h.free()
        assert (st.attn_block_launches_in_last_plan, st.attn_block_jobs_in_last_plan, st.attn_row_launches_in_last_plan) == (2, 1, 0)
        assert np.array_equal(kb[job.b], k1[job.b]) and np.array_equal(vb[job.b], v1[job.b]), f"{case.name} column {job.b}: ring bytes differ from the row by row run"
        at += len(rows)
