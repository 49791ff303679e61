"""GPU: one self-attention block over Q8_0 K / V rings as the k_attn_streams_q8_split launch pair (ggml_backend_mi355x_set_attn_q8_split,
hip_attn_q8_split.h) through the C-ABI, against attn_q8_util's float64 restatement of the contract: outputs within attn_ref_util.BAR plus
the derived slack of DESIGN.md 35, ring bytes equal in every slot of every column.

Shapes: (D, H) = (128, 2) and (64, 3); C = 600 - three chunks of 256 slots, the last partial; forced S = 2 (slices of 2 and 1 chunks) and S = 3;
fills of 1 slot (one chunk: the other slices are empty and still arrive), C - 1, a full ring written in the middle of a chunk (356) and on a chunk's
first row (512 / 256); lockstep B = 2 with RoPE, slots B = 3 with every column at its own position and one column frozen at position 0 beside full
ones. A column's bits depend neither on S nor on B nor on its place; a hipGraph replay finds the arrival counters at zero."""
import numpy as np
import pytest

import attn_q8_util as q8
import attn_ref_util as ar

pytestmark = pytest.mark.gpu
C = 600
SHAPES = [(128, 2), (64, 3)]


def columns(case, cols):
    """the case with columns `cols` only, in that order"""
    cols = list(cols)
    return case._replace(B=len(cols), proj=case.proj[cols], masks=case.masks[cols], slots=[case.slots[b] for b in cols],
                         positions=[case.positions[b] for b in cols], kbits=case.kbits[cols], vbits=case.vbits[cols])


def cases_of(geo, per_stream):
    if per_stream:
        return [ar.streams_case(geo, 3, n_ends, slots, True, seed=500 + n_ends[0], shared=False, name=f"{geo.name} slots n_ends {n_ends} slots {slots}")
                for n_ends, slots in (([C - 1, 1, C], [C - 2, 0, 356]), ([C, C, 1], [512, 256, 0]))]
    return [ar.streams_case(geo, 2, [n], [slot], True, seed=11 * n + slot, shared=True, name=f"{geo.name} lockstep n_end {n} slot {slot}")
            for n, slot in ((1, 0), (C - 1, C - 2), (C, 356), (C, 512))]


def graph(geo, B, per_stream, split):
    g = q8.Q8Graph("hip", geo, B, True, per_stream)
    g.g.L.ggml_backend_mi355x_set_attn_q8_split(g.g.backend, split)
    return g


def plan_counts(g):
    st = g.stats()
    return st.q8_attention_split_blocks_in_last_plan, st.q8_attention_blocks_in_last_plan, st.kernels_in_last_plan


@pytest.mark.parametrize("S", [2, 3])
@pytest.mark.parametrize("per_stream", [False, True], ids=["lockstep", "slots"])
@pytest.mark.parametrize("D,H", SHAPES)
def test_split_block_matches_the_contract(D, H, per_stream, S):
    geo = q8.geometry(D, H, C)
    cases = cases_of(geo, per_stream)
    g = graph(geo, cases[0].B, per_stream, S)
    try:
        for case in cases:
            out, rings = g.run(case)
            ref = q8.reference(case)
            worst = max(float(np.abs(o - r).max() / np.abs(r).max()) for o, r in zip(out, ref.out))
            print(f"{case.name} S {S}: worst |got - ref| / max|ref| {worst:.3e} (bar {ar.BAR:.3e} + slack)")
            ar.assert_matches(out, rings, ref, case.name)
        assert plan_counts(g) == (1, 0, 2)
        again, rings_again = g.run(cases[-1])   # a hipGraph replay: the arrival counters were left at zero
        assert all(np.array_equal(a, o) for a, o in zip(again, out)) and all(np.array_equal(a, r) for a, r in zip(rings_again, rings))
        g.g.L.ggml_backend_mi355x_set_attn_q8_split(g.g.backend, 0)   # drops the plan: the unsplit launch
        out, rings = g.run(cases[-1])
        ar.assert_matches(out, rings, ref, cases[-1].name + " unsplit")
        assert plan_counts(g) == (0, 1, 1)
    finally:
        g.free()


@pytest.mark.parametrize("D,H", SHAPES)
def test_a_columns_bits_depend_on_neither_the_split_nor_its_neighbours_nor_its_place(D, H):
    geo = q8.geometry(D, H, C)
    case = cases_of(geo, True)[0]
    got = {}
    for name, cols, S in (("S2", [0, 1, 2], 2), ("S3", [0, 1, 2], 3), ("B2", [0, 1], 2), ("swapped", [2, 1, 0], 3)):
        g = graph(geo, len(cols), True, S)
        try:
            got[name] = g.run(columns(case, cols))
            assert plan_counts(g) == (1, 0, 2)
        finally:
            g.free()

    def same(a, i, b, j):
        (oa, (ka, va)), (ob, (kb, vb)) = got[a], got[b]
        return np.array_equal(oa[i], ob[j]) and np.array_equal(ka[i], kb[j]) and np.array_equal(va[i], vb[j])

    assert all(same("S2", b, "S3", b) for b in range(3))                   # S = 2 and S = 3
    assert same("S2", 0, "B2", 0) and same("S2", 1, "B2", 1)                # B = 3 and B = 2
    assert same("S2", 0, "swapped", 2) and same("S2", 2, "swapped", 0)      # two columns in swapped places
