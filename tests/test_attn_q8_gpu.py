"""GPU: one self-attention block over Q8_0 K / V rings through the C-ABI (moshi_hot_config::kv_q8, hip_attn_q8.h), as the one
k_attn_streams_q8 launch and as plain nodes (backend flag 1), against attn_q8_util's float64 restatement of the contract: outputs within
attn_ref_util.BAR plus the derived slack, ring bytes equal in every slot of every column.

Shapes: (D, H) = (128, 2) and (64, 3); C = 9 (odd: rows and heads 8- / 4-byte aligned only, the wrap inside one tile), 250 and 300 (the live range
crosses the 128-slot tile border); fills of 1 slot, C - 1 and a full ring written in the middle (past the wrap); lockstep B = 2 with RoPE, slots B = 3
(every column at its own position; column 1 frozen at position 0, as a closed slot is stepped) with RoPE at D = 128 and without at D = 64."""
import numpy as np
import pytest

import attn_q8_util as q8
import attn_ref_util as ar

pytestmark = pytest.mark.gpu

SHAPES = [(D, H, C) for D, H in ((128, 2), (64, 3)) for C in (9, 250, 300)]


def lockstep_cases(geo):
    C = geo.C
    return [ar.streams_case(geo, 2, [n], [slot], True, seed=11 * n + slot, shared=True, name=f"{geo.name} lockstep n_end {n} slot {slot}")
            for n, slot in ((1, 0), (C - 1, C - 2), (C, C // 2))]


def slots_cases(geo):
    C, rope = geo.C, geo.D == 128
    return [ar.streams_case(geo, 3, n_ends, slots, rope, seed=500 + n_ends[0], shared=False, name=f"{geo.name} slots n_ends {n_ends}")
            for n_ends, slots in (([C - 1, 1, C], [C - 2, 0, C // 2]), ([C, C - 1, 1], [0, C - 2, 0]))]


def columns(case, cols):
    """the case with columns `cols` only, in that order"""
    cols = list(cols)
    return case._replace(B=len(cols), proj=case.proj[cols], masks=case.masks[cols], slots=[case.slots[b] for b in cols],
                         positions=[case.positions[b] for b in cols], kbits=case.kbits[cols], vbits=case.vbits[cols])


@pytest.mark.parametrize("flags", [0, 1], ids=["fused", "plain_nodes"])
@pytest.mark.parametrize("per_stream", [False, True], ids=["lockstep", "slots"])
@pytest.mark.parametrize("D,H,C", SHAPES)
def test_q8_attention_block_matches_the_contract(D, H, C, per_stream, flags):
    geo = q8.geometry(D, H, C)
    cases = slots_cases(geo) if per_stream else lockstep_cases(geo)
    g = q8.Q8Graph("hip", geo, cases[0].B, cases[0].rope, per_stream, flags=flags)
    try:
        for case in cases:
            out, rings = g.run(case)
            ref = q8.reference(case)
            worst = max(float(np.abs(o - r).max() / np.abs(r).max()) for o, r in zip(out, ref.out))
            print(f"{case.name} flags {flags}: worst |got - ref| / max|ref| {worst:.3e} (bar {ar.BAR:.3e} + slack)")
            ar.assert_matches(out, rings, ref, case.name)
        st = g.stats()
        if flags == 0:
            assert (st.q8_attention_blocks_in_last_plan, st.kernels_in_last_plan) == (1, 1)
        else:
            assert st.q8_attention_blocks_in_last_plan == 0
    finally:
        g.free()


@pytest.mark.parametrize("D,H,C", [(128, 2, 300), (64, 3, 9)])
def test_a_columns_bits_do_not_depend_on_its_neighbours_or_its_place(D, H, C):
    geo = q8.geometry(D, H, C)
    case = slots_cases(geo)[0]
    got = {}
    for name, cols in (("B3", [0, 1, 2]), ("B2", [0, 1]), ("swapped", [2, 1, 0])):
        g = q8.Q8Graph("hip", geo, len(cols), case.rope, True)
        try:
            got[name] = g.run(columns(case, cols))
        finally:
            g.free()
    (o3, (k3, v3)), (o2, (k2, v2)), (os_, (ks, vs)) = got["B3"], got["B2"], got["swapped"]
    assert np.array_equal(o3[0], o2[0]) and np.array_equal(k3[0], k2[0]) and np.array_equal(v3[0], v2[0])      # column 0 at B = 3 and B = 2
    assert np.array_equal(o3[0], os_[2]) and np.array_equal(k3[0], ks[2]) and np.array_equal(v3[0], vs[2])     # the same conversation in column 2
    assert np.array_equal(o3[2], os_[0]) and np.array_equal(k3[2], ks[0]) and np.array_equal(v3[2], vs[0])
