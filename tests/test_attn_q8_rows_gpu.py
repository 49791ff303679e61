"""GPU: one layer's ring-ordered rows over Q8_0 K / V rings through the C-ABI (kv_q8 = 7, hip_attn_q8_rows.h): n consecutive one-row
blocks of attention_jobs() on one column of Q8_0 [D, C, H, B] rings, every slot holding a random prior row and every mask row open, as ONE k_attn_rows_q8
launch and as plain nodes (flag 1), against a float64 restatement that goes row by row - quantise the row, write its slot, attend over the ring as it then
stands: attn_ref_util.BAR plus attn_q8_util's slack, ring bytes equal. Runs: full, wrapping, across a tile at odd n, shortest, two jobs, a closed range."""
import numpy as np
import pytest

import attn_q8_util as q8
import attn_ref_util as ar
from ggml_util import F32, I32, Q8_0

pytestmark = pytest.mark.gpu

C, H, B, Job = 256, 2, 3, ar.Job
RUNS = {"s0_n16": [Job(1, 0, 16, C, True)], "s250_n16": [Job(1, 0, 16, C + 250, True)], "s127_n5": [Job(1, 0, 5, C + 127, True)], "s3_n2": [Job(1, 0, 2, C + 3, True)],
        "two_jobs": [Job(2, 0, 16, C + 40, True), Job(0, 16, 3, C + 200, True)], "closed_range": [Job(1, 0, 6, C + 100, True)]}


def sequences(case, name):
    seqs = ar.jobs_sequences(case)[0]
    if name == "closed_range":   # row 2 does not see old slots 30 .. 89, row 4 neither those nor the slots rows 0 and 1 wrote
        for t, (lo, hi) in ((2, (30, 90)), (4, (30, 102))):
            seqs[t] = seqs[t]._replace(mask=np.where((np.arange(C) >= lo) & (np.arange(C) < hi), -np.inf, seqs[t].mask).astype(np.float32))
    return seqs


def reference(case, seqs):
    kr, vr = q8.rings_of(case)
    outs, slacks = [], []
    for s in seqs:   # one row: into its slot, then over the ring as it stands
        Hn, _, D = s.q.shape
        kr[s.b][:, s.idx, :] = q8.q8_rows(ar.rope_rows(s.k, s.rot))
        vr[s.b][:, s.idx, :] = q8.q8_rows(s.v)
        (kq, kd), (vq, vd), (qq, qd) = q8.q8_fields(kr[s.b]), q8.q8_fields(vr[s.b]), q8.q8_fields(q8.q8_rows(ar.rope_rows(s.q, s.rot)))
        terms = np.einsum("hcbk,htbk->htcb", kq, qq).astype(np.float32) * (kd[:, None] * qd[:, :, None]).astype(np.float32)
        score = np.zeros(terms.shape[:3], np.float32)
        for b in range(terms.shape[3]):
            score = (score + terms[..., b]).astype(np.float32)
        x = (score * np.float32(ar.attn_scale(D))).astype(np.float32) + s.mask[None].astype(np.float32)
        live = np.isfinite(x)
        x64 = np.where(live, x, -np.inf).astype(np.float64)
        e = np.where(live, np.exp(x64 - x64.max(axis=-1, keepdims=True)), 0.0)
        p = e / e.sum(axis=-1, keepdims=True)
        V = (vd[..., None] * vq.astype(np.float32)).astype(np.float32).reshape(Hn, -1, D).astype(np.float64)
        tau = 2.0 * (4.0 + 2.0 * np.where(live, np.abs(x64), 0.0).max(axis=-1)) * 2.0 ** -24
        outs.append(np.einsum("htc,hcd->htd", p, V))
        slacks.append(tau[..., None] * np.einsum("htc,hcd->htd", p, np.abs(V)))
    return ar.Ref(outs, slacks, kr.view(np.uint16), vr.view(np.uint16), 0, 0, 0, 0.0)


def run(case, seqs, flags):
    """a pass of ring-ordered rows, every one-row sequence expanded before the next is built -> ([per row [H, 1, D]], [K, V ring as uint16], plan counters)"""
    D, T = case.geo.D, case.proj.shape[0]
    g = ar.gu.Graph("hip", mem_mb=96, graph_size=8192)
    g.set_flags(flags)
    proj, iota = g.input(case.proj.astype(np.float32)), g.input(np.arange(C), I32)
    rings = [g.new(Q8_0, D, C, H, case.B), g.new(Q8_0, D, C, H, case.B)]
    consts = [(g.input(s.mask), g.input(s.idx.astype(np.int32), I32), g.input(s.rot)) for s in seqs]
    g.graph = g.L.ggml_new_graph_custom(g.ctx, g.graph_size, False)
    halves = [(g.view_2d(rot, D // 2, 1, rot.contents.nb[1], 0), g.view_2d(rot, D // 2, 1, rot.contents.nb[1], 4 * (D // 2))) for _, _, rot in consts]
    [g.L.ggml_build_forward_expand(g.graph, rotr) for rotr, _ in halves]
    p, row_nb, out_row, U64 = proj.contents, proj.contents.nb[1], D * H * 4, 1 << 64
    out, out_at = g.new(F32, D, H, T), 0
    for row, ((mask, idx, _), (rotr, roti), s) in enumerate(zip(consts, halves, seqs)):
        def rows(off):
            return g.permute(g.reshape_4d(g.cont(g.view_3d(proj, p.ne[0] // 3, 1, 1, row_nb, row_nb, row * row_nb + off)), D, H, 1, 1), 0, 2, 1, 3)
        q, k = ar._apply_rope(g, rows(0), rows(row_nb // 3), rotr, roti)
        k, v = (g.set_rows(g.view_3d(r, D, C, H, r.contents.nb[1], r.contents.nb[2], s.b * r.contents.nb[3]), x, idx) for r, x in zip(rings, (k, rows(row_nb * 2 // 3))))
        w = g.soft_max_ext(g.mul_mat(k, q), mask, ar.attn_scale(D), 0.0)
        o = g.mul_mat(g.cont(g.transpose(g.get_rows(v, g.view_2d(iota, C, H, 0, 0)))), w)
        out = g.cpy(g.permute(o, 0, 2, 1, 3), g.view_3d(out, D, H, 1, D * 4, out_row, ((row - out_at) * out_row) % U64))
        out_at = row
        g.L.ggml_build_forward_expand(g.graph, out)
    out = g.view_3d(out, D * H, T, 1, out_row, out_row * T, (-out_at * out_row) % U64)
    g.L.ggml_build_forward_expand(g.graph, out)
    g.alloc()
    for t, arr in zip(rings, q8.rings_of(case)):
        ar._set_raw(g, t, arr)
    g.compute()
    x, got = g.get(out).reshape(T, H, D), []
    for t in rings:
        buf = np.zeros(g.L.ggml_nbytes(t), np.uint8)
        g.L.ggml_backend_tensor_get(t, buf.ctypes.data, 0, buf.nbytes)
        got.append(buf.view(np.uint16).reshape(case.B, H, C, -1))
    res =[np.ascontiguousarray(x[r:r + 1].transpose(1, 0, 2)) for r in range(T)], got, g.stats()
    g.free()
    return res


@pytest.mark.parametrize("flags", [0, 1], ids=["fused", "plain_nodes"])
@pytest.mark.parametrize("name", list(RUNS))
@pytest.mark.parametrize("D", [64, 128])
def test_ring_ordered_rows_match_the_row_by_row_contract(D, name, flags):
    case = ar.jobs_case(q8.geometry(D, H, C), B, RUNS[name], True, seed=len(name) + D, name=f"q8 rows d{D} {name}")
    seqs = sequences(case, name)
    out, rings, st = run(case, seqs, flags)
    ref = reference(case, seqs)
    print(f"{case.name} flags {flags}: worst |got - ref| / max|ref| {max(float(np.abs(o - r).max() / np.abs(r).max()) for o, r in zip(out, ref.out)):.3e}")
    ar.assert_matches(out, rings, ref, case.name)
    want = (0, 0, 0) if flags else (1, len(case.jobs), len(seqs))
    assert (st.attn_row_launches_in_last_plan, st.attn_row_jobs_in_last_plan, st.attn_row_rows_in_last_plan) == want
    assert st.attn_block_launches_in_last_plan == 0 and st.q8_attention_blocks_in_last_plan == 0 and (flags or st.generic_attention_nodes_in_last_plan == 0)


@pytest.mark.parametrize("D", [64, 128])
def test_a_jobs_bits_do_not_depend_on_its_column_or_its_neighbours(D):
    geo = q8.geometry(D, H, C)
    a = ar.jobs_case(geo, B, RUNS["s250_n16"], True, seed=3)
    rows = np.concatenate([a.proj, ar.qkv_rows(np.random.default_rng(8), 9, H, D)])
    b = a._replace(jobs=[Job(2, 0, 9, C + 40, True), Job(0, 9, 16, C + 250, True)], proj=np.concatenate([rows[16:], rows[:16]]), kbits=a.kbits[[1, 2, 0]], vbits=a.vbits[[1, 2, 0]])
    (oa, (ka, va), _), (ob, (kb, vb), _) = run(a, sequences(a, ""), 0), run(b, sequences(b, ""), 0)
    assert np.array_equal(np.stack(oa), np.stack(ob[9:])) and np.array_equal(ka[1], kb[0]) and np.array_equal(va[1], vb[0])
