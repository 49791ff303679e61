"""GPU: one layer's slot-prefill attention over Q8_0 K / V rings through the C-ABI (kv_q8 = 3, hip_attn_q8_blocks.h): attention_jobs()'s
graph over column views of Q8_0 [D, C, H, B] rings with a random prior ring, as the k_attn_blocks_q8 launch pair and as plain nodes (flag 1), against
attn_q8_util.reference restated for T rows per job (all written before any attends): attn_ref_util.BAR plus the slack tau x sum p |V|, ring bytes equal.
Jobs (pos, T): one row into an empty ring, a whole row tile, a tile and a tail, a live range across the 128-slot tile at odd row alignment, three row
tiles ending exactly at C, two jobs of different T in one launch."""
import numpy as np
import pytest

import attn_q8_util as q8
import attn_ref_util as ar
from ggml_util import F32, I32, Q8_0

pytestmark = pytest.mark.gpu

C, H, B = 256, 2, 3
Job = ar.Job
JOBS = {"p0_t1": [Job(1, 0, 1, 0, False)], "p0_t16": [Job(1, 0, 16, 0, False)], "p3_t17": [Job(1, 0, 17, 3, False)], "p120_t17": [Job(1, 0, 17, 120, False)],
        "p223_t33": [Job(1, 0, 33, 223, False)], "two_jobs": [Job(2, 0, 5, 100, False), Job(0, 5, 20, 7, False)]}


def reference(case):
    kr, vr = q8.rings_of(case)
    outs, slacks = [], []
    for s in ar.jobs_sequences(case)[0]:
        Hn, T, D = s.q.shape
        q, k = ar.rope_rows(s.q, s.rot), ar.rope_rows(s.k, s.rot)
        kr[s.b][:, s.idx, :] = q8.q8_rows(k)
        vr[s.b][:, s.idx, :] = q8.q8_rows(s.v)
        (kq, kd), (vq, vd), (qq, qd) = q8.q8_fields(kr[s.b]), q8.q8_fields(vr[s.b]), q8.q8_fields(q8.q8_rows(q))
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


def run(case, flags):
    """ar.JobsGraph over Q8_0 rings, with the dequantising get_rows(v, iota) in front of the transpose (iota [C] viewed [C, H] with a zero stride)
    -> ([per job [H, n, D]], [K ring, V ring as uint16 [B, H, C, ROWB / 2]], plan counters)"""
    D, T = case.geo.D, case.proj.shape[0]
    g = ar.gu.Graph("hip", mem_mb=96, graph_size=8192)
    g.set_flags(flags)
    proj, iota = g.input(case.proj.astype(np.float32)), g.input(np.arange(C), I32)
    rings = [g.new(Q8_0, D, C, H, case.B), g.new(Q8_0, D, C, H, case.B)]
    consts = [(g.input(s.mask), g.input(s.idx.astype(np.int32), I32), g.input(s.rot)) for s in ar.jobs_sequences(case)[0]]
    g.graph = g.L.ggml_new_graph_custom(g.ctx, g.graph_size, False)
    p, row_nb, out_row, U64 = proj.contents, proj.contents.nb[1], D * H * 4, 1 << 64
    out, out_at = g.new(F32, D, H, T), 0
    for (mask, idx, rot), s in zip(consts, case.jobs):
        def rows(off):
            return g.permute(g.reshape_4d(g.cont(g.view_3d(proj, p.ne[0] // 3, s.n, 1, row_nb, row_nb * s.n, s.row * row_nb + off)), D, H, s.n, 1), 0, 2, 1, 3)
        nb1 = rot.contents.nb[1]
        q, k = ar._apply_rope(g, rows(0), rows(row_nb // 3), g.view_2d(rot, D // 2, s.n, nb1, 0), g.view_2d(rot, D // 2, s.n, nb1, 4 * (D // 2)))
        k, v = (g.set_rows(g.view_3d(r, D, C, H, r.contents.nb[1], r.contents.nb[2], s.b * r.contents.nb[3]), x, idx) for r, x in zip(rings, (k, rows(row_nb * 2 // 3))))
        w = g.soft_max_ext(g.mul_mat(k, q), mask, ar.attn_scale(D), 0.0)
        o = g.mul_mat(g.cont(g.transpose(g.get_rows(v, g.view_2d(iota, C, H, 0, 0)))), w)
        out = g.cpy(g.permute(o, 0, 2, 1, 3), g.view_3d(out, D, H, s.n, D * 4, out_row, ((s.row - out_at) * out_row) % U64))
        out_at = s.row
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
    res = [np.ascontiguousarray(x[s.row:s.row + s.n].transpose(1, 0, 2)) for s in case.jobs], got, g.stats()
    g.free()
    return res


@pytest.mark.parametrize("flags", [0, 1], ids=["fused", "plain_nodes"])
@pytest.mark.parametrize("jobs", list(JOBS))
@pytest.mark.parametrize("D", [64, 128])
def test_q8_prefill_attention_matches_the_contract(D, jobs, flags):
    case = ar.jobs_case(q8.geometry(D, H, C), B, JOBS[jobs], True, seed=len(jobs) + D, name=f"q8 blocks d{D} {jobs}")
    out, rings, st = run(case, flags)
    ref = reference(case)
    print(f"{case.name} flags {flags}: worst |got - ref| / max|ref| {max(float(np.abs(o - r).max() / np.abs(r).max()) for o, r in zip(out, ref.out)):.3e}")
    ar.assert_matches(out, rings, ref, case.name)
    want = (0, 0, 0) if flags else (2, len(case.jobs), 0)
    assert (st.attn_block_launches_in_last_plan, st.attn_block_jobs_in_last_plan, st.q8_attention_blocks_in_last_plan) == want
    assert flags or st.generic_attention_nodes_in_last_plan == 0


@pytest.mark.parametrize("D", [64, 128])
def test_a_jobs_bits_do_not_depend_on_its_column_or_its_neighbours(D):
    geo = q8.geometry(D, H, C)
    a = ar.jobs_case(geo, B, JOBS["p120_t17"], True, seed=3)
    rows = np.concatenate([a.proj, ar.qkv_rows(np.random.default_rng(8), 9, H, D)])
    b = a._replace(jobs=[Job(2, 0, 9, 40, False), Job(0, 9, 17, 120, False)], proj=np.concatenate([rows[17:], rows[:17]]), kbits=a.kbits[[1, 2, 0]], vbits=a.vbits[[1, 2, 0]])
    (oa, (ka, va), _), (ob, (kb, vb), _) = run(a, 0), run(b, 0)
    assert np.array_equal(oa[0], ob[1]) and np.array_equal(ka[1], kb[0]) and np.array_equal(va[1], vb[0])
