"""Helpers for the float-accumulating BF16 / F16 mat-mul (ggml_backend_mi355x_set_float_accumulate, k_mm_f32acc_batched): a graph runner that sets
the mode on the handle before the compute, integer operands, and a CPU float32 emulation of the kernel's summation order."""
import numpy as np

import ggml_util as gu

MMA_U = 4        # hip_mm_float_acc.h: chunks of 32 k dealt in groups of four round-robin to four waves
WAVES = 4


def run_hip(build_fn, mode=1, flags=0, modes=None):
    """build_fn(g) -> outputs, on a fresh MI355X handle in `mode`. modes: a sequence of modes - one compute per entry on the SAME handle and graph.
    -> ([arrays], stats), or a list of such pairs with `modes`"""
    g = gu.Graph("hip")
    try:
        if flags:
            g.set_flags(flags)
        outs = build_fn(g)
        g.build(outs)
        g.alloc()
        res = []
        for m in ([mode] if modes is None else modes):
            g.L.ggml_backend_mi355x_set_float_accumulate(g.backend, m)
            g.compute()
            res.append(([g.get(o) for o in outs], g.stats()))
        return res[0] if modes is None else res
    finally:
        g.free()


def integer_operands(K, M, T):
    """integers of -8 .. 8: exact in BF16 and F16, every partial sum of K <= 11264 products below 2^24 - float sums are exact in any order"""
    r = np.random.default_rng(11 * K + 5 * M + T)
    return r.integers(-8, 9, (M, K)).astype(np.float32), r.integers(-8, 9, (T, K)).astype(np.float32)


def emulate(w, xr):
    """w [M, K], xr [T, K] (both already the values the weight's type holds) -> [T, M] float32 in the kernel's order: wave v takes the chunk groups
    v, v + 4, .. in increasing order, sums sequentially in float32 inside its partition (what the MFMA does inside its 32 terms is not documented;
    a sequential float32 sum is the least favourable reading), and the partial sums meet as ((p0 + p1) + p2) + p3"""
    w, xr = np.asarray(w, np.float32), np.asarray(xr, np.float32)
    K = w.shape[1]
    nch = K // 32
    parts = []
    for v in range(WAVES):
        acc = np.zeros((xr.shape[0], w.shape[0]), np.float32)
        for c in range(nch):
            if (c // MMA_U) % WAVES != v:
                continue
            for k in range(32 * c, 32 * c + 32):
                acc += xr[:, k, None] * w[None, :, k]      # (the product is exact in float32)
        parts.append(acc)
    return ((parts[0] + parts[1]) + parts[2]) + parts[3]
