"""Dumps everything a set of free-running frame-driver scenarios produces - tokens, status values, snapshot blobs, K / V rings, graph op sequences -
as one text file (a digest per array, the small integer ones in full), to compare two BUILDS of the driver byte for byte on one machine:

    git worktree add /tmp/parent HEAD~1 && bash /tmp/parent/moshi.cpp_amd/build.sh        # the other build, side by side: its two
    mkdir -p build_parent && cp /tmp/parent/moshi.cpp_amd/lib*.so build_parent/               # libraries, kept next to each other
    python __graft_entry__.py                                                                # this build (and the oracle)
    python tests/microbench/driver_dump.py --kind oracle --out new.txt
    MI355X_LIB=$PWD/build_parent/libggml-mi355x.so python tests/microbench/driver_dump.py --kind oracle --out old.txt
    cmp old.txt new.txt

MI355X_LIB names the boundary library of the build to load; the harness library libmoshi-hot.so is taken from the same directory.
--kind hip runs the same on the MI355X. Scenarios: the serial single-stream loop (greedy, seeded-sampled), the chain_depth = 2 run-ahead pipeline,
moshi_hot_prefill, PersonaPlex batched prompts, lockstep streams (B = 2), slots (B = 3: staggered opens, hold + prefill, fork, save / load)."""
import argparse
import ctypes
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
import hot_util as hu  # noqa: E402
import sampling_util as sp  # noqa: E402
import slot_prefill_util as pu  # noqa: E402
import slot_state_util as ss  # noqa: E402
import streams_util as su  # noqa: E402

L = hu.L
LIBC = ctypes.CDLL(None)
SAMPLING = (1234, 0.9, 0.6, 12, 17)
LINES = []


def put(name, value):
    a = np.ascontiguousarray(value)
    line = f"{name} {a.dtype} {list(a.shape)} {hashlib.sha256(a.tobytes()).hexdigest()}"
    if a.dtype.kind in "iu" and a.size <= 512:
        line += " " + " ".join(str(int(v)) for v in a.reshape(-1))
    LINES.append(line)


def put_steps(name, results):
    """results of lm_step / sts_frame style calls: tuples of ints, lists and arrays"""
    for k, r in enumerate(results):
        for j, v in enumerate(r):
            put(f"{name}[{k}].{j}", np.array(v) if not isinstance(v, np.ndarray) else v)


def put_graphs(name, m):
    for which in (0, 1):
        g = L.moshi_hot_graph(m, which)
        if not g:
            LINES.append(f"{name}.graph{which} none")
            continue
        ops = [L.ggml_op_name(L.ggml_graph_node(g, i).contents.op).decode() for i in range(L.ggml_graph_n_nodes(g))]
        shapes = [tuple(L.ggml_graph_node(g, i).contents.ne) for i in range(len(ops))]
        LINES.append(f"{name}.graph{which} {len(ops)} {hashlib.sha256(repr(list(zip(ops, shapes))).encode()).hexdigest()} {' '.join(ops)}")


def put_rings(name, m):
    for layer, kv, buf in m.rings(0):
        put(f"{name}.ring{layer}.{kv}", buf)
    put(f"{name}.host_ring", m.host_ring())
    put(f"{name}.offset", np.array(L.moshi_hot_offset(m.m)))


def tiny_lm(**kw):
    return su.lm_only(hu.hot.tiny(L, **kw))


def serial(kind, sampled):
    cfg = tiny_lm(layers=2)
    codes = pu.live_codes(cfg, 12, 3)
    if sampled:
        cfg = sp.sampled(cfg, *SAMPLING[1:])
    m = sp.Model(kind, cfg, seed=5)
    if sampled:
        assert m.set_sampling(0, *SAMPLING) == 0
    name = "serial." + ("sampled" if sampled else "greedy")
    put_steps(name, [m.lm_step(c) + (m.read("text_logits", cfg.text_card),) for c in codes])
    put_rings(name, m)
    put_graphs(name, m.m)
    m.free()


def run_ahead(kind, model):
    cfg = hu.hot.tiny(L, layers=2) if model == "tiny" else hu.hot.tiny_personaplex(L, layers=2)
    cfg.codec_stream, cfg.chain_depth = 1, 2
    n = 2 * max(cfg.delays[i] for i in range(cfg.n_q + 1)) + 8 + 4
    rng = np.random.default_rng(7)
    frames = [rng.standard_normal(1920).astype(np.float32) * 0.1 for _ in range(n)]
    m = hu.Model(kind, cfg, seed=2)
    put_steps(f"run_ahead.{model}", m.sts_pipeline(frames))
    put_rings(f"run_ahead.{model}", m)
    put_graphs(f"run_ahead.{model}", m.m)
    m.free()


def prefill(kind, model):
    cfg = tiny_lm(layers=2) if model == "tiny" else su.lm_only(hu.hot.tiny_personaplex(L, layers=2))
    m = hu.Model(kind, cfg, seed=3)
    n_in = cfg.n_q - cfg.io_dep_q
    name = f"prefill.{model}"
    put_steps(name + ".before", [m.lm_step(list(range(n_in)))])
    if model == "tiny":
        m.prefill(pu.history(cfg, 11, 9), 4)
    else:
        m.system_prompts([21, 22, 23, 24, 25], batched=True, chunk=8)
    put_rings(name, m)
    put(name + ".transformer_out", m.read("transformer_out", cfg.dim))
    put_steps(name + ".after", [m.lm_step([(k + i) % cfg.card for i in range(n_in)]) + (m.read("text_logits", cfg.text_card),) for k in range(4)])
    put_rings(name + ".end", m)
    m.free()


def lockstep(kind):
    cfg = tiny_lm(layers=2)
    put_steps("lockstep", su.run_streams(kind, cfg, su.stream_codes(cfg, 2, 8, seed=4), seed=5, logits=True))


def slots(kind, sampled):
    cfg = tiny_lm(context=24)
    if sampled:
        cfg = sp.sampled(cfg)
    name = "slots." + ("sampled" if sampled else "greedy")
    s = ss.Slots(kind, cfg, 3, seed=5)
    LIBC.srand(4242)       # unseeded sampled columns draw from libc rand(); reseeded AFTER the model is up (the HIP runtime draws from it while it starts)
    if sampled:
        assert s.set_sampling(0, *SAMPLING) == 0
    codes = {b: pu.live_codes(cfg, 40, 60 + b) for b in range(3)}
    at = {b: 0 for b in range(3)}

    def step(tag, live):
        r = ss.step_all(s, {b: codes[b][at[b]] for b in live})
        for b in live:
            at[b] += 1
        put_steps(f"{name}.{tag}", [r])

    assert s.open(0) == 0
    for k in range(3):
        step(f"a{k}", [0])
    assert s.open(1) == 0                                   # staggered: slot 1 joins three frames later
    for k in range(3):
        step(f"b{k}", [0, 1])
    assert s.open(2) == 0 and s.hold(2, True) == 0          # slot 2 is admitted with a history while the others keep stepping
    assert s.prefill([(2, pu.history(cfg, 6, 77))], chunk=4) == 6
    step("c0", [0, 1])
    assert s.hold(2, False) == 0
    for k in range(3):
        step(f"d{k}", [0, 1, 2])
    blob = s.save(1)
    put(name + ".blob1", blob)
    assert s.close(1) == 0 and s.fork(2, 1) == 0            # slot 1 becomes a fork of slot 2
    for k in range(3):
        step(f"e{k}", [0, 1, 2])
    put(name + ".blob1_fork", s.save(1))
    assert s.close(0) == 0 and s.load(0, blob) == 0         # slot 0 continues what slot 1 was
    for k in range(4):
        step(f"f{k}", [0, 1, 2])
    for b in range(3):
        put(f"{name}.blob{b}_end", s.save(b))
        put(f"{name}.position{b}", np.array(s.position(b)))
    put_graphs(name, s.m)
    s.free()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--kind", default="oracle", choices=["oracle", "hip"])
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    for sampled in (False, True):
        serial(args.kind, sampled)
    for model in ("tiny", "personaplex"):
        run_ahead(args.kind, model)
        prefill(args.kind, model)
    lockstep(args.kind)
    for sampled in (False, True):
        slots(args.kind, sampled)
    with open(args.out, "w") as f:
        f.write("\n".join(LINES) + "\n")
    print(f"wrote {args.out}: {len(LINES)} lines, sha256 {hashlib.sha256(open(args.out, 'rb').read()).hexdigest()}")
