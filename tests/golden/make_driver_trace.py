"""Generates tests/golden/driver_trace.npz: what the frame driver's integer protocol (the delay ring of moshi_lmgen_step, lm.h:715-743, 812-834,
930-964, and the header + ring part of a slot snapshot blob) leaves behind for fixed inputs. Every recorded value is a function of the inputs alone -
the model's own samples are overwritten (moshi_hot_force_last) or never enter (provided frames) - so the file holds on any machine and pins the ring
arithmetic and the blob's on-disk format. tests/test_driver_trace_cpu.py calls record() and compares exactly.

Run with the libraries built: `python tests/golden/make_driver_trace.py`.

Single-stream models (teacher-forced; 3 * (max_delay + 2) frames, so the ring wraps): per frame the step's return value, moshi_hot_offset, the ring
after the force and (where the text embedding is not demuxed) the ids the Temporal graph was fed.
  moshika      tiny moshika-shaped model; the other speaker's codes in, every sample forced, a -1 among the forced tokens now and then
  personaplex  moshi_hot_personaplex_system_prompts first, then the same (the Depth chain samples 16 codebooks, the protocol hands back 8)
  tts          delay_steps = 2, a text hook returning a fixed sequence (the offsets it was called with are recorded too)
Slots models (B = 3, ring of 24): slot 0 prefilled with 5 provided frames and slot 2 with max_delay + 3 in ONE call with chunk = 4 (the jobs share and
span passes), slot 1 closed; the bytes of moshi_hot_slot_save of slots 0 and 2 from the header through the end of the delay ring, and
moshi_hot_slot_position of every slot. Once greedy, once sampled with slot 0 seeded."""
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
PATH = os.path.join(HERE, "driver_trace.npz")
BLOB_HEADER = 88                             # sizeof(SlotBlobHeader); the ring follows as ring_rows x ring_cols int32
SAMPLING = (4321, 0.9, 0.6, 12, 17)          # seed, temp, temp_text, top_k, top_k_text of the seeded slot


def max_delay(cfg):
    return max(cfg.delays[i] for i in range(cfg.n_q + 1))


def fed_ids(m, cfg):
    """the ids of the n_q + 1 embeddings of the Temporal graph (negative ids go up as row 0)"""
    g = L.moshi_hot_graph(m.m, 0)
    ids = []
    for i in range(L.ggml_graph_n_nodes(g)):
        t = L.ggml_graph_node(g, i)
        if L.ggml_op_name(t.contents.op) == b"GET_ROWS" and len(ids) < cfg.n_q + 1:
            idx = np.zeros(1, np.int32)
            L.ggml_backend_tensor_get(t.contents.src[1], idx.ctypes.data, 0, 4)
            ids.append(int(idx[0]))
    return ids


def single(variant):
    """-> {"ret", "offset", "ring"[, "ids"][, "hook_offsets"]} of one teacher-forced single-stream run"""
    rng = np.random.default_rng({"moshika": 31, "personaplex": 32, "tts": 33}[variant])
    if variant == "moshika":
        cfg = hu.hot.tiny(L, layers=1)
    elif variant == "personaplex":
        cfg = hu.hot.tiny_personaplex(L, layers=1)
    else:
        cfg = hu.hot.tiny_tts(L, layers=1, linear_type=hu.pkg.F32, embed_type=hu.pkg.F32)
    su.lm_only(cfg)
    n_frames = 3 * (max_delay(cfg) + 2)
    n_in = cfg.n_q - cfg.io_dep_q
    m = hu.Model("oracle", cfg)
    hook_offsets = []
    if variant == "tts":
        hu.set_conditions(m, cfg)
        n = cfg.text_card + 1
        hooked = [int(rng.integers(0, 4)) * n + int(rng.integers(0, cfg.text_card)) for _ in range(n_frames)]   # demuxed (second + 1, first), lm.h:176-191
        hu.set_text_hook(m, lambda offset, sampled: (hook_offsets.append(offset), hooked[offset])[1])
    if variant == "personaplex":
        m.system_prompts([11, 12, 13])
    out = {"ret": [], "offset": [], "ring": [], "ids": []}
    for k in range(n_frames):
        r = m.lm_step_n(rng.integers(0, cfg.card, n_in).tolist())[0]
        if variant != "tts":
            out["ids"].append(fed_ids(m, cfg))
        text = int(rng.integers(0, cfg.text_card))
        audio = rng.integers(0, cfg.card, cfg.dep_q)
        if k % 4 == 2:
            audio[0 if k == 2 else k % cfg.dep_q] = -1   # every fourth frame carries a -1; frame 2's sits in a delay-0 column, where a later read-out meets it
        m.force_last(text, audio.tolist())
        out["ret"].append(r)
        out["offset"].append(L.moshi_hot_offset(m.m))
        out["ring"].append(m.host_ring().copy())
    m.free()
    if variant == "tts":
        del out["ids"]
        out["hook_offsets"] = hook_offsets
    return {k: np.array(v, np.int64 if k == "offset" else np.int32) for k, v in out.items()}


def slots(sampled):
    """-> {"blob0", "blob2", "positions"} of a prefilled B = 3 slots model"""
    cfg = su.lm_only(hu.hot.tiny(L, context=24))
    if sampled:
        cfg = sp.sampled(cfg)
    s = ss.Slots("oracle", cfg, 3, seed=5)
    if sampled:
        assert s.set_sampling(0, *SAMPLING) == 0
    assert s.open(0) == 0 and s.open(2) == 0
    n2 = max_delay(cfg) + 3
    assert s.prefill([(0, pu.history(cfg, 5, 41)), (2, pu.history(cfg, n2, 42))], chunk=4) == 5 + n2
    out = {"positions": np.array([s.position(b) for b in range(3)], np.int64)}
    for b in (0, 2):
        blob = s.save(b)
        ring_rows, ring_cols = blob[48:56].view(np.int32)            # after magic, version, fingerprint, total_bytes, frames, pos, n_rows
        assert ring_cols == cfg.n_q + 1
        out[f"blob{b}"] = blob[:BLOB_HEADER + int(ring_rows) * int(ring_cols) * 4].copy()
    s.free()
    return out


def record():
    out = {}
    for name, part in [(v, single(v)) for v in ("moshika", "personaplex", "tts")] + [("slots", slots(False)), ("slots_sampled", slots(True))]:
        for k, v in part.items():
            out[f"{name}.{k}"] = v
    return out


if __name__ == "__main__":
    np.savez_compressed(PATH, **record())
    print("wrote", PATH, os.path.getsize(PATH), "bytes")
