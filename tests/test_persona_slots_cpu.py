"""CPU: PersonaPlex streams and slots (persona_columns = 1) on the host device with the oracle attached. Every column of a B-column model is a
single-stream PersonaPlex model fed that column's codes - tokens and text logits bit for bit - and a slot that took its persona (voice rows, ring
image, silence, text prompt, silence) in batched [dim, T] passes is afterwards the single-stream model that stepped the same rows one by one
(moshi_hot_lm_step_embedding, moshi_hot_set_host_ring, moshi_hot_personaplex_system_prompts), for every chunking and with several jobs per pass."""
import ctypes as C
import functools
import struct

import numpy as np
import pytest

import hot_util as hu
import persona_util as pp
import sampling_util as sp
import slots_util as sl
from ggml_util import BF16, F16, F32

L = hu.L
N_LIVE = 10
SAMPLING = (4321, 0.9, 0.6, 12, 17)


def cfg1():
    return pp.make_cfg(layers=1)


def persona(which):
    """A: F32 voice with a ring image; B: BF16 voice without one; C: the tool's 6 silence frames (17 rows, F16); D: no image (for a slot that has stepped)"""
    c = cfg1()
    return {"A": pp.Persona(c, 11, vtype=F32, cache=True), "B": pp.Persona(c, 12, vtype=BF16, cache=False),
            "C": pp.Persona(c, 13, n_voice=3, vtype=F16, cache=True, n_text=2, silence=6), "D": pp.Persona(c, 14, vtype=BF16, cache=False)}[which]


def live(which, n=N_LIVE):
    return pp.live_codes(cfg1(), n, seed=70 + ord(which))


@functools.lru_cache(maxsize=None)
def reference(which, n_before=0):
    """the single-stream model of persona `which` (None: no persona), shared by the tests and never changed"""
    before = live("x", n_before) if n_before else ()
    return pp.single_reference("oracle", cfg1(), persona(which) if which else None, live(which or "n"), before=before, seed=5)


def blob_state(cfg, blob):
    """(frames, position, delay ring [rows, n_q + 1], transformer_out) of a snapshot blob (include/moshi_hot.h: the header is 88 bytes)"""
    frames, pos = struct.unpack_from("<qq", blob, 24)
    rows, cols = struct.unpack_from("<ii", blob, 48)
    ring = np.frombuffer(blob, np.int32, rows * cols, 88).reshape(rows, cols)
    tout = np.frombuffer(blob, np.float32, cfg.dim, 88 + rows * cols * 4)
    return frames, pos, ring, tout


def assert_state_equals_single(s, b, ref, what=""):
    frames, pos, ring, tout = blob_state(s.cfg, s.save(b))
    assert frames == ref[3] and pos == ref[3] == s.position(b), (what, frames, pos, ref[3])
    assert np.array_equal(ring, ref[1]), (what, ring, ref[1])
    assert np.array_equal(tout, ref[2]), what


# ---- admission ---------------------------------------------------------------------------------------------------------------------------------
def test_admission_is_opt_in_and_personaplex_only():
    for create in ("moshi_hot_create_streams", "moshi_hot_create_slots"):
        assert not pp.created(create, pp.make_cfg(persona_columns=0), 2), create
        assert pp.created(create, cfg1(), 2) and pp.created(create, cfg1(), 16), create
        assert not pp.created(create, cfg1(), 17), create
        moshika = sl.lm_only(hu.hot.tiny(L, layers=1))
        moshika.persona_columns = 1
        assert not pp.created(create, moshika, 2), create
        for field in ("chain_depth", "codec_stream", "extra_heads", "tp_world", "enable_mimi_decoder", "enable_mimi_encoder",
                      "delay_steps", "condition_sum", "demux_second_stream", "depformer_low_rank"):
            c = cfg1()
            setattr(c, field, 1)
            assert not pp.created(create, c, 2), (create, field)
        c = cfg1()
        c.cross_attention, c.cross_len = 1, 4
        assert not pp.created(create, c, 2), create
    # a single-stream model ignores the flag
    a, b = pp.single_reference("oracle", pp.make_cfg(persona_columns=0), None, live("n", 4), seed=5), reference(None)
    assert all(x[:3] == y[:3] and np.array_equal(x[3], y[3]) for x, y in zip(a[0], b[0]))


# ---- lockstep streams and slots against the single-stream model ---------------------------------------------------------------------------------
def test_every_lockstep_column_is_a_single_stream_model():
    cfg, B, n = cfg1(), 3, 2 * 4 + 4                       # the delay ring has 4 rows
    codes = [pp.live_codes(cfg, n, seed=30 + b) for b in range(B)]
    singles = [pp.single_reference("oracle", cfg, None, codes[b], seed=5)[0] for b in range(B)]
    s = pp.Streams("oracle", cfg, B, seed=5)
    for k in range(n):
        r, txt, aud = s.step([codes[b][k] for b in range(B)])
        logits = s.read("text_logits", cfg.text_card)
        assert r == int(all(singles[b][k][0] for b in range(B))), k
        for b in range(B):
            ok, t1, a1, l1 = singles[b][k]
            assert np.array_equal(logits[b], l1), (k, b)
            if k >= 1:                                      # the delay rings are full: the outputs are written (lm.h:950)
                assert txt[b] == t1 and aud[b] == a1 and len(aud[b]) == 8, (k, b)
    s.free()
    assert any(x[0] for x in singles[0])


def test_slots_opened_in_different_frames_and_reopened():
    cfg, B, n = cfg1(), 3, 14
    codes = {b: pp.live_codes(cfg, n, seed=40 + b) for b in range(B)}
    opened = {0: 0, 1: 3, 2: 1}                            # slot -> the frame it opens in; slot 2 closes in frame 6 and reopens in frame 8
    s = pp.Slots("oracle", cfg, B, seed=5)
    got = {0: [], 1: [], 2: [], "2b": []}
    for k in range(n):
        for b, f in opened.items():
            if f == k:
                assert s.open(b) == 0
        if k == 6:
            assert s.close(2) == 0
        if k == 8:
            assert s.open(2) == 0
        per, key = {}, {}
        for b in range(B):
            if k >= opened[b] and not (b == 2 and 6 <= k < 8):
                key[b] = "2b" if b == 2 and k >= 8 else b
                per[b] = codes[b][len(got[key[b]])] if key[b] != "2b" else codes[0][len(got["2b"])]
        r = s.step_some(per)
        assert [st == -1 for st in r[1]] == [b not in per for b in range(B)], k
        for b in per:
            got[key[b]].append(r)
    s.free()
    for kk, b, cs in ((0, 0, codes[0]), (1, 1, codes[1]), (2, 2, codes[2]), ("2b", 2, codes[0])):
        ref = pp.single_reference("oracle", cfg, None, cs[:len(got[kk])], seed=5)[0]
        pp.assert_slot_equals_single(got[kk], b, ref, f"conversation {kk}")


# ---- persona admission -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", [0, 3, 7])
def test_two_personas_in_one_call_equal_the_single_stream_sequences(chunk):
    # 12 + 12 rows: chunk 3 cuts voice | voice + silence | ... with pieces of one kind and of both; chunk 7 puts the end of job 0 and the head of
    # job 1 into one pass (token rows, then voice rows); chunk 0 is one pass of 24 rows: voice | tokens | voice | tokens
    s = pp.Slots("oracle", cfg1(), 3, seed=5)
    A, Bp = persona("A"), persona("B")
    assert s.open(0) == 0 and s.open(2) == 0
    assert s.persona([(0, A), (2, Bp)], chunk) == A.rows + Bp.rows == 24
    assert s.position(1) == -1
    assert_state_equals_single(s, 0, reference("A"), f"A, chunk {chunk}")
    assert_state_equals_single(s, 2, reference("B"), f"B, chunk {chunk}")
    got = [s.step_some({0: live("A")[k], 2: live("B")[k]}) for k in range(N_LIVE)]
    s.free()
    pp.assert_slot_equals_single(got, 0, reference("A")[0], f"A, chunk {chunk}")
    pp.assert_slot_equals_single(got, 2, reference("B")[0], f"B, chunk {chunk}")
    assert any(g[1][0] == 1 for g in got) and len({g[2][0] for g in got}) > 1


def test_the_tools_silence_and_a_slot_that_has_already_stepped():
    # C: 3 voice rows + 6 + 2 + 6 = 17 rows against moshi_hot_personaplex_system_prompts itself; D: 4 live frames, then 12 rows, no ring image
    s = pp.Slots("oracle", cfg1(), 2, seed=5)
    Cp, D = persona("C"), persona("D")
    assert s.open(0) == 0
    for fr in live("x", 4):
        s.step_some({0: fr})
    assert s.open(1) == 0
    assert s.persona([(1, Cp), (0, D)], 5) == 17 + 12
    assert_state_equals_single(s, 1, reference("C"), "C")
    assert_state_equals_single(s, 0, reference("D", 4), "D")
    assert s.last_raw(0) == reference("D", 4)[1][reference("D", 4)[3] % 4].tolist()
    got = [s.step_some({1: live("C")[k], 0: live("D")[k]}) for k in range(N_LIVE)]
    s.free()
    pp.assert_slot_equals_single(got, 1, reference("C")[0], "C")
    pp.assert_slot_equals_single(got, 0, reference("D", 4)[0], "D")


def test_one_call_per_job_and_a_held_slot_between_calls():
    s = pp.Slots("oracle", cfg1(), 3, seed=5)
    A = persona("A")
    assert s.open(0) == 0 and s.open(1) == 0 and s.hold(0, 1) == 0
    # the persona in two calls around a live frame of the neighbour: voice rows + ring image, then the prompt frames
    head = pp.Persona(s.cfg, 11, vtype=F32, cache=False, n_text=0, silence=0)
    head.cache = A.cache
    tail = pp.Persona(s.cfg, 11, n_voice=0, cache=False)
    tail.text = A.text
    assert np.array_equal(head.voice_f32, A.voice_f32)
    assert s.persona_one(0, head, 2) == 5
    r = s.step_some({1: live("n")[0]})
    assert r[1][0] == -2 and s.position(0) == 5
    assert s.persona_one(0, tail, 4) == 7 and s.hold(0, 0) == 0
    assert_state_equals_single(s, 0, reference("A"), "A in two calls")
    got = [s.step_some({0: live("A")[k], 1: live("n")[1 + k]}) for k in range(N_LIVE - 1)]
    s.free()
    pp.assert_slot_equals_single(got, 0, reference("A")[0][:N_LIVE - 1], "A in two calls")
    pp.assert_slot_equals_single([r] + got, 1, reference(None)[0], "the neighbour")


def test_live_neighbour_is_untouched_by_an_admission_between_its_frames():
    runs = []
    for admit in (False, True):
        s = pp.Slots("oracle", cfg1(), 3, seed=5)
        assert s.open(1) == 0
        got = []
        for k in range(N_LIVE):
            if admit and k == 3:
                assert s.open(0) == 0 and s.open(2) == 0
                assert s.persona([(0, persona("A")), (2, persona("B"))], 7) == 24
                assert s.close(0) == 0 and s.close(2) == 0
            got.append(s.step_some({1: live("n")[k]}))
        s.free()
        runs.append(got)
    for got in runs:
        pp.assert_slot_equals_single(got, 1, reference(None)[0])
    assert any(g[1][1] == 1 for g in runs[0])


def test_refused_calls_change_nothing():
    cfg = cfg1()
    A, Bp = persona("A"), persona("B")
    s = pp.Slots("oracle", cfg, 3, seed=5)
    assert s.open(0) == 0
    before = s.save(0)
    long_one = pp.Persona(cfg, 1, n_voice=20, n_text=3, silence=2)                 # 27 rows > the ring's 24
    assert s.persona_one(0, long_one) == -1
    assert s.persona([(0, A), (1, Bp)]) == -1                                       # slot 1 is closed
    assert s.persona([(0, A), (0, Bp)]) == -1                                       # named twice
    assert s.persona([(0, A), (3, Bp)]) == -1 and s.persona_one(-1, A) == -1        # bad indices
    assert s.persona([(0, A), (1, A), (2, A), (0, A)]) == -1                        # more jobs than slots
    bad = pp.Persona(cfg, 1)
    bad.vtype = 12                                                                  # a voice that is no F32 / BF16 / F16 tensor
    assert s.persona_one(0, bad) == -1
    neg = pp.Persona(cfg, 1)
    neg.silence = -1
    assert s.persona_one(0, neg) == -1
    assert s.persona([]) == 0
    assert np.array_equal(s.save(0), before) and s.position(0) == 0
    assert s.persona_one(0, A, 7) == A.rows
    got = [s.step_some({0: live("A")[k]}) for k in range(N_LIVE)]
    s.free()
    pp.assert_slot_equals_single(got, 0, reference("A")[0], "after refusals")
    # a slot at position 14: 14 + 12 rows pass the ring's end
    s = pp.Slots("oracle", cfg, 2, seed=5)
    assert s.open(0) == 0
    s.set_fill(0, 14)
    assert s.persona_one(0, A) == -1 and s.position(0) == 14
    s.free()
    # other model kinds: a moshika-shaped slots model, PersonaPlex lockstep streams, a single-stream model
    st, keep = A.struct()
    sb = (C.c_int32 * 1)(0)
    mk = sp.Slots("oracle", sl.lm_only(hu.hot.tiny(L, layers=1)), 2, seed=5)
    assert mk.open(0) == 0 and L.moshi_hot_slots_persona(mk.m, 1, sb, C.byref(st), 0) == -1 and mk.position(0) == 0
    mk.free()
    ls = pp.Streams("oracle", cfg, 2, seed=5)
    assert L.moshi_hot_slot_persona(ls.m, 0, C.byref(st), 0) == -1
    flat = np.zeros(4 * 17, np.int32)
    assert L.moshi_hot_set_host_ring(ls.m, flat.ctypes.data, flat.size) == -1
    ls.free()
    m = hu.Model("oracle", cfg, seed=5)
    assert L.moshi_hot_slot_persona(m.m, 0, C.byref(st), 0) == -1 and L.moshi_hot_offset(m.m) == 0
    assert L.moshi_hot_set_host_ring(m.m, flat.ctypes.data, flat.size - 1) == -1
    m.free()


# ---- sampling and snapshots ------------------------------------------------------------------------------------------------------------------------
def test_a_seeded_persona_conversation_is_the_same_in_any_column():
    cfg = sp.sampled(cfg1())
    A = persona("A")
    runs = []
    for B, b in ((2, 0), (3, 2)):
        s = pp.Slots("oracle", cfg, B, seed=5)
        assert s.set_sampling(b, *SAMPLING) == 0 and s.open(b) == 0
        if B == 3:
            assert s.open(0) == 0                          # an unseeded live neighbour
        assert s.persona_one(b, A, 5) == A.rows
        frames = [s.step_some({b: fr, 0: fr} if B == 3 else {b: fr}) for fr in live("A", 12)]
        runs.append([(f[1][b], f[2][b], f[3][b]) for f in frames])
        s.free()
    assert runs[0] == runs[1]
    assert any(st == 1 for st, _, _ in runs[0])


def test_snapshot_after_admission_continues_in_another_model():
    cfg = cfg1()
    A = persona("A")
    a = pp.Slots("oracle", cfg, 3, seed=5)
    assert a.open(2) == 0 and a.persona_one(2, A, 0) == A.rows
    blob = a.save(2)
    b = pp.Slots("oracle", cfg, 2, seed=5)
    assert b.load(1, blob) == 0 and b.position(1) == A.rows
    got_a = [a.step_some({2: fr}) for fr in live("A")]
    got_b = [b.step_some({1: fr}) for fr in live("A")]
    pp.assert_slot_equals_single(got_a, 2, reference("A")[0], "the saved slot")
    pp.assert_slot_equals_single(got_b, 1, reference("A")[0], "the loaded slot")
    # a moshika-shaped blob is refused here, a PersonaPlex blob there; the replay / _full calls are the tts shape's
    mk = sp.Slots("oracle", sl.lm_only(hu.hot.tiny(L, layers=1)), 2, seed=5)
    assert mk.open(0) == 0
    n = L.moshi_hot_slot_save(mk.m, 0, None, 0)
    mblob = np.zeros(n, np.uint8)
    assert L.moshi_hot_slot_save(mk.m, 0, mblob.ctypes.data, n) == n
    assert b.load(0, mblob) == -1 and b.position(0) == -1
    assert L.moshi_hot_slot_load(mk.m, 1, blob.ctypes.data, blob.nbytes) == -1 and mk.position(1) == -1
    assert L.moshi_hot_slot_fork(b.m, 1, 0) == 0 and b.position(0) == b.position(1)
    assert L.moshi_hot_slot_save_full(b.m, 1, None, 0) == L.moshi_hot_slot_save(b.m, 1, None, 0)   # not the tts shape: the plain calls
    frames = np.zeros(17, np.int32)
    fp = (C.c_void_p * 1)(frames.ctypes.data)
    assert L.moshi_hot_slots_replay(b.m, 1, (C.c_int32 * 1)(1), fp, (C.c_int32 * 1)(1), 0) == -1
    for x in (a, b, mk):
        x.free()
