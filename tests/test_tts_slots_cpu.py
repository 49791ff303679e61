"""CPU (oracle): B text-to-speech conversations per frame step. A tts-shaped model (n_q == dep_q; cross-attention, condition sum, demuxed text,
low-rank Depth embeddings, a weight schedule, delay_steps) as lockstep streams and as slots: every column, with its own conditions
(moshi_hot_set_conditions_column) and its own text stream (moshi_hot_lm_step_*_text), is the single-stream model with those conditions and a text
hook returning those tokens, bit for bit."""
import ctypes as C
import functools

import numpy as np
import pytest

import hot_util as hu
import ggml_util as gu
import sampling_util as sp
import slots_util as sl
import streams_util as su
import tts_slots_util as tu

L = hu.L
N = 12                     # frames: past delay_steps (2) + max(delays) (2) and the delay ring's turn-over
SEED = 5


def cfg_of(linear_type=gu.F32, embed_type=gu.F32, layers=1):
    return tu.tts_cfg(linear_type=linear_type, embed_type=embed_type, layers=layers)


@functools.lru_cache(maxsize=None)
def reference(linear_type, embed_type, cond_seed, text_b, n=N, layers=1):
    cfg = cfg_of(linear_type, embed_type, layers)
    return tu.single_reference("oracle", cfg, cond_seed, tu.text_stream(cfg, text_b, n), seed=SEED)


def run_lockstep(cfg, B, n=N, cond=lambda b: 4 + b, text=lambda b: b, before=None):
    s = tu.Streams("oracle", cfg, B, seed=SEED)
    for b in range(B):
        if cond(b) is not None:
            assert s.set_conditions(b, cond(b)) == 0
    streams = [tu.text_stream(cfg, text(b), n) for b in range(B)]
    out = []
    for i in range(n):
        if before:
            before(s, i)
        r = s.step([streams[b][i] for b in range(B)])
        out.append(r + (tu.reads(s, cfg, i >= cfg.delay_steps),))
    s.free()
    return out


def check_lockstep(linear_type, embed_type, B):
    cfg = cfg_of(linear_type, embed_type)
    got = run_lockstep(cfg, B)
    assert any(g[0] == 1 for g in got)
    for b in range(B):
        tu.assert_column_equals_single(got, b, reference(linear_type, embed_type, 4 + b, b), f"lockstep B={B}")


@pytest.mark.parametrize("B", [2, 3])
def test_lockstep_columns_equal_single_stream_models(B):
    check_lockstep(gu.F32, gu.F32, B)


@pytest.mark.parametrize("linear_type", [gu.Q8_0, gu.Q4_K], ids=["q8_0", "q4_k"])
def test_lockstep_columns_equal_single_stream_models_quantised(linear_type):
    cfg = cfg_of(linear_type, gu.Q4_0)
    assert cfg.demux_second_stream and cfg.depformer_low_rank and cfg.dep_schedule_len and cfg.cross_attention and cfg.condition_sum
    check_lockstep(linear_type, gu.Q4_0, 2)


def test_staggered_slots_equal_single_stream_models():
    cfg = cfg_of()
    n, B = 17, 3
    # (slot, first frame, end frame, conditions, text stream): slot b opens at frame 2 b - one column sits inside delay_steps while another runs the
    # Depth graph; slot 0's first conversation ends at frame 9 and a second one with new conditions takes the slot over at frame 10
    convs = [(0, 0, 9, 4, 0), (1, 2, n, 5, 1), (2, 4, n, 6, 2), (0, 10, n, 9, 3)]
    s = tu.Slots("oracle", cfg, B, seed=SEED)
    frames = []
    for i in range(n):
        text_in = [tu.KEEP] * B
        for b, f0, f1, cond, tb in convs:
            if i == f0:
                assert s.set_conditions(b, cond) == 0 and s.open(b) == 0
            if i == f1:
                assert s.close(b) == 0
            if f0 <= i < f1:
                text_in[b] = tu.text_stream(cfg, tb, n)[i - f0]
        r = s.step(text_in)
        frames.append(r + (tu.reads(s, cfg, True),))
    s.free()
    lag = cfg.delay_steps + max(cfg.delays[i] for i in range(cfg.n_q + 1))
    for b, f0, f1, cond, tb in convs:
        ref = reference(gu.F32, gu.F32, cond, tb, n)[:f1 - f0]
        got = []
        for k, fr in enumerate(frames[f0:f1]):
            n_valid, status, texts, audios, rd = fr
            if k < cfg.delay_steps:   # a replaced column: nothing is read out, its Depth logits are not its conversation's
                assert status[b] == 0 and texts[b] == -1 and audios[b] == [-1] * cfg.dep_q, (b, k, status, audios[b])
                rd = {name: v for name, v in rd.items() if not name.startswith("dep_logits")}
            got.append((status[b], texts, audios, rd))
        for k, (g, r) in enumerate(zip(got, ref)):   # (the single-stream reference reads the Depth logits from frame delay_steps on)
            assert set(g[3]) == set(r[3]), (b, k)
        tu.assert_column_equals_single(got, b, ref, f"slots conversation of slot {b} from frame {f0}")
        valid = [k for k, g in enumerate(got) if g[0] == 1]
        assert valid and valid[0] >= lag and valid == list(range(valid[0], f1 - f0)), (b, valid)
    # a closed slot reports -1
    assert frames[9][1][0] == -1 and frames[0][1][1] == -1 and frames[3][1][2] == -1


def test_conditions_are_per_column():
    cfg = cfg_of()

    def change(s, i):
        if i == 3:
            assert s.set_conditions(1, 11) == 0
    base = run_lockstep(cfg, 2, n=6)
    changed = run_lockstep(cfg, 2, n=6, before=change)
    differs = False
    for k, (a, c) in enumerate(zip(base, changed)):
        assert a[0] == c[0] and a[1][0] == c[1][0] and a[2][0] == c[2][0], k
        for name in a[3]:
            assert np.array_equal(a[3][name][0], c[3][name][0]), (k, name)
        same = np.array_equal(a[3]["transformer_out"][1], c[3]["transformer_out"][1])
        assert same == (k < 3), k                  # it takes effect from the next step on
        differs = differs or not same
    assert differs
    # a column that was never set has zero conditions: a single-stream model before moshi_hot_set_conditions
    got = run_lockstep(cfg, 2, n=6, cond=lambda b: 4 if b == 0 else None)
    tu.assert_column_equals_single(got, 1, reference(gu.F32, gu.F32, None, 1, 6), "never set")
    tu.assert_column_equals_single(got, 0, reference(gu.F32, gu.F32, 4, 0, 6), "beside a column never set")


def test_text_keep_leaves_the_sampled_token():
    cfg = cfg_of()
    n = 6
    forced = tu.text_stream(cfg, 1, n)
    s = tu.Streams("oracle", cfg, 2, seed=SEED)
    assert s.set_conditions(0, 4) == 0 and s.set_conditions(1, 5) == 0
    got = []
    for i in range(n):
        r = s.step([tu.KEEP, forced[i]])
        got.append(r + (tu.reads(s, cfg, i >= cfg.delay_steps),))
    s.free()
    kept = tu.single_reference("oracle", cfg, 4, [tu.KEEP] * n, seed=SEED)
    # (column 0's sampled tokens stay below text_card: no right half; the neighbour's are demuxed pairs)
    for g, r in zip(got, kept):
        g_ok = g[0]
        assert np.array_equal(g[3]["text_logits"][0], r[3]["text_logits"]) and np.array_equal(g[3]["transformer_out"][0], r[3]["transformer_out"])
        if g_ok and r[0]:
            assert g[1][0] == r[1] and g[2][0] == r[2] and 0 <= g[1][0] < cfg.text_card
    ref1 = reference(gu.F32, gu.F32, 5, 1, n)
    for g, r in zip(got, ref1):
        assert np.array_equal(g[3]["text_logits"][1], r[3]["text_logits"])
        if g[0] and r[0]:
            assert g[1][1] == r[1] and g[2][1] == r[2]


def test_text_in_null_is_the_existing_call_on_the_moshika_shape():
    cfg = su.lm_only(hu.hot.tiny(L, layers=1))
    codes = su.stream_codes(cfg, 2, 30, seed=3)
    ref = su.run_streams("oracle", cfg, codes, seed=SEED, logits=True)
    s = tu.Streams("oracle", cfg, 2, seed=SEED)
    for k, fr in enumerate(codes):
        r = s.step(None, fr)
        assert r[0] == ref[k][0], k
        if r[0]:
            assert r[1:] == ref[k][1:3], k
        assert np.array_equal(s.read("text_logits", cfg.text_card), ref[k][3]), k
    s.free()
    events = {0: [("open", 0)], 3: [("open", 1)]}
    a = sl.Slots("oracle", cfg, 2, seed=SEED)
    ref = sl.run_slots(a, codes, events, logits=True)
    a.free()
    b = tu.Slots("oracle", cfg, 2, seed=SEED)
    for k, fr in enumerate(codes):
        for _, slot in events.get(k, []):
            assert b.open(slot) == 0
        r = b.step(None, fr)
        assert r == ref[k][:4], k
        assert np.array_equal(b.read("text_logits", cfg.text_card), ref[k][4]), k
    # a forced text token on the moshika shape reaches the delay ring: it is what the step hands back once the ring has turned over
    r = b.step([123, tu.KEEP], codes[0])
    r = b.step(None, codes[1])
    assert r[1][0] == 1 and r[2][0] == 123
    b.free()


def test_seeded_conversation_is_the_same_in_any_column():
    cfg = sp.sampled(cfg_of())
    n = 10
    conv = (77, 0.8, 0.7, 20, 25)
    texts = [tu.KEEP if i % 3 == 2 else t for i, t in enumerate(tu.text_stream(cfg, 0, n))]

    def run(B, col):
        s = tu.Streams("oracle", cfg, B, seed=SEED)
        for b in range(B):
            assert s.set_conditions(b, 4 if b == col else 20 + b + B) == 0
            assert s.set_sampling(b, *(conv if b == col else (1000 + b + B, 0.9, 0.6, 12, 17))) == 0
        out = []
        for i in range(n):
            other = tu.text_stream(cfg, 5 + B, n)[i]
            r = s.step([texts[i] if b == col else other for b in range(B)])
            out.append((r[0], r[1][col], r[2][col]))
        s.free()
        return out
    a, b = run(2, 0), run(3, 2)
    assert a == b
    assert any(ok for ok, _, _ in a)
    assert len({tuple(aud) for ok, _, aud in a if ok}) > 1


def _created(cfg, B, fn):
    be = hu.make_backend("oracle")
    m = getattr(L, fn)(be, C.byref(cfg), 0, B)
    if m:
        L.moshi_hot_free(m)
    L.ggml_backend_free(be)
    return bool(m)


def test_admission_and_refusals():
    for fn in ("moshi_hot_create_slots", "moshi_hot_create_streams"):
        assert _created(cfg_of(), 2, fn) and _created(cfg_of(), 16, fn)
        assert not _created(cfg_of(), 17, fn)
        # every tts flag alone, in any combination, on the tts shape
        for field in ("cross_attention", "condition_sum", "demux_second_stream", "depformer_low_rank", "dep_schedule_len", "delay_steps"):
            c = cfg_of(); setattr(c, field, 0)
            assert _created(c, 2, fn), field
        # each tts flag set alone on a moshika-shaped configuration stays refused
        for field, value in (("cross_attention", 1), ("condition_sum", 1), ("demux_second_stream", 1), ("depformer_low_rank", 128), ("dep_schedule_len", 3),
                             ("delay_steps", 1)):
            c = su.lm_only(hu.hot.tiny(L, layers=1)); setattr(c, field, value); c.cross_len = 5
            assert not _created(c, 2, fn), field
        for field in ("personaplex", "chain_depth", "codec_stream", "extra_heads", "tp_world", "enable_mimi_decoder"):
            c = cfg_of(); setattr(c, field, 1); c.extra_heads_dim = 6
            assert not _created(c, 2, fn), field
        c = cfg_of(); c.cross_len = 0
        assert not _created(c, 2, fn)
    cfg = cfg_of()
    cond = tu.conditions(cfg, 4)
    # set_conditions_column: a single-stream model, a bad column, a model without the condition
    m = hu.Model("oracle", cfg)
    assert hu.hot.set_conditions_column(L, m.m, 0, *cond) == -1
    m.free()
    s = tu.Slots("oracle", cfg, 2, seed=SEED)
    assert s.set_conditions(-1, 4) == -1 and s.set_conditions(2, 4) == -1
    assert hu.hot.set_conditions_column(L, s.m, 0, None, None) == 0 and hu.hot.set_conditions_column(L, s.m, 1, cond[0], None) == 0
    L.moshi_hot_set_conditions(s.m, cond[0].ctypes.data, cond[1].ctypes.data)      # the single-stream call does nothing on B > 1
    moshika = sl.Slots("oracle", su.lm_only(hu.hot.tiny(L, layers=1)), 2)
    assert hu.hot.set_conditions_column(L, moshika.m, 0, *cond) == -1 and hu.hot.set_conditions_column(L, moshika.m, 0, None, None) == -1
    moshika.free()
    nosum = cfg_of(); nosum.condition_sum = 0
    t = tu.Slots("oracle", nosum, 2)
    assert hu.hot.set_conditions_column(L, t.m, 0, cond[0], None) == -1 and hu.hot.set_conditions_column(L, t.m, 0, None, cond[1]) == 0
    t.free()
    # prefill and snapshots refuse a tts slots model, and its next step is what it would have been
    assert s.set_conditions(0, 4) == 0 and s.set_conditions(1, 5) == 0 and s.open(0) == 0 and s.open(1) == 0
    texts = [tu.text_stream(cfg, b, 6) for b in range(2)]
    got = []
    for i in range(6):
        if i == 4:
            toks = np.zeros((2, cfg.n_q + 1), np.int32)
            assert s.prefill_one(0, toks.tolist(), 0) == -1
            assert s.close(1) == 0 and s.fork(0, 1) == -1 and s.open(1) == 0 and s.close(1) == 0     # (a fresh conversation in slot 1 from here)
            assert s.save_size(0) == -1 and s.save(0) is None
            assert s.load(1, np.zeros(4096, np.uint8)) == -1
        r = s.step([texts[0][i], texts[1][i]])
        got.append((r[1][0], r[2], r[3], tu.reads(s, cfg, i >= cfg.delay_steps)))
    s.free()
    tu.assert_column_equals_single(got, 0, reference(gu.F32, gu.F32, 4, 0, 6), "after refusals")
