"""CPU (oracle): replay on tts-shaped slots. moshi_hot_slots_replay / moshi_hot_slot_replay push a history - the frames a conversation committed, as
moshi_hot_slot_last_raw logs them - through the Temporal stack as batched [dim, T] passes with each job's own conditions; afterwards the slot is the
fresh single-stream model with those conditions that was stepped over the same frames with moshi_hot_force_last after each: the live frames that
follow are that model's bit for bit (status, tokens, text logits, transformer_out, every Depth step's logits), for every chunking, any number of jobs
per pass, past the ring's end, greedy and seeded."""
import functools

import numpy as np
import pytest

import ggml_util as gu
import hot_util as hu
import sampling_util as sp
import slots_util as sl
import streams_util as su
import tts_replay_util as ru
import tts_slots_util as tu

L = hu.L
N = 12                     # frames of a conversation: past delay_steps (2) + max(delays) (2)
CUT = 7                    # frames 0 .. 6 are the history, 7 .. 11 run live
SEED = 5
KEEP = tu.KEEP


def cfg_of(linear_type=gu.F32, embed_type=gu.F32, context=24, **off):
    cfg = tu.tts_cfg(linear_type=linear_type, embed_type=embed_type, layers=1)
    cfg.context = context
    for field in off:
        setattr(cfg, field, 0)
    if not cfg.dep_schedule_len:
        cfg.dep_context = cfg.dep_q     # (tiny_tts sizes the Depth ring by the schedule's length)
    return cfg


@functools.lru_cache(maxsize=None)
def logged(linear_type, embed_type, cond_seed, text_b, n=N, context=24, off=()):
    """the single-stream conversation (conditions cond_seed, text stream text_b), every frame's committed tokens logged"""
    cfg = cfg_of(linear_type, embed_type, context, **{f: 0 for f in off})
    return ru.single_reference("oracle", cfg, cond_seed, texts_of(cfg, text_b, n), seed=SEED)


def texts_of(cfg, text_b, n):
    if cfg.demux_second_stream:
        return tu.text_stream(cfg, text_b, n)
    return [7 + i + text_b for i in range(n)]     # (no demux: a plain text token)


def live(s, b, texts, first, depth=True):
    """slot b alone runs frames first .. of its text stream; every other slot is fed KEEP"""
    out = []
    for t in texts[first:]:
        text_in = [KEEP] * s.B
        text_in[b] = t
        out.append(ru.step(s, text_in, depth))
    return out


def replayed_then_live(cfg, cond_seed, texts, hist, chunk, b=1, B=2):
    s = ru.Slots("oracle", cfg, B, seed=SEED)
    assert s.set_conditions(b, cond_seed) == 0 and s.open(b) == 0
    assert s.replay_one(b, hist, chunk) == len(hist)
    assert s.position(b) == len(hist)
    got = live(s, b, texts, len(hist))
    s.free()
    return got


@pytest.mark.parametrize("chunk", [64, 3, 1])
def test_logged_history_round_trips(chunk):
    cfg = cfg_of()
    ref, raw = logged(gu.F32, gu.F32, 4, 0)
    assert any(r[0] for r in ref[CUT:]) and any(-1 in fr for fr in raw[:CUT]) and not any(-1 in fr for fr in raw[CUT - 1:])
    got = replayed_then_live(cfg, 4, texts_of(cfg, 0, N), raw[:CUT], chunk)
    tu.assert_column_equals_single(ru.column(got, 1), 1, ref[CUT:], f"round trip, chunk {chunk}")


def test_logged_history_round_trips_quantised():
    cfg = cfg_of(gu.Q4_K, gu.Q4_0)
    ref, raw = logged(gu.Q4_K, gu.Q4_0, 4, 0)
    got = replayed_then_live(cfg, 4, texts_of(cfg, 0, N), raw[:CUT], 3)
    tu.assert_column_equals_single(ru.column(got, 1), 1, ref[CUT:], "round trip q4_k")


@functools.lru_cache(maxsize=None)
def forced_reference(cond_seed, text_b, hist_seed, n_hist, n=N, context=24, live_before=0):
    """single-stream: live_before frames by the text hook, then n_hist frames forced to history(hist_seed), then live frames up to n"""
    cfg = cfg_of(context=context)
    hist = ru.history(cfg, n_hist, hist_seed)
    forced = {live_before + i: fr for i, fr in enumerate(hist)}
    out, raw = ru.single_reference("oracle", cfg, cond_seed, texts_of(cfg, text_b, n), forced=forced, seed=SEED)
    return out, raw, hist


def test_forced_prefix_equals_force_last_after_every_frame():
    cfg = cfg_of()
    ref, _, hist = forced_reference(4, 0, 11, CUT)
    assert all(-1 not in fr for fr in hist[:cfg.delay_steps])     # tokens the -1 rules would never have written
    for chunk in (64, 2):
        got = replayed_then_live(cfg, 4, texts_of(cfg, 0, N), hist, chunk)
        tu.assert_column_equals_single(ru.column(got, 1), 1, ref[CUT:], f"forced prefix, chunk {chunk}")


JOBS = [(2, 13, 4, 0, 21), (0, 6, 5, 1, 22), (3, 1, 6, 2, 23)]     # (slot, history frames, conditions, text stream, history seed)
N_JOBS_LIVE = 5


def run_jobs(one_call):
    cfg = cfg_of()
    s = ru.Slots("oracle", cfg, 4, seed=SEED)
    jobs = []
    for b, nh, cond, tb, hs in JOBS:
        assert s.set_conditions(b, cond) == 0 and s.open(b) == 0
        jobs.append((b, ru.history(cfg, nh, hs)))
    if one_call:
        assert s.replay(jobs, 8) == 20
    else:
        for b, h in jobs:
            assert s.replay([(b, h)], 8) == len(h)
    out = []
    for k in range(N_JOBS_LIVE):
        text_in = [KEEP] * 4
        for b, nh, cond, tb, hs in JOBS:
            text_in[b] = texts_of(cfg, tb, nh + N_JOBS_LIVE)[nh + k]
        out.append(ru.step(s, text_in))
    s.free()
    return out


def test_several_jobs_in_one_call():
    cfg = cfg_of()
    got = run_jobs(True)
    for b, nh, cond, tb, hs in JOBS:
        ref, _, _ = forced_reference(cond, tb, hs, nh, n=nh + N_JOBS_LIVE)
        frames = ru.column(got, b)
        tu.assert_column_equals_single(frames, b, ref[nh:], f"job of slot {b}")
    ru.same_frames(got, run_jobs(False), [b for b, *_ in JOBS], "one call against one call per job")


@pytest.mark.parametrize("chunk", [64, 5, 3, 1])
def test_past_the_rings_end(chunk):
    cfg = cfg_of(context=8)
    n0, n1, before = 19, 5, 8       # slot 0: a history of 19 frames from position 0; slot 1: 8 live frames, then 5 history frames from position 8
    n_live = 4
    ref0, _, h0 = forced_reference(4, 0, 31, n0, n=n0 + n_live, context=8)
    ref1, _, h1 = forced_reference(5, 1, 32, n1, n=before + n1 + n_live, context=8, live_before=before)
    t0, t1 = texts_of(cfg, 0, n0 + n_live), texts_of(cfg, 1, before + n1 + n_live)
    s = ru.Slots("oracle", cfg, 2, seed=SEED)
    assert s.set_conditions(0, 4) == 0 and s.set_conditions(1, 5) == 0 and s.open(1) == 0
    first = [ru.step(s, [KEEP, t1[i]], i >= cfg.delay_steps) for i in range(before)]
    tu.assert_column_equals_single(ru.column(first, 1), 1, ref1[:before], "live before the replay")
    assert s.position(1) == 8 and s.open(0) == 0
    assert s.replay([(0, h0), (1, h1)], chunk) == n0 + n1
    assert s.position(0) == n0 and s.position(1) == before + n1
    got = [ru.step(s, [t0[n0 + k], t1[before + n1 + k]]) for k in range(n_live)]
    s.free()
    tu.assert_column_equals_single(ru.column(got, 0), 0, ref0[n0:], f"19 frames round a ring of 8, chunk {chunk}")
    tu.assert_column_equals_single(ru.column(got, 1), 1, ref1[before + n1:], f"a job from position 8, chunk {chunk}")


def test_replay_leaves_live_neighbours_alone_and_works_on_a_held_slot():
    cfg = cfg_of()
    n, nh, start = 10, 13, 4        # slot 1's history is in place before frame 4, from which it lives
    hist = ru.history(cfg, nh, 41)
    t0, t1 = texts_of(cfg, 0, n), texts_of(cfg, 1, nh + n)

    def run(mode):
        """slot 0 lives through n frames; slot 1: "none", "call" (one replay call before frame 4) or "held" (opened and held before frame 1, one pass
        of 4 rows before each of the frames 1 .. 4, then released)"""
        s = ru.Slots("oracle", cfg, 3, seed=SEED)
        assert s.set_conditions(0, 4) == 0 and s.set_conditions(1, 5) == 0 and s.open(0) == 0
        out, done = [], 0
        for i in range(n):
            if mode == "call" and i == start:
                assert s.open(1) == 0 and s.replay_one(1, hist, 4) == nh
                done = nh
            if mode == "held" and i == 1:
                assert s.open(1) == 0 and s.hold(1, True) == 0
            if mode == "held" and 1 <= i <= start:
                k = min(4, nh - done)
                assert s.replay_one(1, hist[done:done + k], 4) == k
                done += k
                if i == start:
                    assert done == nh and s.hold(1, False) == 0
            text_in = [t0[i], t1[nh + i - start] if done == nh else KEEP, KEEP]
            out.append(ru.step(s, text_in, i >= cfg.delay_steps))
        s.free()
        return out
    base, call, held = run("none"), run("call"), run("held")
    ru.same_frames(base, call, [0], "a live neighbour, with and without a replay between its frames")
    ru.same_frames(base, held, [0], "a live neighbour beside a held slot replayed pass by pass")
    assert [f[1][1] for f in held[:start]] == [-1, -2, -2, -2]
    ru.same_frames(call[start:], held[start:], [1], "a held slot replayed one pass at a time against one call")
    ref, _, _ = forced_reference(5, 1, 41, nh, n=nh + n - start)
    tu.assert_column_equals_single(ru.column(call[start:], 1), 1, ref[nh:], "one call")


def test_last_raw_logged_and_replayed_continues_identically():
    cfg = cfg_of()
    n_log, n_more = 10, 4
    texts = texts_of(cfg, 0, n_log + n_more)
    s = ru.Slots("oracle", cfg, 3, seed=SEED)
    assert s.last_raw(0) is None
    assert s.set_conditions(0, 4) == 0 and s.set_conditions(2, 4) == 0 and s.open(0) == 0
    assert s.last_raw(0) is None                     # open, no frame yet
    log = []
    for i in range(n_log):
        ru.step(s, [texts[i], KEEP, KEEP], i >= cfg.delay_steps)
        log.append(s.last_raw(0))
    _, raw = logged(gu.F32, gu.F32, 4, 0, n_log + n_more)
    assert log == raw[:n_log]                        # what the single-stream model's moshi_hot_last_raw_tokens logs
    assert log[0][0] == texts[0] and log[0][1:] == [-1] * cfg.dep_q and -1 not in log[-1]
    assert s.open(2) == 0 and s.replay_one(2, log, 0) == n_log
    assert s.last_raw(2) == log[-1] and s.last_raw(1) is None and s.last_raw(3) is None and s.last_raw(-1) is None
    got = [ru.step(s, [texts[n_log + k], KEEP, texts[n_log + k]]) for k in range(n_more)]
    s.free()
    assert any(f[1][0] == 1 for f in got)
    for k, f in enumerate(got):
        assert f[1][0] == f[1][2] and f[2][0] == f[2][2] and f[3][0] == f[3][2], k
        for name, v in f[4].items():
            assert np.array_equal(v[0], v[2]), (k, name)


CONV = (77, 0.8, 0.7, 20, 25)     # seed, temp, temp_text, top_k, top_k_text


def test_seeded_conversation_continues_with_the_single_stream_models_tokens():
    """The single-stream model takes a seed only with every tts flag off (moshi_hot_set_sampling refuses the tts branches on it): on that tts-shaped
    configuration it is the reference. With the flags on, the reference is the same seeded conversation stepped live in another column and model."""
    n = N
    plain = sp.sampled(cfg_of(cross_attention=0, condition_sum=0, demux_second_stream=0, depformer_low_rank=0, dep_schedule_len=0, delay_steps=0), *CONV[1:])
    texts = [KEEP if i % 3 == 2 else t for i, t in enumerate(texts_of(plain, 0, n))]
    ref, raw = ru.single_reference("oracle", plain, None, texts, seed=SEED, sampling=CONV)
    s = ru.Slots("oracle", plain, 2, seed=SEED)
    assert s.set_sampling(1, *CONV) == 0 and s.open(1) == 0 and s.replay_one(1, raw[:CUT], 3) == CUT
    got = live(s, 1, texts, CUT)
    s.free()
    assert any(r[0] for r in ref[CUT:]) and len({tuple(r[2]) for r in ref if r[0]}) > 1
    tu.assert_column_equals_single(ru.column(got, 1), 1, ref[CUT:], "seeded, tts shape without the branches")

    cfg = sp.sampled(cfg_of(), *CONV[1:])
    full = hu.Model("oracle", cfg, seed=SEED)
    assert hu.hot.set_sampling(L, full.m, 0, *CONV) == -1
    full.free()
    texts = [KEEP if i % 3 == 2 else t for i, t in enumerate(texts_of(cfg, 0, n))]
    a = ru.Slots("oracle", cfg, 2, seed=SEED)
    assert a.set_conditions(0, 4) == 0 and a.set_sampling(0, *CONV) == 0 and a.open(0) == 0
    lived, log = [], []
    for i in range(n):
        lived.append(ru.step(a, [texts[i], KEEP], i >= cfg.delay_steps))
        log.append(a.last_raw(0))
    a.free()
    b = ru.Slots("oracle", cfg, 3, seed=SEED)
    assert b.set_conditions(2, 4) == 0 and b.set_sampling(2, *CONV) == 0 and b.set_sampling(0, 1000, 0.9, 0.6, 12, 17) == 0 and b.open(2) == 0
    assert b.replay_one(2, log[:CUT], 0) == CUT
    got = live(b, 2, texts, CUT)
    b.free()
    assert any(f[1][0] == 1 for f in lived[CUT:])
    for k, (g, r) in enumerate(zip(got, lived[CUT:])):
        assert g[1][2] == r[1][0] and g[2][2] == r[2][0] and g[3][2] == r[3][0], k
        for name in g[4]:
            assert np.array_equal(g[4][name][2], r[4][name][0]), (k, name)


@pytest.mark.parametrize("field", ["cross_attention", "condition_sum", "demux_second_stream", "depformer_low_rank", "dep_schedule_len", "delay_steps"])
def test_each_tts_flag_off(field):
    cfg = cfg_of(**{field: 0})
    ref, raw = logged(gu.F32, gu.F32, 4, 0, off=(field,))
    got = replayed_then_live(cfg, 4, texts_of(cfg, 0, N), raw[:CUT], 3)
    tu.assert_column_equals_single(ru.column(got, 1), 1, ref[CUT:], f"{field} = 0")


def _replay_refused(s, cfg, b=0):
    toks = np.zeros((2, cfg.n_q + 1), np.int32).tolist()
    return s.replay_one(b, toks, 0) == -1 and s.replay([(b, toks)], 0) == -1


def test_refusals():
    class Moshika(ru.Slots, sl.Slots):
        step = sl.Slots.step
    # moshika- and stt-shaped slots: the call is for the tts shape alone (they have moshi_hot_slots_prefill), and nothing changes
    for cfg in (su.lm_only(hu.hot.tiny(L, layers=1)), hu.hot.tiny_stt(L, layers=1)):
        s = Moshika("oracle", cfg, 2)
        assert s.open(0) == 0 and _replay_refused(s, cfg) and s.position(0) == 0
        s.free()
    cfg = cfg_of()
    hist = ru.history(cfg, 3, 1)
    # lockstep streams and a single-stream model
    st = tu.Streams("oracle", cfg, 2, seed=SEED)
    buf = np.array(hist, np.int32).reshape(-1)
    assert L.moshi_hot_slot_replay(st.m, 0, buf.ctypes.data, 3, 0) == -1 and L.moshi_hot_slot_last_raw(st.m, 0, buf.ctypes.data) == -1
    st.free()
    m = hu.Model("oracle", cfg)
    assert L.moshi_hot_slot_replay(m.m, 0, buf.ctypes.data, 3, 0) == -1 and L.moshi_hot_slot_last_raw(m.m, 0, buf.ctypes.data) == -1
    m.free()
    s = ru.Slots("oracle", cfg, 3, seed=SEED)
    assert s.set_conditions(0, 4) == 0 and s.open(0) == 0 and s.open(2) == 0
    assert s.replay_one(1, hist, 0) == -1                              # closed
    assert s.replay_one(-1, hist, 0) == -1 and s.replay_one(3, hist, 0) == -1
    assert s.replay([(0, hist), (0, hist)], 0) == -1                   # named twice
    assert s.replay([(0, hist), (1, hist)], 0) == -1                   # one bad job refuses the call
    assert s.replay([(0, hist), (2, hist), (0, hist), (2, hist)], 0) == -1   # n_jobs > B
    assert s.position(0) == 0 and s.position(2) == 0 and s.last_raw(0) is None
    assert s.replay_one(0, [], 0) == 0 and s.replay([], 0) == 0 and s.position(0) == 0
    # after the refusals the slot is the fresh conversation it was; the prefill calls still refuse the shape
    assert s.prefill_one(0, hist, 0) == -1
    texts = texts_of(cfg, 0, 6)
    got = [ru.step(s, [texts[i], KEEP, KEEP], i >= cfg.delay_steps) for i in range(6)]
    s.free()
    ref, _ = logged(gu.F32, gu.F32, 4, 0, 6)
    tu.assert_column_equals_single(ru.column(got, 0), 0, ref, "after refusals")
