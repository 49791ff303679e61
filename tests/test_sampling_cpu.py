"""CPU: per-conversation sampling (moshi_hot_set_sampling) on the host device with the oracle attached. In sampled mode a seeded conversation gets,
in any column of any B-column model beside any neighbours, exactly the tokens of a fresh single-stream model configured and seeded alike; columns
that were never seeded keep their rand() draws; the noise source is the formula of include/moshi_hot.h."""
import ctypes as C

import numpy as np
import pytest

import hot_util as hu
import sampling_util as sp
import slots_util as sl
import streams_util as su

L = hu.L
libc = C.CDLL(None)


def tiny_sampled(**kw):
    return sp.sampled(su.lm_only(hu.hot.tiny(L)), **kw)


def check_conversations(cfg, codes, got, events, sampling, seed):
    """every conversation of `events` against a fresh single-stream oracle model with its slot's sampling, bit for bit (tokens and text logits)"""
    spans = sl.conversations(events, len(codes))
    texts = {}
    for b, convs in spans.items():
        for s, e in convs:
            ref = sp.run_single("oracle", cfg, sampling[b], [codes[k][b] for k in range(s, e)], seed=seed, logits=True)
            for k in range(s, e):
                g, r = got[k], ref[k - s]
                assert g[1][b] == r[0], (b, s, k)
                if r[0]:
                    assert g[2][b] == r[1] and g[3][b] == r[2], (b, s, k, g[2][b], r[1], g[3][b], r[2])
                    texts.setdefault((b, s), []).append(r[1])
                else:
                    assert g[2][b] == -1 and g[3][b] == [-1] * cfg.dep_q, (b, s, k)
                assert np.array_equal(g[4][b], r[3]), (b, s, k)
    return spans, texts


def test_seeded_slots_equal_fresh_seeded_single_stream_models():
    cfg = tiny_sampled()                                    # temp 0.8 / 0.7, top_k 20 / 25: the compiled maximum of every slot
    C_ = cfg.context
    n = C_ + 16
    B = 3
    #            seed   temp temp_text top_k top_k_text
    sampling = [(101, 0.8, 0.7, 20, 25), (0xDEADBEEFCAFE, 1.1, 0.5, 7, 25), (303, 0.6, 0.9, 20, 3)]
    # staggered opens, a close, and a reopen of slot 0 after its conversation ran past the 24-slot ring's wrap
    events = {0: [("open", 0)], 5: [("open", 1)], 11: [("open", 2)], 14: [("close", 1)], 17: [("open", 1)], C_ + 4: [("close", 0), ("open", 0)]}
    codes = sl.slot_codes(cfg, B, n, seed=11)
    s = sp.Slots("oracle", cfg, B, seed=5)
    for b in range(B):
        assert s.set_sampling(b, *sampling[b]) == 0
        assert s.get_sampling(b) == (sampling[b][0], np.float32(sampling[b][1]), np.float32(sampling[b][2]), sampling[b][3], sampling[b][4], True)
    got = sl.run_slots(s, codes, events, logits=True)
    s.free()
    spans, texts = check_conversations(cfg, codes, got, events, sampling, seed=5)
    assert spans == {0: [(0, C_ + 4), (C_ + 4, n)], 1: [(5, 14), (17, n)], 2: [(11, n)]}
    # really sampled (as tests/test_hip_frame.py asks of its sampled run): a conversation's text tokens are not all one value
    for key, t in texts.items():
        if len(t) >= 8:
            assert len(set(t)) > 1, (key, t)
    assert sum(len(t) >= 8 for t in texts.values()) >= 3


def test_a_seeded_conversation_does_not_depend_on_its_column_or_neighbours():
    cfg = tiny_sampled()
    n = 14
    conv = sl.slot_codes(cfg, 1, n, seed=21)               # the conversation's codes: [frame][0]
    other = sl.slot_codes(cfg, 3, n + 6, seed=22)
    mine = (77, 0.9, 0.6, 11, 9)

    def run(B, slot, start, neighbours, seed_of=mine):
        s = sp.Slots("oracle", cfg, B, seed=5)
        assert s.set_sampling(slot, *seed_of) == 0
        events = {start: [("open", slot)]}
        for b, (at, smp) in neighbours.items():
            events.setdefault(at, []).append(("open", b))
            if smp:
                assert s.set_sampling(b, *smp) == 0
        codes = [[conv[k - start][0] if b == slot and start <= k < start + n else other[k][b] for b in range(B)] for k in range(start + n)]
        got = sl.run_slots(s, codes, events)
        s.free()
        return [(g[1][slot], g[2][slot], g[3][slot]) for g in got[start:]]

    a = run(2, 0, 0, {1: (3, None)})                                                   # slot 0 of B = 2, beside an unseeded neighbour admitted later
    b = run(3, 2, 4, {0: (0, (5, 0.8, 0.7, 20, 25)), 1: (2, (6, 1.3, 1.2, 3, 4))})     # slot 2 of B = 3, admitted at frame 4 beside two seeded ones
    assert a == b
    assert any(st == 1 for st, _, _ in a)
    c = run(2, 0, 0, {1: (3, None)}, seed_of=(78,) + mine[1:])                         # another seed, everything else equal
    assert [x[1:] for x in a] != [x[1:] for x in c]


def test_unseeded_columns_keep_their_rand_draws():
    cfg = tiny_sampled()
    B, n = 3, 12
    codes = sl.slot_codes(cfg, B, n, seed=31)
    events = {0: [("open", 0), ("open", 1)], 3: [("open", 2)], 8: [("close", 1)]}

    def run(seeded):
        s = sp.Slots("oracle", cfg, B, seed=5)
        if seeded is not None:
            assert s.set_sampling(seeded, 9, 0.5, 0.9, 4, 5) == 0
        got = sl.run_slots(s, codes, events, before_step=lambda i: libc.srand(1000 + i))
        s.free()
        return got

    plain, one = run(None), run(1)
    for k, (p, o) in enumerate(zip(plain, one)):
        for b in (0, 2):
            assert (p[1][b], p[2][b], p[3][b]) == (o[1][b], o[2][b], o[3][b]), (k, b)
    assert any((p[2][1], p[3][1]) != (o[2][1], o[3][1]) for p, o in zip(plain, one))   # the seeded column itself did change
    # the same for a lockstep model
    def run_streams(seeded):
        s = sp.Streams("oracle", cfg, 2, seed=5)
        if seeded:
            assert s.set_sampling(0, 9, 0.5, 0.9, 4, 5) == 0
        out = []
        for i in range(6):
            libc.srand(1000 + i)
            out.append(s.step(codes[i][:2]))
        s.free()
        return out
    plain, one = run_streams(False), run_streams(True)
    assert [(r[1][1], r[2][1]) for r in plain] == [(r[1][1], r[2][1]) for r in one]


def test_noise_source_equals_the_header_formula_and_is_exponential():
    for seed in (0, 1, 12345, 0xFFFFFFFFFFFFFFFF, 0x9E3779B97F4A7C15):
        for frame in (0, 1, 7, 1000, 2 ** 33):
            for site in (0, 1, 8, 16):
                got = sp.lib_noise(seed, frame, site, 6)
                for rank in range(6):
                    u = sp.noise_u(seed, frame, site, rank)
                    assert 0 < u < 1
                    want = -np.log(np.float64(u))
                    # logf: within a few ulp of the correctly rounded logarithm; near u = 1 the result is tiny and the bar is absolute
                    assert abs(float(got[rank]) - want) <= 4 * np.spacing(np.float32(want)) + 1e-12, (seed, frame, site, rank, got[rank], want)
    # ranks beyond a call's n continue the same sequence; sites, frames and seeds are distinct streams
    assert np.array_equal(sp.lib_noise(5, 3, 2, 300)[:25], sp.lib_noise(5, 3, 2, 25))
    base = sp.lib_noise(5, 3, 2, 64)
    for other in (sp.lib_noise(6, 3, 2, 64), sp.lib_noise(5, 4, 2, 64), sp.lib_noise(5, 3, 3, 64)):
        assert not np.array_equal(base, other)
    # 100 000 draws over many (seed, frame, site): finite and > 0
    draws = np.concatenate([sp.lib_noise(1000 + s, f, site, 250) for s in range(5) for f in range(10) for site in range(8)])
    assert draws.size == 100000
    assert np.all(np.isfinite(draws)) and np.all(draws > 0)
    assert float(sp.lib_noise(0, 0, 0, 1)[0]) > 0 and -np.log(np.float32(1 - 2.0 ** -24)) > 0   # the smallest value the formula can give
    assert abs(float(draws.astype(np.float64).mean()) - 1.0) < 0.02          # standard error of an Exp(1) mean at this count: 0.0032
    hist, _ = np.histogram(np.exp(-draws.astype(np.float64)), bins=16, range=(0.0, 1.0))
    assert np.all(np.abs(hist - 6250) < 625), hist                           # exp(-x) is uniform: 6 250 per bin expected, sigma about 77


def test_refusals_change_nothing():
    greedy = su.lm_only(hu.hot.tiny(L))
    assert not greedy.temp > 0
    s = sp.Slots("oracle", greedy, 2)
    before = s.get_sampling(0)
    assert s.set_sampling(0, 1, 0.8, 0.7, 5, 5) == -1 and s.get_sampling(0) == before and before[5] is False
    s.free()
    cfg = tiny_sampled()
    s = sp.Slots("oracle", cfg, 3)
    before = [s.get_sampling(b) for b in range(3)]
    assert before[0] == (0, np.float32(0.8), np.float32(0.7), 20, 25, False)
    assert s.get_sampling(3) is None and s.get_sampling(-1) is None
    for b, args in [(3, (1, 0.8, 0.7, 20, 25)), (-1, (1, 0.8, 0.7, 20, 25)),          # bad column
                    (0, (1, 0.8, 0.7, 21, 25)), (0, (1, 0.8, 0.7, 20, 26)),           # top-k above the compiled maximum
                    (0, (1, 0.8, 0.7, 0, 25)), (0, (1, 0.8, 0.7, 20, 0)),             # top-k below 1
                    (0, (1, 0.0, 0.7, 20, 25)), (0, (1, 0.8, -1.0, 20, 25)), (0, (1, float("nan"), 0.7, 20, 25))]:
        assert s.set_sampling(b, *args) == -1, (b, args)
    assert [s.get_sampling(b) for b in range(3)] == before
    assert L.moshi_hot_set_sampling(s.m, 0, None) == -1
    # the setting belongs to the column: it survives close / open
    assert s.set_sampling(1, 4, 0.9, 0.6, 2, 3) == 0
    s.open(1); s.close(1); s.open(1)
    assert s.get_sampling(1) == (4, np.float32(0.9), np.float32(0.6), 2, 3, True)
    s.free()
    # single-stream: only the seed is free
    m = sp.Model("oracle", cfg)
    before = m.get_sampling(0)
    for args in [(1, 0.9, 0.7, 20, 25), (1, 0.8, 0.6, 20, 25), (1, 0.8, 0.7, 19, 25), (1, 0.8, 0.7, 20, 24)]:
        assert m.set_sampling(0, *args) == -1, args
    assert m.set_sampling(1, 1, 0.8, 0.7, 20, 25) == -1
    assert m.get_sampling(0) == before
    assert m.set_sampling(0, 1, 0.8, 0.7, 20, 25) == 0 and m.get_sampling(0)[5] is True
    m.free()
    # a variant whose samplers do not all sit in the two frame graphs refuses
    cd = sp.copy_cfg(cfg)
    cd.chain_depth = 1
    m = sp.Model("oracle", cd)
    assert m.set_sampling(0, 1, 0.8, 0.7, 20, 25) == -1 and m.get_sampling(0)[5] is False
    m.free()
