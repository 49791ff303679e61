"""CPU (oracle): B-column models of 17 .. 64 conversations (wide_streams = 1 in the configuration; MOSHI_HOT_MAX_STREAMS = 64). Every statement the narrower suites make about a column -
it is the single-stream model of its conversation, bit for bit - at the new widths: lockstep at B = 33, slots at B = 64 with staggered opens, a
reopened slot and seeded columns, stt heads at B = 20, tts conditions at B = 18, 40 prefill jobs in one call, and snapshots across widths."""
import ctypes as C

import numpy as np
import pytest

import hot_util as hu
import sampling_util as sp
import slot_prefill_util as pu
import slot_state_util as ss
import slots_util as sl
import streams_util as su
import stt_slots_util as st
import tts_slots_util as tu

L = hu.L
libc = C.CDLL(None)
SEED = 5


def wide(cfg, on=1):
    cfg.wide_streams = on
    return cfg


def tiny(**kw):
    return wide(su.lm_only(hu.hot.tiny(L, **kw)))


def _created(cfg, n, fn):
    be = hu.make_backend("oracle")
    m = getattr(L, fn)(be, C.byref(cfg), 0, n)
    if m:
        assert L.moshi_hot_n_streams(m) == n
        L.moshi_hot_free(m)
    L.ggml_backend_free(be)
    return bool(m)


def stt_no_heads():
    c = hu.hot.tiny_stt(L, layers=1)
    c.extra_heads = c.extra_heads_dim = 0
    return c


@pytest.mark.parametrize("shape", ["moshika", "stt", "stt_no_heads", "tts"])
def test_widths_up_to_64_create_and_65_is_refused(shape):
    cfg_of = {"moshika": lambda: tiny(layers=1), "stt": lambda: hu.hot.tiny_stt(L, layers=1), "stt_no_heads": stt_no_heads,
              "tts": lambda: tu.tts_cfg(layers=1)}[shape]
    for fn in ("moshi_hot_create_streams", "moshi_hot_create_slots"):
        assert hu.hot.MAX_STREAMS == 64
        for B in (17, 33, hu.hot.MAX_STREAMS):
            assert _created(wide(cfg_of()), B, fn), (fn, B)
        for B in (65, 66, 128):
            assert not _created(wide(cfg_of()), B, fn), (fn, B)
        # a configuration that does not ask for wide batches keeps the limit of 16
        assert _created(wide(cfg_of(), 0), 16, fn) and not _created(wide(cfg_of(), 0), 17, fn) and not _created(wide(cfg_of(), 0), 64, fn)


def test_lockstep_33_columns_equal_single_stream_models():
    cfg = tiny()
    B, n = 33, 10
    codes = su.stream_codes(cfg, B, n, seed=33)
    last = f"dep_logits{cfg.dep_q - 1}"
    s = su.Streams("oracle", cfg, B, seed=SEED)
    got = []
    for fr in codes:
        got.append(s.step(fr) + (s.read("text_logits", cfg.text_card), s.read(last, cfg.card)))
    s.free()
    assert any(g[0] == 1 for g in got)
    for b in (0, 16, 32):
        m = hu.Model("oracle", cfg, seed=SEED)
        for k in range(n):
            r = m.lm_step(codes[k][b])
            g = got[k]
            assert g[0] == r[0], (b, k)
            if r[0]:
                assert g[1][b] == r[1] and g[2][b] == r[2], (b, k)
            assert np.array_equal(g[3][b], m.read("text_logits", cfg.text_card)), (b, k)
            assert np.array_equal(g[4][b], m.read(last, cfg.card)), (b, k)
        m.free()
    assert len({tuple(got[-1][2][b]) for b in (0, 16, 32)}) > 1 or len({got[-1][1][b] for b in (0, 16, 32)}) > 1   # the columns differ


def test_slots_64_staggered_reopened_and_seeded_columns():
    cfg = sp.sampled(tiny(layers=1))
    B, n = 64, 12
    conv = sl.slot_codes(cfg, 1, n, seed=61)                   # the seeded conversation's codes, fed to columns 3 and 60 from their own first frame
    codes = sl.slot_codes(cfg, B, n, seed=64)
    start = {b: b % 6 for b in range(B)}                       # opens staggered over the first 6 frames
    for b in (3, 60):
        for k in range(start[b], n):
            codes[k][b] = conv[k - start[b]][0]
    events = {}
    for b, f in start.items():
        events.setdefault(f, []).append(("open", b))
    events.setdefault(8, []).append(("close", 63))
    events.setdefault(10, []).append(("open", 63))
    mine = (77, 0.9, 0.6, 11, 9)

    def run(seeded):
        s = sp.Slots("oracle", cfg, B, seed=SEED)
        for b in seeded:
            assert s.set_sampling(b, *mine) == 0
        got = sl.run_slots(s, codes, events, before_step=lambda i: libc.srand(1000 + i))
        s.free()
        return got

    plain, both = run(()), run((3, 60))
    ref = sp.run_single("oracle", cfg, mine, [c[0] for c in conv], seed=SEED)
    for b in (3, 60):
        for k in range(start[b], n):
            g, r = both[k], ref[k - start[b]]
            assert g[1][b] == r[0], (b, k)
            if r[0]:
                assert g[2][b] == r[1] and g[3][b] == r[2], (b, k)
    assert any(r[0] for r in ref)
    # every unseeded column keeps the rand() draws it has without the seeded pair - the reopened column 63 among them
    for k, (p, o) in enumerate(zip(plain, both)):
        for b in range(B):
            if b not in (3, 60):
                assert (p[1][b], p[2][b], p[3][b]) == (o[1][b], o[2][b], o[3][b]), (k, b)
    assert any((p[2][3], p[3][3]) != (o[2][3], o[3][3]) for p, o in zip(plain, both))   # the seeded columns themselves did change
    # column 63: open from frame 3, closed for frames 8 and 9, a fresh conversation (its delay ring filling again) from frame 10
    assert [g[1][63] for g in both[8:10]] == [-1, -1] and both[7][1][63] == 1 and [g[1][63] for g in both[10:]] == [g[1][3] for g in both[3:5]]
    assert max(g[0] for g in both) >= B - 2


def test_stt_heads_at_20_columns():
    cfg = wide(hu.hot.tiny_stt(L, context=24))
    B, n = 20, 6
    convs = {b: st.codes(cfg, n, seed=500 + b) for b in range(B)}
    closed = {4, 19}
    s = st.Slots("oracle", cfg, B, seed=SEED)
    for b in range(B):
        if b not in closed:
            assert s.open(b) == 0
    got = []
    for k in range(n):
        r = st.step_all(s, {b: convs[b][k] for b in range(B) if b not in closed})
        assert r[5].shape == (B, cfg.extra_heads, cfg.extra_heads_dim)
        buf = np.zeros(B * cfg.extra_heads * cfg.extra_heads_dim, np.float32)
        assert L.moshi_hot_last_heads(s.m, buf.ctypes.data, buf.size) == buf.size
        assert L.moshi_hot_last_heads(s.m, buf.ctypes.data, buf.size - 1) == -1
        for b in closed:
            assert r[1][b] == -1 and np.all(r[5][b] == -1), (k, b)
        got.append(r)
    s.free()
    for b in (0, 5, 16, 18):
        st.assert_column_equals_single(got, b, st.single_reference("oracle", cfg, [], convs[b], seed=SEED), f"column {b}")
    assert all(g[0] == B - len(closed) for g in got)


def test_tts_18_columns_with_their_own_conditions():
    cfg = wide(tu.tts_cfg())
    B, n = 18, 8
    s = tu.Streams("oracle", cfg, B, seed=SEED)
    for b in range(B):
        assert s.set_conditions(b, 4 + b) == 0
    streams = [tu.text_stream(cfg, b, n) for b in range(B)]
    got = []
    for i in range(n):
        r = s.step([streams[b][i] for b in range(B)])
        got.append(r + (tu.reads(s, cfg, i >= cfg.delay_steps),))
    s.free()
    assert any(g[0] == 1 for g in got)
    for b in (0, 17):
        tu.assert_column_equals_single(got, b, tu.single_reference("oracle", cfg, 4 + b, streams[b], seed=SEED), f"column {b}")
    assert not np.array_equal(got[-1][3]["transformer_out"][0], got[-1][3]["transformer_out"][17])


def test_forty_prefill_jobs_in_one_call_on_64_slots():
    cfg = tiny()
    B, n_jobs, n_live = 64, 40, 3
    lens = [1 + (j % 5) for j in range(n_jobs)]                # histories of 1 .. 5 frames: 120 rows, two 64-row passes, jobs that span them
    slots = [(3 * j + 1) % B for j in range(n_jobs)]           # not in column order
    assert len(set(slots)) == n_jobs
    hists = [pu.history(cfg, lens[j], seed=900 + lens[j]) for j in range(n_jobs)]   # five distinct histories
    live = {ln: pu.live_codes(cfg, n_live, seed=950 + ln) for ln in set(lens)}
    s = pu.Slots("oracle", cfg, B, seed=SEED)
    for b in slots:
        assert s.open(b) == 0
    assert s.prefill(list(zip(slots, hists)), 64) == sum(lens)
    assert [s.position(b) for b in slots] == lens
    got = [pu.step_all(s, {b: live[lens[j]][k] for j, b in enumerate(slots)}) for k in range(n_live)]
    s.free()
    refs = {ln: pu.single_reference("oracle", cfg, pu.history(cfg, ln, seed=900 + ln), live[ln], seed=SEED, chunk=64) for ln in set(lens)}
    for j, b in enumerate(slots):
        pu.assert_slot_equals_single(got, b, refs[lens[j]], f"job {j} in slot {b}")
    idle = sorted(set(range(B)) - set(slots))
    assert all(g[1][b] == -1 for g in got for b in idle)


def test_fork_into_column_50_and_a_b4_blob_loaded_into_column_40_of_b64():
    cfg = tiny()
    n_before, n_after = 7, 6
    A = ss.live_codes(cfg, n_before + n_after, seed=71)
    ref = ss.single_reference("oracle", cfg, [], A, seed=SEED)
    small = ss.Slots("oracle", cfg, 4, seed=SEED)
    assert small.open(1) == 0
    ss.run(small, {1: A}, n_before)
    blob = small.save(1)
    small.free()
    assert blob is not None
    s = ss.Slots("oracle", cfg, 64, seed=SEED)
    assert s.open(2) == 0
    before = ss.run(s, {2: A}, n_before)
    assert s.fork(2, 50) == 0 and s.position(50) == n_before
    assert s.load(40, blob) == 0 and s.position(40) == n_before      # the fingerprint does not carry B
    after = [ss.step_all(s, {2: A[n_before + k], 50: A[n_before + k], 40: A[n_before + k]}) for k in range(n_after)]
    again = s.save(40)
    s.free()
    ss.assert_slot_equals_single(before + after, 2, ref, "source")
    for b in (50, 40):
        ss.assert_slot_equals_single(after, b, ref[n_before:], f"column {b}")
    assert any(r[1][40] == 1 for r in after)
    back = ss.Slots("oracle", cfg, 4, seed=SEED)                     # and a blob saved from column 40 of the wide model loads into a narrow one
    assert back.load(3, again) == 0 and back.position(3) == n_before + n_after
    back.free()
