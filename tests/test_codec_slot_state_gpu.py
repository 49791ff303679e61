"""-m gpu: codec slot snapshots (moshi_hot_codec_slot_fork / _save / _load) on the MI355X, at Mimi's own size, for the decoder and the encoder. The
copies are exact, so blobs are compared byte for byte (fork against source, reload against blob, the two-launch plan against the generic nodes) and
continuations with np.array_equal (the project guarantees the same bits in any column of any batch). An oracle blob continues on the device within
2 x the single-stream device decode's own deviation from the oracle on the same codes, measured in the same test (the rule of
tests/test_codec_slots_gpu.py). The destination column is always dirty: another conversation ran through it for two frames first."""
import functools

import numpy as np
import pytest

import codec_slot_state_util as cs

pytestmark = pytest.mark.gpu
SEED = 3
N = 8
A, X = 900, 902
halves = pytest.mark.parametrize("half", cs.HALVES, ids=repr)
WRAP = 124                       # frames: one more frame fills the 250-row ring


def check_fork(half, s, src, dst, a):
    """fork src -> dst (dst closed and dirty), compare the blobs, then 3 frames of the same input"""
    assert cs.fork(s, src, dst) == 0 and s.position(dst) == s.position(src)
    one, two = cs.save(s, src), cs.save(s, dst)
    assert np.array_equal(one, two), f"fork {src} -> {dst} of {s.B}: {int(np.sum(one != two))} bytes differ"
    assert np.any(one[cs.HEADER:cs.HEADER + 4096] != 0) and np.any(one[-cs.FRAME_BYTES:] != 0)
    for k, f in enumerate(a):
        got = half.step(s, {src: f, dst: f})
        assert cs.same(got[src], got[dst]), (src, dst, k)
    return one


# both directions at B = 2; columns 1 <-> 2 at B = 3 (the encoder's 24-byte tail on an 8-aligned and on a 16-aligned base)
@halves
@pytest.mark.parametrize("B,src,dst", [(2, 0, 1), (2, 1, 0), (3, 1, 2), (3, 2, 1)])
def test_fork_copies_the_state_exactly_after_one_frame_and_past_the_wrap(half, B, src, dst):
    s = half.make("hip", B, seed=SEED)
    cs.dirty(half, s, dst)
    a = half.frames(A, N)
    assert s.open(src) == 0
    cs.run(half, s, src, a[:1])
    blob = check_fork(half, s, src, dst, a[1:4])                     # n = 2
    assert cs.header(blob)["n"] == 2
    assert s.close(dst) == 0
    s.set_fill(src, WRAP)
    cs.run(half, s, src, a[4:5])
    blob = check_fork(half, s, src, dst, a[5:8])                     # n = 250: live rows nobody wrote among them
    assert cs.header(blob)["n"] == cs.CAPACITY and cs.header(blob)["pos"] == WRAP + 1
    s.free()


@halves
def test_saved_slot_reloads_exactly_and_continues_like_the_uninterrupted_conversation(half):
    s = half.make("hip", 2, seed=SEED)
    a = half.frames(A, N)
    assert s.open(1) == 0
    cs.run(half, s, 1, a[:3])
    blob = cs.save(s, 1)
    assert cs.save_size(s, 1) == blob.nbytes and cs.header(blob)["n"] == 6
    want = cs.run(half, s, 1, a[3:6])                                # the uninterrupted conversation
    s.free()
    t = half.make("hip", 3, seed=SEED)
    cs.dirty(half, t, 2)
    assert cs.load(t, 2, blob) == 0 and t.position(2) == 3
    again = cs.save(t, 2)
    assert np.array_equal(again, blob), f"reload: {int(np.sum(again != blob))} bytes differ"
    got = cs.run(half, t, 2, a[3:6])
    t.free()
    for k in range(3):
        assert cs.same(got[k], want[k]), k


@halves
def test_wide_batch_fork_from_the_first_into_the_last_of_33_columns(half):
    s = half.make("hip", 33, seed=SEED, wide=True)
    cs.dirty(half, s, 32)
    a = half.frames(A, N)
    assert s.open(0) == 0
    cs.run(half, s, 0, a[:2])
    check_fork(half, s, 0, 32, a[2:4])
    s.free()


@halves
def test_live_neighbour_is_untouched_by_snapshots_of_other_columns(half):
    a, x = half.frames(A, N), half.frames(X, N)

    def run(snapshots):
        s = half.make("hip", 3, seed=SEED)
        cs.dirty(half, s, 2)
        assert s.open(0) == 0 and s.open(1) == 0
        out = [half.step(s, {0: a[0], 1: x[0]})[0]]
        blob = None
        if snapshots:
            assert cs.fork(s, 1, 2) == 0
            blob = cs.save(s, 1)
            assert s.close(2) == 0
        out.append(half.step(s, {0: a[1], 1: x[1]})[0])
        if snapshots:
            assert cs.load(s, 2, blob) == 0 and s.close(2) == 0
        out.append(half.step(s, {0: a[2], 1: x[2]})[0])
        s.free()
        return out
    plain, busy = run(False), run(True)
    for k in range(3):
        assert cs.same(plain[k], busy[k]), k


@halves
def test_two_launch_plan_against_generic_nodes(half):
    s = half.make("hip", 4, seed=SEED)
    cs.dirty(half, s, 1)
    cs.dirty(half, s, 3, seed=951)
    assert s.open(2) == 0
    cs.run(half, s, 2, half.frames(A, N)[:2])                        # (the frames run under the default plan: one state for both paths)
    want = cs.save(s, 2)
    for flags, dst in ((0, 1), (1, 3)):                              # 1: no fusion - every cpy of the snapshot graphs runs as a generic copy
        cs.L.ggml_backend_mi355x_set_flags(s.be, flags)
        assert cs.fork(s, 2, dst) == 0
        assert s.stats().state_copy_launches_in_last_plan == 1 - flags
        got = cs.save(s, dst)
        assert s.stats().state_copy_launches_in_last_plan == 1 - flags
        assert np.array_equal(got, want), f"flags {flags}: {int(np.sum(got != want))} bytes differ between the fork and its source"
    s.free()


@functools.lru_cache(maxsize=None)
def oracle_decoder(n):
    half = cs.HALVES[0]
    out = half.reference("oracle", half.frames(A, N)[:n], seed=SEED)
    return np.stack([o[0] for o in out])


def test_oracle_decoder_blob_continues_on_the_device():
    half = cs.HALVES[0]
    a = half.frames(A, N)
    o = half.make("oracle", 2, seed=SEED)
    assert o.open(0) == 0
    cs.run(half, o, 0, a[:3])
    blob = cs.save(o, 0)
    o.free()
    t = half.make("hip", 3, seed=SEED)
    cs.dirty(half, t, 1)
    assert cs.load(t, 1, blob) == 0 and t.position(1) == 3
    got = np.stack([g[0] for g in cs.run(half, t, 1, a[3:6])])
    t.free()
    ref = oracle_decoder(6)
    dev = np.stack([g[0] for g in half.reference("hip", a[:6], seed=SEED, flags=16)])   # the single-stream device decode: plain launches
    single = float(np.abs(dev - ref).max())
    worst = float(np.abs(got - ref[3:6]).max())
    print(f"oracle blob continued on the device: max abs PCM deviation from the oracle's continuation {worst:.3e}; single-stream device decode {single:.3e}")
    assert worst <= 2 * single, (worst, single)


@halves
def test_each_call_plans_one_ring_copy_and_one_state_copy_launch(half):
    a = half.frames(A, N)
    for flags in (0, 1):
        s = half.make("hip", 3, seed=SEED, flags=flags)
        cs.dirty(half, s, 1)
        assert s.open(0) == 0
        cs.run(half, s, 0, a[:2])
        plans = {}
        assert cs.fork(s, 0, 1) == 0
        plans["fork"] = s.stats()
        blob = cs.save(s, 0)
        plans["save"] = s.stats()
        assert cs.load(s, 2, blob) == 0
        plans["load"] = s.stats()
        s.free()
        for name, st in plans.items():
            print(f"{half} flags {flags} {name}: {st.kernels_in_last_plan} launches, {st.ring_copy_launches_in_last_plan} ring-copy launches holding "
                  f"{st.ring_copy_jobs_in_last_plan} jobs, {st.state_copy_launches_in_last_plan} state-copy launches holding {st.state_copy_jobs_in_last_plan} jobs")
            if flags:
                assert st.ring_copy_launches_in_last_plan == 0 and st.state_copy_launches_in_last_plan == 0 and st.state_copy_jobs_in_last_plan == 0, name
                assert st.kernels_in_last_plan == 2 * cs.LAYERS + 11, name
            else:
                assert st.ring_copy_launches_in_last_plan == 1 and st.ring_copy_jobs_in_last_plan == 2 * cs.LAYERS, name
                assert st.state_copy_launches_in_last_plan == 1 and st.state_copy_jobs_in_last_plan == 11, name
                assert st.kernels_in_last_plan == 2, name
