"""CPU: the committed protocol trace tests/golden/driver_trace.npz (made by tests/golden/make_driver_trace.py) replayed on the host device with the
oracle attached. Everything in it is a function of the inputs alone - teacher-forced delay rings, return values and frame counts of three
single-stream variants, and the header-through-ring bytes of slot snapshot blobs after a multi-pass slot prefill - so the comparison is exact: it pins
the delay-ring arithmetic and the blob's on-disk format."""
import functools
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_driver_trace as mk  # noqa: E402


@functools.lru_cache(maxsize=None)
def golden():
    with np.load(mk.PATH) as z:
        return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=None)
def replayed(name):
    part = mk.single(name) if name in ("moshika", "personaplex", "tts") else mk.slots(name == "slots_sampled")
    return {f"{name}.{k}": v for k, v in part.items()}


PARTS = ("moshika", "personaplex", "tts", "slots", "slots_sampled")


def test_the_trace_has_every_part_and_nothing_else():
    want = {"ret", "offset", "ring"}
    keys = {p: {k.split(".", 1)[1] for k in golden() if k.startswith(p + ".")} for p in PARTS}
    assert keys["moshika"] == keys["personaplex"] == want | {"ids"} and keys["tts"] == want | {"hook_offsets"}
    assert keys["slots"] == keys["slots_sampled"] == {"blob0", "blob2", "positions"}
    assert sum(len(v) for v in keys.values()) == len(golden())


@pytest.mark.parametrize("name", PARTS)
def test_replay_equals_the_committed_trace(name):
    got, want = replayed(name), {k: v for k, v in golden().items() if k.startswith(name + ".")}
    assert sorted(got) == sorted(want)
    for k in sorted(want):
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert np.array_equal(got[k], want[k]), (k, np.argwhere(got[k] != want[k])[:4].tolist())


def test_the_trace_covers_what_it_is_there_for():
    g = golden()
    for name in ("moshika", "personaplex", "tts"):
        ring, ret, off = g[f"{name}.ring"], g[f"{name}.ret"], g[f"{name}.offset"]
        assert len(ret) > 2 * ring.shape[1] and np.all(np.diff(off) == 1)       # the ring wraps at least twice
        assert ret[0] == (name == "personaplex") and ret[-1] == 1               # still filling (the prompt frames have filled PersonaPlex's), then valid
        assert 0 in ret[off > ring.shape[1]]                                    # a forced -1 met by a read-out of the full ring
        assert -1 in ring and not np.any(ring[-1] == -2)                        # the fresh ring's -2 is gone by the end
    assert g["personaplex.offset"][0] == 6 + 3 + 6 + 1                          # the system prompts' provided frames count
    assert g["tts.hook_offsets"].tolist() == list(range(len(g["tts.ret"])))
    assert g["slots.positions"].tolist() == g["slots_sampled.positions"].tolist() == [5, -1, 4]
    seeded = [int(g[f"{p}.blob{b}"][56:60].view(np.int32)[0]) for p in ("slots", "slots_sampled") for b in (0, 2)]
    assert seeded == [0, 0, 1, 0]                                               # the seeded flag of the header
    assert not np.array_equal(g["slots.blob0"][mk.BLOB_HEADER:], g["slots.blob2"][mk.BLOB_HEADER:])
