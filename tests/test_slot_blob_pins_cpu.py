"""CPU (oracle): the header of a snapshot blob, pinned. One model per blob kind - a moshika-shaped slots model (tests/test_slot_state_cpu.py's
configuration), a tts-shaped one through the _full calls (tests/test_tts_slot_state_cpu.py's), decoder slots and encoder slots at Mimi's own size
(tests/test_codec_slot_state_cpu.py's) - has one slot positioned with moshi_hot_slot_set_fill / moshi_hot_codec_slot_set_fill at 0, at a few frames
and past the ring's end, and saved. Magic, version, kind (where the format has it), fingerprint, total_bytes, position and live row count are
integer functions of the configuration and the position alone, so they hold on any host; no frame is stepped.

PINS was recorded by running this file's body against the library built from commit 7b17597, the last one before the two blob kinds were put on one
fingerprint mixer, one ring size and one save / load scaffold - never from the library under test. A change of a blob is a change of this table, made
on purpose."""
import struct

import pytest

import codec_slot_state_util as cs
import ggml_util as gu
import hot_util as hu
import slot_state_util as ss
import streams_util as su
import tts_replay_util as ru
import tts_slots_util as tu

L = hu.L
SEED = 5
LM_POSITIONS = (0, 3, 30)        # the LM rings hold 24 rows
CODEC_POSITIONS = (0, 3, 130)    # the codec rings hold 250 rows, two a frame: full from frame 125 on


def lm_header(blob):
    names = ("magic", "version", "fingerprint", "total_bytes", "frames", "pos", "n", "ring_rows", "ring_cols")
    return dict(zip(names, struct.unpack("<IIQqqqqii", bytes(blob[:56]))))


def moshika_slots(positions):
    s = ss.Slots("oracle", su.lm_only(hu.hot.tiny(L, context=24)), 2, seed=SEED)
    assert s.open(1) == 0
    for pos in positions:
        s.set_fill(1, pos)
        yield lm_header(s.save(1))
    s.free()


def tts_slots(positions):
    cfg = tu.tts_cfg(linear_type=gu.F32, embed_type=gu.F32, layers=1, cross_len=5)
    cfg.context = 24
    s = ru.Slots("oracle", cfg, 2, seed=SEED)
    assert s.set_conditions(1, 4) == 0 and s.open(1) == 0
    for pos in positions:
        s.set_fill(1, pos)
        assert s.save_size(1) == -1                  # the plain call refuses the shape
        yield lm_header(s.save_full(1))
    s.free()


def codec_slots(half, positions):
    s = half.make("oracle", 2, seed=SEED)
    assert s.open(1) == 0
    for pos in positions:
        s.set_fill(1, pos)
        h = cs.header(cs.save(s, 1))
        assert h["reserved"] == 0
        yield h
    s.free()


# one model per kind, its slot 1 moved from position to position
KINDS = {
    "moshika_slots": (moshika_slots, LM_POSITIONS),
    "tts_slots_full": (tts_slots, LM_POSITIONS),
    "decoder_slots": (lambda positions: codec_slots(cs.HALVES[0], positions), CODEC_POSITIONS),
    "encoder_slots": (lambda positions: codec_slots(cs.HALVES[1], positions), CODEC_POSITIONS),
}

# per kind: (magic, version, kind or None, fingerprint), then per position (total_bytes, live rows)
PINS = {
    "moshika_slots": ((0x544c534d, 1, None, 0xef33aed0b6972185), [(2224, 0), (14512, 3), (100528, 24)]),
    "tts_slots_full": ((0x544c534d, 2, None, 0x471913eebf1c5f3b), [(14576, 0), (20720, 3), (63728, 24)]),
    "decoder_slots": ((0x4c53434d, 1, 1, 0x25c4b7a2a0cbf0ad), [(923184, 0), (1021488, 6), (5019184, 250)]),
    "encoder_slots": ((0x4c53434d, 1, 2, 0x8987a9124b2f1efd), [(46160, 0), (144464, 6), (4142160, 250)]),
}


@pytest.mark.parametrize("kind", list(KINDS))
def test_blob_header_is_what_it_was(kind):
    make, positions = KINDS[kind]
    (magic, version, kind_id, fingerprint), per_pos = PINS[kind]
    assert len(per_pos) == len(positions)
    for pos, (total, n), h in zip(positions, per_pos, list(make(positions))):
        print(f"{kind} at {pos}: " + " ".join(f"{k}={v:#x}" if k in ("magic", "fingerprint") else f"{k}={v}" for k, v in h.items()))
        assert (h["magic"], h["version"], h.get("kind"), h["fingerprint"]) == (magic, version, kind_id, fingerprint), (kind, pos)
        assert (h["total_bytes"], h["pos"], h["n"]) == (total, pos, n), (kind, pos)
