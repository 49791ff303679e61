"""Helpers for the codec slot snapshot tests (moshi_hot_codec_slot_fork / _save / _load, include/moshi_hot.h): the decoder-slots and the encoder-slots
model behind one interface, so that every case runs for both halves, the snapshot calls, and the blob's layout."""
import ctypes as C
import struct

import numpy as np

import codec_slots_util as du
import encoder_slots_util as eu
import hot_util as hu

L = hu.L
HEADER = 48                      # magic, version, kind, reserved (u32 each), fingerprint (u64), total bytes, position, n (i64 each)
LAYERS, DIM, ROWS_PER_FRAME, CAPACITY = 8, 512, 2, 250
FRAME_BYTES = 2 * LAYERS * DIM * 2 * ROWS_PER_FRAME   # K and V, every layer, H x D BF16, the rows of one frame


class Half:
    """one half of the codec at B columns: `decoder` (codes in, PCM out) or `encoder` (PCM in, codes and both latents out)"""

    def __init__(self, name):
        assert name in ("decoder", "encoder")
        self.name, self.dec = name, name == "decoder"
        self.kind_id = 1 if self.dec else 2

    def __repr__(self):
        return self.name

    def cfg(self, wide=False):
        return du.cfg_of(wide) if self.dec else eu.cfg_of(wide)

    def make(self, kind, B, seed=0, flags=0, wide=False):
        return (du.CodecSlots if self.dec else eu.EncoderSlots)(kind, self.cfg(wide), B, seed=seed, flags=flags)

    def frames(self, seed, n):
        """n frames of seeded input: codes [n, 8] or PCM [n, 1920]"""
        return du.codes(seed, n) if self.dec else eu.pcm(seed, n)

    def step(self, s, rows):
        """one frame; rows: {slot: input frame} for exactly the open slots -> {slot: tuple of output arrays}"""
        full = [rows.get(b) for b in range(s.B)]
        if self.dec:
            r, pcm, status = s.decode(full)
            assert r == len(rows) and all(status[b] == 1 for b in rows), (r, list(status))
            return {b: (pcm[b].copy(),) for b in rows}
        r, codes, status = s.encode(full)
        assert r == len(rows) and all(status[b] == 1 for b in rows), (r, list(status))
        lf, lr = s.latents()
        return {b: (codes[b].copy(), lf[b].copy(), lr[b].copy()) for b in rows}

    def reference(self, kind, frames, seed=0, fill=0, flags=0):
        """a fresh single-stream codec-only model, its transformer position moved to `fill` frames first, fed `frames` one by one -> list of output tuples"""
        m = hu.Model(kind, self.cfg(), seed=seed, flags=flags)
        if fill:
            L.moshi_hot_set_context_fill(m.m, fill)
        out = []
        for f in frames:
            if self.dec:
                out.append((m.mimi_decode(f.tolist()),))
            else:
                out.append((np.array(m.mimi_encode(f), np.int32), m.read("enc_latent_first", 256), m.read("enc_latent_rest", 256)))
        m.free()
        return out


HALVES = [Half("decoder"), Half("encoder")]


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def fork(s, src, dst):
    return L.moshi_hot_codec_slot_fork(s.m, src, dst)


def save_size(s, b):
    return L.moshi_hot_codec_slot_save(s.m, b, None, 0)


def save(s, b):
    n = save_size(s, b)
    assert n > HEADER, n
    buf = np.full(n, 0xA5, np.uint8)
    assert L.moshi_hot_codec_slot_save(s.m, b, buf.ctypes.data, n) == n
    return buf


def load(s, b, blob):
    blob = np.ascontiguousarray(blob, np.uint8)
    return L.moshi_hot_codec_slot_load(s.m, b, blob.ctypes.data, blob.nbytes)


def header(blob):
    """-> dict of the blob's header fields"""
    names = ("magic", "version", "kind", "reserved", "fingerprint", "total_bytes", "pos", "n")
    return dict(zip(names, struct.unpack("<IIIIQqqq", bytes(blob[:HEADER]))))


def dirty(half, s, b, seed=950):
    """another conversation runs through column b for two frames and leaves: a state or a ring row that a later copy misses shows"""
    assert s.open(b) == 0
    for f in half.frames(seed, 8)[:2]:
        half.step(s, {b: f})
    assert s.close(b) == 0


def run(half, s, b, frames):
    """slot b alone through `frames` -> list of output tuples"""
    return [half.step(s, {b: f})[b] for f in frames]
