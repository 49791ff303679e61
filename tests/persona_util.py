"""Helpers for PersonaPlex streams and slots (persona_columns = 1, moshi_hot_slots_persona): B-column models whose frames take and give 8 codes per
column, personas (voice rows, ring image, text prompt, silence), and the single-stream sequence of the contract of include/moshi_hot.h."""
import ctypes as C

import numpy as np

import hot_util as hu
import sampling_util as sp
from ggml_util import BF16, F16, F32, bf16_bits_to_f32, f32_to_bf16_bits

L = hu.L
hot = hu.hot


def make_cfg(layers=1, persona_columns=1, **kw):
    """hot.tiny_personaplex, the LM alone: dim 512, 4 heads, a ring of 24, 16 Depth steps over a ring of 8"""
    cfg = hot.tiny_personaplex(L, layers=layers, **kw)
    cfg.enable_mimi_encoder = cfg.enable_mimi_decoder = 0
    cfg.persona_columns = persona_columns
    return cfg


def created(create, cfg, B):
    """does moshi_hot_create_streams / _slots (by name) build a model from cfg at B columns?"""
    be = hu.make_backend("oracle")
    m = getattr(L, create)(be, C.byref(cfg), 0, B)
    if m:
        L.moshi_hot_free(m)
    L.ggml_backend_free(be)
    return bool(m)


class _Columns:
    """a frame of a PersonaPlex B-column model: B x 8 codes in, B x 8 codes out (lm.h:802-805)"""

    def _io(self, codes):
        n = self.cfg.io_dep_q
        assert self.cfg.n_q - n == n
        ia = np.ascontiguousarray(np.array(codes, np.int32).reshape(self.B * n))
        return ia, np.full(self.B, -7, np.int32), np.full(self.B * n, -7, np.int32)


class Streams(_Columns, sp.Streams):
    def step(self, codes):
        """-> (ok, [B text tokens], [B lists of 8 audio tokens])"""
        ia, txt, aud = self._io(codes)
        r = L.moshi_hot_lm_step_streams(self.m, ia.ctypes.data, txt.ctypes.data, aud.ctypes.data)
        return r, txt.tolist(), aud.reshape(self.B, -1).tolist()


class Slots(_Columns, sp.Slots):
    def step(self, codes):
        """-> (n_valid, [B status], [B text tokens], [B lists of 8 audio tokens])"""
        ia, txt, aud = self._io(codes)
        st = np.full(self.B, -7, np.int32)
        r = L.moshi_hot_lm_step_slots(self.m, ia.ctypes.data, txt.ctypes.data, aud.ctypes.data, st.ctypes.data)
        return r, st.tolist(), txt.tolist(), aud.reshape(self.B, -1).tolist()

    def step_some(self, per_slot):
        """one frame, per_slot = {slot: 8 codes} (the others get zeros) -> step() + (text_logits [B, text_card],)"""
        codes = [per_slot.get(b, [0] * self.cfg.io_dep_q) for b in range(self.B)]
        return self.step(codes) + (self.read("text_logits", self.cfg.text_card),)

    def persona(self, jobs, chunk=0):
        """jobs: [(slot, Persona)] in one moshi_hot_slots_persona call -> its return value"""
        n = len(jobs)
        structs, keep = [], []
        for _, p in jobs:
            st, k = p.struct()
            structs.append(st)
            keep.append(k)
        arr = (hot.Persona * max(n, 1))(*structs)
        slots = (C.c_int32 * max(n, 1))(*[b for b, _ in jobs])
        return L.moshi_hot_slots_persona(self.m, n, slots, arr, chunk)

    def persona_one(self, b, p, chunk=0):
        st, keep = p.struct()
        return L.moshi_hot_slot_persona(self.m, b, C.byref(st), chunk)

    def hold(self, b, on):
        return L.moshi_hot_slot_hold(self.m, b, 1 if on else 0)

    def last_raw(self, b):
        out = np.zeros(self.cfg.n_q + 1, np.int32)
        assert L.moshi_hot_slot_last_raw(self.m, b, out.ctypes.data) == 0
        return out.tolist()

    def save(self, b):
        n = L.moshi_hot_slot_save(self.m, b, None, 0)
        if n < 0:
            return None
        buf = np.zeros(n, np.uint8)
        assert L.moshi_hot_slot_save(self.m, b, buf.ctypes.data, n) == n
        return buf

    def load(self, b, blob):
        return L.moshi_hot_slot_load(self.m, b, blob.ctypes.data, blob.nbytes)


class Persona:
    """n_voice voice rows of `vtype` (F32 / BF16 / F16; the values are exactly representable in it), a ring image or none, a text prompt, silence"""

    def __init__(self, cfg, seed, n_voice=5, vtype=F32, cache=True, n_text=3, silence=2):
        rng = np.random.default_rng(seed)
        v = (rng.standard_normal((n_voice, cfg.dim)) * 0.5).astype(np.float32)
        if vtype == BF16:
            self.raw = f32_to_bf16_bits(v).reshape(v.shape)
            v = bf16_bits_to_f32(self.raw)
        elif vtype == F16:
            self.raw = v.astype(np.float16)
            v = self.raw.astype(np.float32)
            self.raw = self.raw.view(np.uint16)
        else:
            self.raw = v
        self.voice_f32, self.vtype, self.silence = v, vtype, silence
        self.text = rng.integers(0, cfg.text_card, n_text).astype(np.int32)
        rows = 1 + 2 + 1          # max delay 1, + 2, + PersonaPlex's extra row (lm.h:727-731)
        self.cache = None
        if cache:
            self.cache = np.concatenate([rng.integers(0, cfg.text_card, (rows, 1)), rng.integers(0, cfg.card, (rows, cfg.n_q))], axis=1).astype(np.int32)
        self.rows = n_voice + 2 * silence + n_text

    def struct(self):
        return hot.persona(self.raw, self.vtype, self.cache, self.text, self.silence)


def live_codes(cfg, n, seed):
    return np.random.default_rng(seed).integers(0, cfg.card, (n, cfg.io_dep_q)).tolist()


def single_reference(kind, cfg, persona, codes, before=(), seed=0):
    """the contract's single-stream sequence on a fresh model: `before` live frames, n_voice x moshi_hot_lm_step_embedding, moshi_hot_set_host_ring,
    the system prompts (moshi_hot_personaplex_system_prompts when silence is the tool's 6, else the same provided frames one by one), then one live
    frame per entry of `codes` -> ([(ok, text, audio, text_logits)] per live frame, then the delay ring, transformer_out and the frame count right after the persona)"""
    m = hu.Model(kind, cfg, seed=seed)
    for fr in before:
        m.lm_step(fr)
    if persona is not None:
        for row in persona.voice_f32:
            m.lm_step_embedding(row)
        if persona.cache is not None:
            flat = np.ascontiguousarray(persona.cache.reshape(-1))
            assert L.moshi_hot_set_host_ring(m.m, flat.ctypes.data, flat.size) == 0
        if persona.silence == 6:
            m.system_prompts(persona.text.tolist())
        else:
            pt = [L.moshi_hot_personaplex_prompt_tokens()[i] for i in range(17)]
            for text in [pt[0]] * persona.silence + persona.text.tolist() + [pt[0]] * persona.silence:
                m.lm_step_n([text] + pt[1:])
    ring, tout, frames = m.host_ring().copy(), m.read("transformer_out", cfg.dim), L.moshi_hot_offset(m.m)
    out = []
    for fr in codes:
        r = m.lm_step(fr)
        out.append(r + (m.read("text_logits", cfg.text_card),))
    m.free()
    return out, ring, tout, frames


def assert_slot_equals_single(got, b, ref, what=""):
    """got: Slots.step_some results of the frames in which slot b ran the conversation whose single-stream frames are ref: bit for bit"""
    assert len(got) == len(ref)
    for k, (g, r) in enumerate(zip(got, ref)):
        assert g[1][b] == r[0], (what, b, k, g[1], r[0])
        if r[0]:
            assert g[2][b] == r[1] and g[3][b] == r[2], (what, b, k)
        assert np.array_equal(g[4][b], r[3]), (what, b, k)
