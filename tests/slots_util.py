"""Helpers for stream-slot models (moshi_hot_create_slots / moshi_hot_lm_step_slots)."""

import numpy as np

import hot_util as hu
import streams_util as su

L = hu.L
lm_only = su.lm_only


class Slots(su.Streams):
    """B stream slots over one set of weights on a backend ("oracle" or "hip"); every slot starts closed."""

    create = "moshi_hot_create_slots"

    def open(self, b):
        return L.moshi_hot_slot_open(self.m, b)

    def close(self, b):
        return L.moshi_hot_slot_close(self.m, b)

    def position(self, b):
        return L.moshi_hot_slot_position(self.m, b)

    def set_fill(self, b, offset):
        L.moshi_hot_slot_set_fill(self.m, b, offset)

    def step(self, codes):
        """codes: B lists of (n_q - dep_q) codes -> (n_valid, [B status], [B text tokens], [B lists of dep_q audio tokens])"""
        B, n_in, dq = self.B, self.cfg.n_q - self.cfg.dep_q, self.cfg.dep_q
        ia = np.ascontiguousarray(np.array(codes, np.int32).reshape(B * n_in))
        txt = np.full(B, -7, np.int32)
        aud = np.full(B * dq, -7, np.int32)
        st = np.full(B, -7, np.int32)
        r = L.moshi_hot_lm_step_slots(self.m, ia.ctypes.data, txt.ctypes.data, aud.ctypes.data, st.ctypes.data)
        return r, st.tolist(), txt.tolist(), aud.reshape(B, dq).tolist()


def run_slots(slots, codes, events=None, logits=False, dep_logits=False, before_step=None):
    """every frame of `codes` ([frame][slot]) through a Slots model. events: {frame: [("open" | "close", slot), ...]} applied before that frame's
    step. -> per frame (n_valid, status, texts, audios[, text_logits [B, text_card]][, last Depth logits [B, card]])"""
    cfg = slots.cfg
    out = []
    for i, fr in enumerate(codes):
        for what, b in (events or {}).get(i, []):
            assert (slots.open(b) if what == "open" else slots.close(b)) == 0
        if before_step:
            before_step(i)
        r = slots.step(fr)
        if logits:
            r = r + (slots.read("text_logits", cfg.text_card),)
        if dep_logits:
            r = r + (slots.read(f"dep_logits{cfg.dep_q - 1}", cfg.card),)
        out.append(r)
    return out


def conversations(events, n_frames):
    """events -> {slot: [(first frame, end frame)]}: the frame ranges each conversation occupied its slot"""
    spans, start = {}, {}
    for i in range(n_frames + 1):
        for what, b in (events or {}).get(i, []):
            if b in start:
                spans.setdefault(b, []).append((start.pop(b), i))
            if what == "open":
                start[b] = i
    for b, s in start.items():
        spans.setdefault(b, []).append((s, n_frames))
    return spans


def slot_codes(cfg, n_slots, n_frames, seed=0):
    return su.stream_codes(cfg, n_slots, n_frames, seed)
