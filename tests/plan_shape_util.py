"""The plan counters of every model kind, graph by graph: one two-layer synthetic model per kind, two steps (plus the frames a tts model waits
before its first Depth step) or the batched passes of its kind and a live step, the counters read after every call that computes graphs, then each
cached graph computed once more on its own and read again. Shared by tests/test_plan_shape_gpu.py (asserts the counters) and tests/microbench/plan_dump_shapes.py (prints them)."""
import codec_slot_state_util as cs
import codec_slots_util as du
import encoder_slots_util as eu
import hot_util as hu
import persona_util as pp
import sampling_util as sp
import slot_prefill_long_util as lu
import slot_prefill_util as pu
import slot_state_util as ss
import slots_util as sl
import streams_util as su
import stt_slots_util as st
import tts_replay_util as ru
import tts_slots_util as tu
from ggml_util import F32, Q4_0, Q4_K

L = hu.L

COUNTERS = ("kernels_in_last_plan", "fused_nodes_in_last_plan", "nodes_in_last_plan", "chained_matvecs_in_last_plan", "chain_step_programs_in_last_plan",
            "vq_levels_chained_in_last_plan", "attn_block_launches_in_last_plan", "attn_block_jobs_in_last_plan", "generic_attention_nodes_in_last_plan",
            "ring_copy_launches_in_last_plan", "ring_copy_jobs_in_last_plan", "attention_folds_planned",
            "attn_row_launches_in_last_plan", "attn_row_jobs_in_last_plan", "attn_row_rows_in_last_plan", "cross_block_launches_in_last_plan",
            "cross_block_jobs_in_last_plan", "float_batched_mms_in_last_plan", "float_acc_mms_in_last_plan", "pass_input_launches_in_last_plan",
            "pass_input_rows_in_last_plan",
            "convtr_column_groups_in_last_plan", "codec_attn_launches_in_last_plan", "vq_column_levels_in_last_plan", "code_gather_columns_in_last_plan",
            "state_copy_launches_in_last_plan", "state_copy_jobs_in_last_plan")
GRAPHS = ((0, "temporal graph"), (1, "depth graph"))
RING = 8


def counters(model):
    s = model.stats()
    return tuple(int(getattr(s, n)) for n in COUNTERS)


def cached_graphs(model, out):
    """each cached LM graph once more on its own (same inputs, same ring slots): its plan is then the last one"""
    for which, name in GRAPHS:
        g = L.moshi_hot_graph(model.m, which)
        if g:
            assert L.ggml_backend_graph_compute(model.be, g) == 0
            out.append((name, counters(model)))
    model.free()
    return out


def moshika(sampled):
    # moshika's widths with two layers: the in_proj + attention merge and the paired gate need the real widths (tests/test_attn_fold.py)
    cfg = su.lm_only(hu.hot.moshika(L))
    cfg.num_layers = 2
    if sampled:
        cfg.temp, cfg.temp_text = 0.8, 0.7
    m = hu.Model("hip", cfg)
    out = []
    for k in range(2):
        m.lm_step([0] * 8)
        out.append((f"step {k}", counters(m)))
    return cached_graphs(m, out)


def tiny(context=RING):
    cfg = su.lm_only(hu.hot.tiny(L, linear_type=Q4_K, embed_type=Q4_0, context=context))
    cfg.update_scale = 1.0 / 256
    return cfg


def lockstep_streams():
    cfg = tiny()                                           # tests/test_streams_gpu.py
    s = su.Streams("hip", cfg, 2)
    out = []
    for k, fr in enumerate(su.stream_codes(cfg, 2, 2, seed=2)):
        s.step(fr)
        out.append((f"step {k}", counters(s)))
    return cached_graphs(s, out)


def slots_prefill_fork():
    cfg = tiny(context=24)                                 # tests/test_slot_prefill_gpu.py, tests/test_slot_state_gpu.py
    s = ss.Slots("hip", cfg, 2)
    codes = pu.live_codes(cfg, 2, seed=81)
    out = []
    assert s.open(0) == 0
    assert s.prefill([(0, pu.history(cfg, 3, seed=60))], 8) == 3
    out.append(("prefill pass", counters(s)))
    pu.step_all(s, {0: codes[0]})
    out.append(("step 0", counters(s)))
    assert s.fork(0, 1) == 0
    out.append(("fork", counters(s)))
    pu.step_all(s, {0: codes[1], 1: codes[1]})
    out.append(("step 1", counters(s)))
    return cached_graphs(s, out)


def stt_slots():
    cfg = hu.hot.tiny_stt(L, linear_type=Q4_K, embed_type=Q4_0, context=RING)   # tests/test_stt_slots_gpu.py
    cfg.update_scale = 1.0 / 256
    s = st.Slots("hip", cfg, 2)
    out = []
    for b in range(2):
        assert s.open(b) == 0
    for k, fr in enumerate(sl.slot_codes(cfg, 2, 2, seed=2)):
        s.step(fr)
        out.append((f"step {k}", counters(s)))
    return cached_graphs(s, out)


def tts_slots():
    cfg = tts_cfg()
    s = tu.Slots("hip", cfg, 2)
    n = 2 + cfg.delay_steps                                # the Depth graph first runs in frame delay_steps
    out = []
    for b in range(2):
        assert s.set_conditions(b, 4 + b) == 0
        assert s.open(b) == 0
    streams = [tu.text_stream(cfg, b, n) for b in range(2)]
    for k in range(n):
        s.step([streams[b][k] for b in range(2)])
        out.append((f"step {k}", counters(s)))
    return cached_graphs(s, out)


def wide_slots():
    cfg = sp.sampled(tiny())                               # tests/test_wide_streams_gpu.py: the 3-tile mat-mul and the raised sampler width
    cfg.wide_streams = 1
    B = 33
    s = sp.Slots("hip", cfg, B)
    out = []
    for b in range(B):
        assert s.open(b) == 0
        assert s.set_sampling(b, 4000 + 17 * b, 0.6 + 0.1 * (b % 5), 0.5 + 0.1 * (b % 4), 20 if b % 3 else 6, 25 if b % 3 != 1 else 4) == 0
    for k, fr in enumerate(sl.slot_codes(cfg, B, 2, seed=2)):
        s.step(fr)
        out.append((f"step {k}", counters(s)))
    return cached_graphs(s, out)


def slots_prefill_long():
    cfg = tiny(context=24)                                 # tests/test_slot_prefill_long_gpu.py
    s = lu.Slots("hip", cfg, 2)
    out = []
    for b in range(2):
        assert s.open(b) == 0
        s.set_fill(b, 24)                                  # the ring's end: every provided row is ring-ordered
    assert s.prefill_long([(b, lu.history(cfg, 3, seed=60 + b)) for b in range(2)], 8) == 6
    out.append(("pass of two ring-ordered pieces", counters(s)))   # two rows jobs, one rows launch per layer
    assert s.close(1) == 0 and s.open(1) == 0 and s.position(1) == 0
    assert s.prefill_long([(0, lu.history(cfg, 2, seed=62)), (1, lu.history(cfg, 3, seed=63))], 8) == 5
    out.append(("mixed pass", counters(s)))                # a rows job (slot 0, two rows from 27) and a three-row block (slot 1 from 0)
    codes = lu.live_codes(cfg, 1, seed=81)
    lu.step_all(s, {0: codes[0], 1: codes[0]})
    out.append(("step 0", counters(s)))
    return cached_graphs(s, out)


def tts_cfg():
    cfg = tu.tts_cfg(linear_type=Q4_K, embed_type=Q4_0, layers=2, cross_len=5)   # tests/test_tts_slots_gpu.py, tests/test_tts_replay_gpu.py
    cfg.context = RING
    cfg.update_scale = 1.0 / 256
    return cfg


def tts_slots_replay():
    cfg = tts_cfg()
    s = ru.Slots("hip", cfg, 2)
    out = []
    for b in range(2):
        assert s.set_conditions(b, 4 + b) == 0
        assert s.open(b) == 0
    assert s.replay([(0, ru.history(cfg, 3, seed=60)), (1, ru.history(cfg, 2, seed=61))], 8) == 5
    out.append(("replay pass", counters(s)))               # cross-attention jobs and column blocks
    s.step([tu.text_stream(cfg, b, 1)[0] for b in range(2)])
    out.append(("step 0", counters(s)))
    return cached_graphs(s, out)


def persona_slots():
    cfg = pp.make_cfg(layers=2, linear_type=Q4_K, embed_type=Q4_0)   # tests/test_persona_slots_gpu.py
    cfg.update_scale = 1.0 / 256
    s = pp.Slots("hip", cfg, 2)
    voiced = pp.Persona(cfg, 11, n_voice=2, vtype=F32, cache=True, n_text=1, silence=1)
    mute = pp.Persona(cfg, 12, n_voice=0, vtype=F32, cache=False)
    out = []
    for b in range(2):
        assert s.open(b) == 0
    assert s.persona([(0, voiced), (1, mute)], 0) == voiced.rows + mute.rows   # one pass: voice | tokens | tokens
    out.append(("persona pass", counters(s)))
    s.step(pp.live_codes(cfg, 2, seed=21))
    out.append(("step 0", counters(s)))
    return cached_graphs(s, out)


def tts_single():
    cfg = tts_cfg()
    m = hu.Model("hip", cfg)
    hu.set_conditions(m, cfg)
    n = 1 + cfg.delay_steps                                # the Depth graph first runs in frame delay_steps
    texts = tu.text_stream(cfg, 0, n)
    hu.set_text_hook(m, lambda offset, sampled: texts[offset])
    out = []
    for k in range(n):
        m.lm_step_n([])
        out.append((f"step {k}", counters(m)))
    return cached_graphs(m, out)


def single_prefill():
    cfg = tiny()
    m = hu.Model("hip", cfg)
    m.prefill(pu.history(cfg, 5, seed=60), 8)              # one block of five rows: the T > 4 launches of a whole ring, not a column
    out = [("prefill", counters(m))]
    m.lm_step([0] * (cfg.n_q - cfg.dep_q))
    out.append(("step 0", counters(m)))
    return cached_graphs(m, out)


def codec_single():
    cfg = du.cfg_of()                                      # tests/test_codec_slots_gpu.py's single-stream reference, with the encoder beside it
    cfg.enable_mimi_encoder = 1
    m = hu.Model("hip", cfg)
    m.mimi_encode(eu.pcm(900)[0])                          # single-column conv, dw-conv, VQ levels and the chained VQ
    out = [("encode", counters(m))]
    m.mimi_decode(du.codes(900)[0].tolist())               # single-column code gather, convtr, dw-convtr
    out.append(("decode", counters(m)))
    m.free()
    return out


def codec_slots(half):
    """the codec graphs have no cached-graph accessor: the counters after every call that computes one"""
    s = half.make("hip", 2)                                # tests/test_codec_slot_state_gpu.py
    fr = half.frames(900, 2)
    out = []
    for b in range(2):
        assert s.open(b) == 0
    for k in range(2):
        half.step(s, {0: fr[k], 1: fr[k]})
        out.append((f"frame {k}", counters(s)))
    assert s.close(1) == 0 and cs.fork(s, 0, 1) == 0
    out.append(("fork", counters(s)))
    blob = cs.save(s, 0)
    out.append(("save", counters(s)))
    assert s.close(1) == 0 and cs.load(s, 1, blob) == 0
    out.append(("load", counters(s)))
    s.free()
    return out


CASES = {
    "moshika_greedy": lambda: moshika(False),
    "moshika_sampled": lambda: moshika(True),
    "lockstep_streams_b2": lockstep_streams,
    "slots_b2_prefill_fork": slots_prefill_fork,
    "stt_slots_b2": stt_slots,
    "tts_slots_b2": tts_slots,
    "wide_slots_b33": wide_slots,
    "slots_b2_prefill_long": slots_prefill_long,
    "tts_slots_b2_replay": tts_slots_replay,
    "persona_slots_b2": persona_slots,
    "tts_single": tts_single,
    "single_prefill_t5": single_prefill,
    "codec_single": codec_single,
    "decoder_slots_b2": lambda: codec_slots(cs.HALVES[0]),
    "encoder_slots_b2": lambda: codec_slots(cs.HALVES[1]),
}
