"""-m gpu: the plans of every model kind, pinned graph by graph. Each case (tests/plan_shape_util.py) builds one two-layer synthetic model - moshika's
widths for the single-stream cases, the tiny configurations whose plans the *_gpu.py files of each kind already assert for the others - takes two
steps (the tts case two more, until its Depth graph has run) and reads the plan counters after every call that computes graphs; then each cached LM
graph is computed once more on its own and read again, so the Temporal plan and the Depth plan are both seen. Five cases take the batched passes
instead, for the attention forms no live step shows: slot prefill past the ring's end (a pass of two ring-ordered pieces, then a rows job beside a
three-row block), a tts replay pass (cross-attention jobs and column blocks), a PersonaPlex persona pass, a single-stream tts model (cross-attention
at B = 1) and a single-stream prefill of five frames (a block of more than 4 rows on whole rings) - each followed by one live step. Three cases are
the codec's: a codec-only single-stream model (one encode frame, one decode frame: the single-column conv, convtr, dw-convtr, VQ-level and chained VQ
paths) and decoder slots and encoder slots at B = 2 (two frames, then a fork, a save and a load). Their graphs have no cached-graph accessor, so the
counters are read after each call only.

The counters are exact: what the planner fuses, chains and launches for a given graph is a property of the planner alone. EXPECTED - the twelve LM
cases and their first 21 counters - was recorded by running this file's body (tests/microbench/plan_dump_shapes.py prints it) against the library built
from commit 612970c, the last one before the attention matchers were put on one shared block walk - never from the library under test. The first
twelve values of the first seven cases came out as they were recorded from commit f3717a4, the last one before build_plan was split into passes. The
three codec cases, and the last six counters of every row, were recorded the same way from commit 7b17597, the last one before the codec-slot
matchers and the snapshot graphs were folded into the forms they were copied from; the first 21 counters of the twelve older cases came out of that
run as they stood. A change of a plan is a change of this table, made on purpose."""
import pytest

import plan_shape_util as ps

pytestmark = pytest.mark.gpu

# per case: (what was computed last, counters in the order of plan_shape_util.COUNTERS: kernels, fused nodes, nodes, chained mat-vecs, step programs,
# VQ levels chained, attention-block launches, attention-block jobs, generic attention nodes, ring-copy launches, ring-copy jobs, attention_folds_planned,
# then attention-rows launches, jobs, rows, cross-attention-block launches, jobs, float batched mat-muls, float-accumulating ones, pass-input launches, rows,
# then convtr column groups, codec attention launches, VQ column levels, code-gather columns, state-copy launches, state-copy jobs)
EXPECTED = {
    "moshika_greedy": [
        ("step 0", (1, 1641, 1954, 208, 1, 0, 0, 0, 0, 0, 0, 2,   0, 0, 0, 0, 0, 0, 0, 0, 0,   0, 0, 0, 0, 0, 0)),
        ("step 1", (1, 1641, 1954, 208, 1, 0, 0, 0, 0, 0, 0, 2,   0, 0, 0, 0, 0, 0, 0, 0, 0,   0, 0, 0, 0, 0, 0)),
        ("temporal graph", (11, 185, 191, 0, 0, 0, 0, 0, 0, 0, 0, 2,   0, 0, 0, 0, 0, 0, 0, 0, 0,   0, 0, 0, 0, 0, 0)),
        ("depth graph", (1, 1641, 1954, 208, 1, 0, 0, 0, 0, 0, 0, 2,   0, 0, 0, 0, 0, 0, 0, 0, 0,   0, 0, 0, 0, 0, 0)),
    ],
    "moshika_sampled": [
        ("step 0", (1, 1753, 2066, 216, 1, 0, 0, 0, 0, 0, 0, 2,   0, 0, 0, 0, 0, 0, 0, 0, 0,   0, 0, 0, 0, 0, 0)),
        ("step 1", (1, 1753, 2066, 216, 1, 0, 0, 0, 0, 0, 0, 2,   0, 0, 0, 0, 0, 0, 0, 0, 0,   0, 0, 0, 0, 0, 0)),
        ("temporal graph", (12, 199, 205, 0, 0, 0, 0, 0, 0, 0, 0, 2,   0, 0, 0, 0, 0, 0, 0, 0, 0,   0, 0, 0, 0, 0, 0)),
        ("depth graph", (1, 1753, 2066, 216, 1, 0, 0, 0, 0, 0, 0, 2,   0, 0, 0, 0, 0, 0, 0, 0, 0,   0, 0, 0, 0, 0, 0)),
    ],
    "lockstep_streams_b2": [
        ("step 0", (49, 210, 278, 0, 0, 0, 0, 0, 0, 0, 0, 0,   0, 0, 0, 0, 0, 0, 0, 0, 0,   0, 0, 0, 0, 0, 0)),
        ("step 1", (49, 210, 278, 0, 0, 0, 0, 0, 0, 0, 0, 0,   0, 0, 0, 0, 0, 0, 0, 0, 0,   0, 0, 0, 0, 0, 0)),
        ("temporal graph", (17, 149, 165, 0, 0, 0, 0, 0, 0, 0, 0, 0,   0, 0, 0, 0, 0, 0, 0, 0, 0,   0, 0, 0, 0, 0, 0)),
        ("depth graph", (49, 210, 278, 0, 0, 0, 0, 0, 0, 0, 0, 0,   0, 0, 0, 0, 0, 0, 0, 0, 0,   0, 0, 0, 0, 0, 0)),
    ],
    "slots_b2_prefill_fork": [
        ("prefill pass", (16, 154, 169, 0, 0, 0, 4, 2, 0, 0, 0, 0,   0, 0, 0, 0, 0, 0, 0, 0, 0,   0, 0, 0, 0, 0, 0)),
        ("step 0", (49, 210, 278, 0, 0, 0, 0, 0, 0, 0, 0, 0,   0, 0, 0, 0, 0, 0, 0, 0, 0,   0, 0, 0, 0, 0, 0)),
        ("fork", (2, 4, 15, 0, 0, 0, 0, 0, 0, 1, 4, 0,   0, 0, 0, 0, 0, 0, 0, 0, 0,   0, 0, 0, 0, 0, 0)),
        ("step 1", (49, 210, 278, 0, 0, 0, 0, 0, 0, 0, 0, 0,   0, 0, 0, 0, 0, 0, 0, 0, 0,   0, 0, 0, 0, 0, 0)),
        ("temporal graph", (17, 147, 164, 0, 0, 0, 0, 0, 0, 0, 0, 0,   0, 0, 0, 0, 0, 0, 0, 0, 0,   0, 0, 0, 0, 0, 0)),
        ("depth graph", (49, 210, 278, 0, 0, 0, 0, 0, 0, 0, 0, 0,   0, 0, 0, 0, 0, 0, 0, 0, 0,   0, 0, 0, 0, 0, 0)),
    ],
    "stt_slots_b2": [
        ("step 0", (18, 165, 182, 0, 0, 0, 0, 0, 0, 0, 0, 0,   0, 0, 0, 0, 0, 0, 0, 0, 0,   0, 0, 0, 0, 0, 0)),
        ("step 1", (18, 165, 182, 0, 0, 0, 0, 0, 0, 0, 0, 0,   0, 0, 0, 0, 0, 0, 0, 0, 0,   0, 0, 0, 0, 0, 0)),
        ("temporal graph", (18, 165, 182, 0, 0, 0, 0, 0, 0, 0, 0, 0,   0, 0, 0, 0, 0, 0, 0, 0, 0,   0, 0, 0, 0, 0, 0)),
    ],
    "tts_slots_b2": [
        ("step 0", (54, 152, 209, 0, 0, 0, 0, 0, 0, 0, 0, 0,   0, 0, 0, 0, 0, 0, 0, 0, 0,   0, 0, 0, 0, 0, 0)),
        ("step 1", (54, 152, 209, 0, 0, 0, 0, 0, 0, 0, 0, 0,   0, 0, 0, 0, 0, 0, 0, 0, 0,   0, 0, 0, 0, 0, 0)),
        ("step 2", (140, 560, 749, 0, 0, 0, 0, 0, 0, 0, 0, 0,   0, 0, 0, 0, 0, 0, 0, 0, 0,   0, 0, 0, 0, 0, 0)),
        ("step 3", (140, 560, 749, 0, 0, 0, 0, 0, 0, 0, 0, 0,   0, 0, 0, 0, 0, 0, 0, 0, 0,   0, 0, 0, 0, 0, 0)),
        ("temporal graph", (54, 152, 209, 0, 0, 0, 0, 0, 0, 0, 0, 0,   0, 0, 0, 0, 0, 0, 0, 0, 0,   0, 0, 0, 0, 0, 0)),
        ("depth graph", (140, 560, 749, 0, 0, 0, 0, 0, 0, 0, 0, 0,   0, 0, 0, 0, 0, 0, 0, 0, 0,   0, 0, 0, 0, 0, 0)),
    ],
    "wide_slots_b33": [
        ("step 0", (48, 263, 329, 0, 0, 0, 0, 0, 0, 0, 0, 0,   0, 0, 0, 0, 0, 0, 0, 0, 0,   0, 0, 0, 0, 0, 0)),
        ("step 1", (48, 263, 329, 0, 0, 0, 0, 0, 0, 0, 0, 0,   0, 0, 0, 0, 0, 0, 0, 0, 0,   0, 0, 0, 0, 0, 0)),
        ("temporal graph", (17, 164, 181, 0, 0, 0, 0, 0, 0, 0, 0, 0,   0, 0, 0, 0, 0, 0, 0, 0, 0,   0, 0, 0, 0, 0, 0)),
        ("depth graph", (48, 263, 329, 0, 0, 0, 0, 0, 0, 0, 0, 0,   0, 0, 0, 0, 0, 0, 0, 0, 0,   0, 0, 0, 0, 0, 0)),
    ],
    "slots_b2_prefill_long": [
        ("pass of two ring-ordered pieces", (21, 696, 734, 0, 0, 0, 0, 0, 0, 0, 0, 0,   2, 4, 12, 0, 0, 0, 0, 0, 0,   0, 0, 0, 0, 0, 0)),
        ("mixed pass", (22, 372, 398, 0, 0, 0, 4, 2, 0, 0, 0, 0,   2, 2, 4, 0, 0, 0, 0, 0, 0,   0, 0, 0, 0, 0, 0)),
        ("step 0", (49, 210, 278, 0, 0, 0, 0, 0, 0, 0, 0, 0,   0, 0, 0, 0, 0, 0, 0, 0, 0,   0, 0, 0, 0, 0, 0)),
        ("temporal graph", (17, 147, 164, 0, 0, 0, 0, 0, 0, 0, 0, 0,   0, 0, 0, 0, 0, 0, 0, 0, 0,   0, 0, 0, 0, 0, 0)),
        ("depth graph", (49, 210, 278, 0, 0, 0, 0, 0, 0, 0, 0, 0,   0, 0, 0, 0, 0, 0, 0, 0, 0,   0, 0, 0, 0, 0, 0)),
    ],
    "tts_slots_b2_replay": [
        ("replay pass", (61, 273, 362, 0, 0, 0, 4, 4, 0, 0, 0, 0,   0, 0, 0, 2, 4, 0, 0, 0, 0,   0, 0, 0, 0, 0, 0)),
        ("step 0", (140, 560, 749, 0, 0, 0, 0, 0, 0, 0, 0, 0,   0, 0, 0, 0, 0, 0, 0, 0, 0,   0, 0, 0, 0, 0, 0)),
        ("temporal graph", (54, 152, 209, 0, 0, 0, 0, 0, 0, 0, 0, 0,   0, 0, 0, 0, 0, 0, 0, 0, 0,   0, 0, 0, 0, 0, 0)),
        ("depth graph", (140, 560, 749, 0, 0, 0, 0, 0, 0, 0, 0, 0,   0, 0, 0, 0, 0, 0, 0, 0, 0,   0, 0, 0, 0, 0, 0)),
    ],
    "persona_slots_b2": [
        ("persona pass", (19, 296, 352, 0, 0, 0, 4, 4, 0, 0, 0, 0,   0, 0, 0, 0, 0, 0, 0, 1, 12,   0, 0, 0, 0, 0, 0)),
        ("step 0", (257, 1120, 1474, 0, 0, 0, 0, 0, 0, 0, 0, 0,   0, 0, 0, 0, 0, 0, 0, 0, 0,   0, 0, 0, 0, 0, 0)),
        ("temporal graph", (17, 177, 194, 0, 0, 0, 0, 0, 0, 0, 0, 0,   0, 0, 0, 0, 0, 0, 0, 0, 0,   0, 0, 0, 0, 0, 0)),
        ("depth graph", (257, 1120, 1474, 0, 0, 0, 0, 0, 0, 0, 0, 0,   0, 0, 0, 0, 0, 0, 0, 0, 0,   0, 0, 0, 0, 0, 0)),
    ],
    "tts_single": [
        ("step 0", (24, 179, 206, 4, 0, 0, 0, 0, 0, 0, 0, 0,   0, 0, 0, 0, 0, 0, 0, 0, 0,   0, 0, 0, 0, 0, 0)),
        ("step 1", (24, 179, 206, 4, 0, 0, 0, 0, 0, 0, 0, 0,   0, 0, 0, 0, 0, 0, 0, 0, 0,   0, 0, 0, 0, 0, 0)),
        ("step 2", (76, 568, 717, 64, 0, 0, 0, 0, 0, 0, 0, 0,   0, 0, 0, 0, 0, 0, 0, 0, 0,   0, 0, 0, 0, 0, 0)),
        ("temporal graph", (24, 179, 206, 4, 0, 0, 0, 0, 0, 0, 0, 0,   0, 0, 0, 0, 0, 0, 0, 0, 0,   0, 0, 0, 0, 0, 0)),
        ("depth graph", (76, 568, 717, 64, 0, 0, 0, 0, 0, 0, 0, 0,   0, 0, 0, 0, 0, 0, 0, 0, 0,   0, 0, 0, 0, 0, 0)),
    ],
    "single_prefill_t5": [
        ("prefill", (14, 150, 162, 0, 0, 0, 0, 0, 0, 0, 0, 0,   0, 0, 0, 0, 0, 0, 0, 0, 0,   0, 0, 0, 0, 0, 0)),
        ("step 0", (14, 220, 266, 28, 0, 0, 0, 0, 0, 0, 0, 0,   0, 0, 0, 0, 0, 0, 0, 0, 0,   0, 0, 0, 0, 0, 0)),
        ("temporal graph", (10, 153, 161, 4, 0, 0, 0, 0, 0, 0, 0, 0,   0, 0, 0, 0, 0, 0, 0, 0, 0,   0, 0, 0, 0, 0, 0)),
        ("depth graph", (14, 220, 266, 28, 0, 0, 0, 0, 0, 0, 0, 0,   0, 0, 0, 0, 0, 0, 0, 0, 0,   0, 0, 0, 0, 0, 0)),
    ],
    "codec_single": [
        ("encode", (24, 833, 844, 40, 1, 7, 0, 0, 0, 0, 0, 0,   0, 0, 0, 0, 0, 0, 0, 0, 0,   0, 0, 0, 0, 0, 0)),
        ("decode", (24, 726, 753, 40, 1, 0, 0, 0, 0, 0, 0, 0,   0, 0, 0, 0, 0, 0, 0, 0, 0,   0, 0, 0, 0, 0, 0)),
    ],
    "decoder_slots_b2": [
        ("frame 0", (224, 536, 798, 0, 0, 0, 0, 0, 0, 0, 0, 0,   0, 0, 0, 0, 0, 0, 0, 0, 0,   4, 8, 0, 0, 0, 0)),
        ("frame 1", (224, 536, 798, 0, 0, 0, 0, 0, 0, 0, 0, 0,   0, 0, 0, 0, 0, 0, 0, 0, 0,   4, 8, 0, 0, 0, 0)),
        ("fork", (2, 27, 81, 0, 0, 0, 0, 0, 0, 1, 16, 0,   0, 0, 0, 0, 0, 0, 0, 0, 0,   0, 0, 0, 0, 1, 11)),
        ("save", (2, 27, 81, 0, 0, 0, 0, 0, 0, 1, 16, 0,   0, 0, 0, 0, 0, 0, 0, 0, 0,   0, 0, 0, 0, 1, 11)),
        ("load", (2, 27, 81, 0, 0, 0, 0, 0, 0, 1, 16, 0,   0, 0, 0, 0, 0, 0, 0, 0, 0,   0, 0, 0, 0, 1, 11)),
    ],
    "encoder_slots_b2": [
        ("frame 0", (212, 669, 870, 0, 0, 0, 0, 0, 0, 0, 0, 0,   0, 0, 0, 0, 0, 0, 0, 0, 0,   0, 8, 8, 2, 0, 0)),
        ("frame 1", (212, 669, 870, 0, 0, 0, 0, 0, 0, 0, 0, 0,   0, 0, 0, 0, 0, 0, 0, 0, 0,   0, 8, 8, 2, 0, 0)),
        ("fork", (2, 27, 81, 0, 0, 0, 0, 0, 0, 1, 16, 0,   0, 0, 0, 0, 0, 0, 0, 0, 0,   0, 0, 0, 0, 1, 11)),
        ("save", (2, 27, 81, 0, 0, 0, 0, 0, 0, 1, 16, 0,   0, 0, 0, 0, 0, 0, 0, 0, 0,   0, 0, 0, 0, 1, 11)),
        ("load", (2, 27, 81, 0, 0, 0, 0, 0, 0, 1, 16, 0,   0, 0, 0, 0, 0, 0, 0, 0, 0,   0, 0, 0, 0, 1, 11)),
    ],
}

@pytest.mark.parametrize("case", list(ps.CASES))
def test_plan_counters_of_every_graph(case):
    got = ps.CASES[case]()
    for what, c in got:
        print(f"{case}: {what}: {c}")
    want = EXPECTED[case]
    assert [w for w, _ in got] == [w for w, _ in want]
    for (what, c), (_, w) in zip(got, want):
        assert c == w, f"{case}, {what}: " + ", ".join(f"{n} {a} (was {b})" for n, a, b in zip(ps.COUNTERS, c, w) if a != b)
