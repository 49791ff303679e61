"""MI355X_DUMP_PLAN=1 python tests/microbench/plan_dump_shapes.py [case ..] : plan listings (stderr) and plan counters (stdout) of every model kind at
two layers - moshika single stream greedy and sampled, lockstep streams, slots with a prefill pass and a fork, stt slots, tts slots, wide slots, slot
prefill past the ring's end, a tts replay pass, a persona pass, single-stream tts, a single-stream prefill of five frames, the single-stream codec, decoder slots and encoder slots with a fork, a
save and a load (tests/plan_shape_util.py). Run against two builds (MI355X_LIB), both outputs must be byte-identical when the planner has not changed a plan."""
import os, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")); sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import plan_shape_util as ps
for name in sys.argv[1:] or ps.CASES:
    sys.stderr.write(f"==== {name}\n"); sys.stderr.flush()
    for what, c in ps.CASES[name]():
        print(name, what, " ".join(f"{k.replace('_in_last_plan', '')}={v}" for k, v in zip(ps.COUNTERS, c)), flush=True)
