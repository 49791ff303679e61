"""float_streams_bench.py with one more setting: `fast` = MI355X_MMF=2, the float-accumulating BF16 mat-mul (k_mm_f32acc_batched) as the
starting mode of the child's handle, alternated with `default` (the f64-MFMA mat-mul) on the same box. Method, children, time limits and output are
float_streams_bench.py's own (moshika BF16, lockstep streams, context 750, one fresh child per line, 5 warm-up frames + 3 rounds of 40 frames - 10 at
B = 64 - median round; nothing is started after a failure). A `fast` line reports float_batched_mms_in_temporal_plan = 0 (that counter keeps counting
the f64 launches only) with the Temporal plan's launch count unchanged. With --out, every A/B entry of the file also gets fast's ratio to default.
    python tests/microbench/float_acc_streams_bench.py [--out FILE] [--reps N] [--settings default,fast] [--frames N] [--rounds N] [B ...]"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import float_streams_bench as base  # noqa: E402

base.SETTINGS["fast"] = {"MI355X_MMF": "2"}


def main():
    args = sys.argv[1:]
    if "--settings" not in args:
        args = ["--settings", "default,fast"] + args
    sys.argv = [sys.argv[0]] + args
    base.main()
    if "--out" in args:
        out = args[args.index("--out") + 1]
        with open(out) as f:
            result = json.load(f)
        for ab in result["ab"]:
            med = ab["median_ms_per_step"]
            if "default" in med and "fast" in med:
                ab["fast_over_default"] = round(med["fast"] / med["default"], 3)
                print(json.dumps({"n_streams": ab["n_streams"], "fast_over_default": ab["fast_over_default"]}), flush=True)
        with open(out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
