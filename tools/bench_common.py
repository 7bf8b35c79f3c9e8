"""What bench_windows.py, bench_windows_at.py, bench_epochs.py, bench_bank.py, bench_windows_bank.py and bench_streams.py share: the alternating HIP-event
timing loop and its summaries, the command line, and the loop that runs the cases, writes one JSON
line per case and turns mismatches into the exit status.  No tool of its own."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mi-bminet_amd"))


def time_alternating(fns, reps, warmup):
    """{key: [ms per repeat]} of the candidates ``fns`` ({key: callable}), all of them run in turn
    within every warm-up round and every timed repeat, each timed call between two HIP events."""
    import torch

    for _ in range(warmup):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(reps):
        for k, f in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    return ms


def medians(ms):
    return {k: statistics.median(v) for k, v in ms.items()}


def min_max(v):
    return [round(min(v), 4), round(max(v), 4)]


def main(doc, cases, run_case, count, prefix, failures, reps=7, warmup=2):
    """The tools' command line and case loop.  ``count`` names the tool's size option ("windows",
    "epochs"); ``run_case(name, count, reps, warmup, variant)`` returns a case's result, which goes
    as one JSON line to stdout and to <out-dir>/<prefix>_<name>[_<variant>].json; the process exits
    with 1 if ``failures(result)`` is non-zero for any case.  ``reps`` and ``warmup`` are the defaults of
    those options."""
    tool = os.path.basename(sys.argv[0])
    ap = argparse.ArgumentParser(description=doc, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cases", default=",".join(cases))
    ap.add_argument("--" + count, type=int, default=65536)
    ap.add_argument("--reps", type=int, default=reps)
    ap.add_argument("--warmup", type=int, default=warmup)
    ap.add_argument("--variant", default="canonical", choices=("canonical", "plain_bn"),
                    help="plain_bn: a set without REORDER_BN (the plain-BN kernels); the file name then carries it")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args()
    names = [n for n in args.cases.split(",") if n]
    for n in names:
        if n not in cases:
            ap.error(f"unknown case {n} (known: {', '.join(cases)})")
    import torch

    if not torch.cuda.is_available():
        sys.exit(f"{tool} needs a GPU (there is no CPU path)")
    os.makedirs(args.out_dir, exist_ok=True)
    suffix = "" if args.variant == "canonical" else "_" + args.variant
    bad = 0
    for n in names:
        res = run_case(n, getattr(args, count), args.reps, args.warmup, args.variant)
        line = json.dumps(res)
        print(line, flush=True)
        with open(os.path.join(args.out_dir, f"{prefix}_{n}{suffix}.json"), "w") as f:
            f.write(line + "\n")
        bad += failures(res)
        torch.cuda.empty_cache()
    sys.exit(1 if bad else 0)
