#!/usr/bin/env python3
"""Windows at given onsets against the entries a caller had before.

For each case (one MI355X, one process, HIP events, the candidates alternating within every repeat):
  (a) forward_windows_at_torch on the whole array with the onset list already on the device (what
      a C caller of net_model_compute_windows_at runs: layer 1 once per sample, then layers 2-5 at
      the onsets); the multi cases also time forward_windows_multi_torch, which builds and copies
      the list on every call (a_py);
  (b) one forward_windows_torch call per recording (multi cases);
  (c) forward_epochs_torch on the same onsets (layer 1 per epoch);
  (d) forward_windows_torch at the same regular hop (the regular case).
All logit rows of the candidates are compared with (a)'s.  The regular case is gated: (a)'s median
must lie within 3 % above (d)'s plus the spread (max - min) of (d)'s samples.  One JSON line per
case goes to <out-dir>/windows_at_<name>.json and to stdout.  There is no CPU path: without a GPU
this fails.

  python tools/bench_windows_at.py [--cases multi_p64,multi_b22,random_b22,regular_b22]
                                   [--windows 65536] [--reps 7] [--warmup 2]
                                   [--variant canonical|plain_bn] [--out-dir profiles]
"""
from bench_common import main, medians, min_max, time_alternating

CASES = {  # name: (kind, C, T, N, hop, recordings, samples per recording)
    "multi_p64": ("multi", 64, 480, 2, 8, 64, 20000),
    "multi_b22": ("multi", 22, 1125, 4, 8, 12, 96000),
    "random_b22": ("random", 22, 1125, 4, 8, 1, 0),   # --windows random onsets, eight samples per window
    "regular_b22": ("regular", 22, 1125, 4, 8, 1, 0),  # --windows onsets w hop
}
GATE = 0.03  # the same-box A/B noise


def run_case(name, W, reps, warmup, variant, seed=2026):
    import numpy as np
    import torch

    from mibminet import lib
    from mibminet.params import ParamSet

    kind, C, T, N, hop, R, Lr = CASES[name]
    ps = ParamSet.synthetic(seed=seed, C=C, T=T, N=N, reorder_bn=variant != "plain_bn")
    lib.params_load(ps)
    g = torch.Generator(device="cuda").manual_seed(seed)
    rng = np.random.default_rng(seed)
    if kind == "multi":
        lengths = [int(v) for v in Lr + rng.integers(-Lr // 13, Lr // 13 + 1, size=R)]  # unequal
        onsets_np, first = lib.windows_multi_onsets(lengths, hop)
        onsets = torch.from_numpy(onsets_np).cuda()
    elif kind == "random":
        lengths = [hop * W + T]
        onsets = torch.randint(0, lengths[0] - T + 1, (W,), dtype=torch.int64, device="cuda", generator=g)
    else:
        lengths = [T + (W - 1) * hop]
        onsets = torch.arange(W, dtype=torch.int64, device="cuda") * hop
    L = sum(lengths)
    x = torch.randint(-128, 128, (C, L), dtype=torch.int8, device="cuda", generator=g)
    fns = {"a": lambda: lib.forward_windows_at_torch(x, onsets, check=False)}
    if kind == "multi":
        starts = np.concatenate(([0], np.cumsum(lengths))).tolist()
        recs = [x[:, starts[r]: starts[r + 1]].contiguous() for r in range(R)]
        fns["a_py"] = lambda: lib.forward_windows_multi_torch((x, lengths), hop)[0]
        fns["b"] = lambda: torch.cat([lib.forward_windows_torch(t, hop) for t in recs], dim=0)
    if kind in ("multi", "random"):
        fns["c"] = lambda: lib.forward_epochs_torch(x, onsets, check=False)
    if kind == "regular":
        fns["d"] = lambda: lib.forward_windows_torch(x, hop)
    ya = fns["a"]()
    mismatches = {k: int((f() != ya).any(dim=1).sum().item()) for k, f in fns.items() if k != "a"}
    ms = time_alternating(fns, reps, warmup)
    med = medians(ms)
    res = {
        "name": name, "kind": kind, "C": C, "T": T, "N": N, "hop": hop, "recordings": R, "samples": L,
        "windows": int(onsets.numel()), "variant": variant, "path": lib.params_info()["path"], "reps": reps, "warmup": warmup,
        "ms": {k: round(v, 4) for k, v in med.items()},
        "ms_min_max": {k: min_max(v) for k, v in ms.items()},
        "over_a": {k: round(v / med["a"], 4) for k, v in med.items() if k != "a"},
        "windows_per_s": round(int(onsets.numel()) / med["a"] * 1e3),
        "recording_bytes": C * L, "workspace_bytes": lib.windows_workspace(L),
        "mismatched_rows": mismatches, "device": torch.cuda.get_device_name(0),
    }
    if kind == "multi":
        res["lengths_min_max"] = [min(lengths), max(lengths)]
    if kind == "regular":
        limit = (1 + GATE) * med["d"] + (max(ms["d"]) - min(ms["d"]))
        res["gate_ms"] = round(limit, 4)
        res["gate_ok"] = bool(med["a"] <= limit)
    return res


def failures(res):
    return sum(res["mismatched_rows"].values()) + (0 if res.get("gate_ok", True) else 1)


if __name__ == "__main__":
    main(__doc__, CASES, run_case, "windows", "windows_at", failures)
