#!/usr/bin/env python3
"""Sliding windows over a recording against the batched forward on the same windows.

For each case (one MI355X, one process, HIP events, the three alternating within every repeat):
  (a) forward_windows_torch on the recording (layer 1 once per sample, then layers 2-5 per window);
  (b) forward_ct_torch on the windows materialised beforehand ([W][C][T] already in memory);
  (c) the materialisation (unfold + contiguous copy on the device) plus (b): what a caller without
      the windows entry pays.
All logits of (a) are compared with (b).  One JSON line per case goes to
<out-dir>/windows_<name>.json and to stdout.  There is no CPU path: without a GPU this fails.

  python tools/bench_windows.py [--cases b22_h1,b22_h8,b22_h125,p64_h8] [--windows 65536]
                                [--reps 7] [--warmup 2] [--variant canonical|plain_bn]
                                [--out-dir profiles]
"""
from bench_common import main, medians, min_max, time_alternating

CASES = {  # name: (C, T, N, hop)
    "b22_h1": (22, 1125, 4, 1),
    "b22_h8": (22, 1125, 4, 8),
    "b22_h125": (22, 1125, 4, 125),
    "p64_h8": (64, 480, 2, 8),
}


def run_case(name, W, reps, warmup, variant, seed=2026):
    import torch

    from mibminet import lib
    from mibminet.params import ParamSet

    C, T, N, hop = CASES[name]
    ps = ParamSet.synthetic(seed=seed, C=C, T=T, N=N, reorder_bn=variant != "plain_bn")
    lib.params_load(ps)
    L = T + (W - 1) * hop
    assert lib.windows_count(L, hop) == W
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randint(-128, 128, (C, L), dtype=torch.int8, device="cuda", generator=g)

    def materialise():
        return x.unfold(1, T, hop).permute(1, 0, 2).contiguous()  # [W][C][T]

    wins = materialise()

    def a():
        return lib.forward_windows_torch(x, hop)

    def b():
        return lib.forward_ct_torch(wins)

    def c():
        return lib.forward_ct_torch(materialise())

    ya, yb = a(), b()
    mismatches = int((ya != yb).any(dim=1).sum().item())
    fns = {"a": a, "b": b, "c": c}
    ms = time_alternating(fns, reps, warmup)
    med = medians(ms)
    return {
        "name": name, "C": C, "T": T, "N": N, "hop": hop, "windows": W, "samples": L,
        "variant": variant, "path": lib.params_info()["path"], "reps": reps, "warmup": warmup,
        "ms_windows": round(med["a"], 4), "ms_batch_ct": round(med["b"], 4),
        "ms_materialise_batch_ct": round(med["c"], 4),
        "ms_windows_min_max": min_max(ms["a"]),
        "ms_batch_ct_min_max": min_max(ms["b"]),
        "windows_per_s": round(W / med["a"] * 1e3), "batch_ct_per_s": round(W / med["b"] * 1e3),
        "recording_bytes": C * L, "materialised_bytes": W * C * T, "workspace_bytes": lib.windows_workspace(L),
        "mismatched_windows": mismatches, "device": torch.cuda.get_device_name(0),
    }


if __name__ == "__main__":
    main(__doc__, CASES, run_case, "windows", "windows", lambda res: res["mismatched_windows"])
