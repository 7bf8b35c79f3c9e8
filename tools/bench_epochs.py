#!/usr/bin/env python3
"""Epochs read straight from a wider array against gather + batched forward on the same epochs.

For each case (one MI355X, one process, HIP events, the three alternating within every repeat):
  (a) forward_epochs_torch / forward_crop_torch on the source (no intermediate buffer);
  (b) a torch gather to a contiguous [E][C][T] plus forward_ct_torch / forward_f32_torch: what a
      caller without the epochs entry pays;
  (c) that forward alone on epochs already materialised.
All logits of (a) are compared with (c).  One JSON line per case goes to
<out-dir>/epochs_<name>.json and to stdout.  There is no CPU path: without a GPU this fails.

  python tools/bench_epochs.py [--cases b22_rec,p19_crop_i8,p19_crop_f32] [--epochs 65536]
                               [--reps 7] [--warmup 2] [--variant canonical|plain_bn]
                               [--out-dir profiles]
"""
from bench_common import main, medians, min_max, time_alternating

P19 = [0, 2, 4, 8, 10, 12, 14, 21, 23, 29, 31, 33, 35, 37, 40, 41, 47, 54, 61]  # 19 of 64 rows
CASES = {  # name: (kind, C, T, N, rows of the source, float32)
    "b22_rec": ("recording", 22, 1125, 4, 22, False),       # random onsets in a 22-row recording
    "p19_crop_i8": ("crop", 19, 480, 3, 64, False),         # 19 of 64 channels x 480 of [B][64][640]
    "p19_crop_f32": ("crop", 19, 480, 3, 64, True),
}
SCALE = 3.0


def run_case(name, E, reps, warmup, variant, seed=2026):
    import torch

    from mibminet import lib
    from mibminet.params import ParamSet

    kind, C, T, N, R, f32 = CASES[name]
    ps = ParamSet.synthetic(seed=seed, C=C, T=T, N=N, reorder_bn=variant != "plain_bn")
    lib.params_load(ps)
    g = torch.Generator(device="cuda").manual_seed(seed)
    fwd = (lambda t: lib.forward_f32_torch(t, SCALE)) if f32 else lib.forward_ct_torch
    scale = SCALE if f32 else None

    def source(shape):
        if f32:
            return torch.randn(shape, dtype=torch.float32, device="cuda", generator=g) * 1.3
        return torch.randint(-128, 128, shape, dtype=torch.int8, device="cuda", generator=g)

    if kind == "recording":
        L = 8 * E + T  # a recording eight samples per epoch long: the epochs overlap heavily
        x = source((R, L))
        onsets = torch.randint(0, L - T + 1, (E,), dtype=torch.int64, device="cuda", generator=g)

        def gather():  # one indexing pass over the [L - T + 1][C][T] view of every window -> [E][C][T]
            return x.unfold(1, T, 1).permute(1, 0, 2)[onsets].contiguous()

        def a():
            return lib.forward_epochs_torch(x, onsets, scale=scale, check=False)
    else:
        Tf, t0 = 640, 80
        x = source((E, R, Tf))
        rows = torch.tensor(P19, device="cuda")

        def gather():
            return x[:, rows, t0: t0 + T].contiguous()

        def a():
            return lib.forward_crop_torch(x, t0, channels=P19, scale=scale)

    eps = gather()

    def b():
        return fwd(gather())

    def c():
        return fwd(eps)

    ya, yc = a(), c()
    mismatches = int((ya != yc).any(dim=1).sum().item())
    fns = {"a": a, "b": b, "c": c}
    ms = time_alternating(fns, reps, warmup)
    med = medians(ms)
    esz = 4 if f32 else 1
    return {
        "name": name, "kind": kind, "C": C, "T": T, "N": N, "source_rows": R, "float32": f32, "epochs": E,
        "variant": variant, "path": lib.params_info()["path"], "reps": reps, "warmup": warmup,
        "ms_epochs": round(med["a"], 4), "ms_gather_forward": round(med["b"], 4), "ms_forward": round(med["c"], 4),
        "ms_epochs_min_max": min_max(ms["a"]),
        "ms_gather_forward_min_max": min_max(ms["b"]),
        "ms_forward_min_max": min_max(ms["c"]),
        "epochs_over_gather_forward": round(med["a"] / med["b"], 4), "epochs_over_forward": round(med["a"] / med["c"], 4),
        "epochs_per_s": round(E / med["a"] * 1e3),
        "source_bytes": x.numel() * esz, "materialised_bytes": E * C * T * esz,
        "mismatched_epochs": mismatches, "device": torch.cuda.get_device_name(0),
    }


if __name__ == "__main__":
    main(__doc__, CASES, run_case, "epochs", "epochs", lambda res: res["mismatched_epochs"])
