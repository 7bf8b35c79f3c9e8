#!/usr/bin/env python3
"""The sliding windows of many recordings, each under its own network, in one call against what a
caller had before.

For each case (one MI355X, one process, HIP events around each candidate, host work included):
  (a) one net_model_compute_windows_bank call over all recordings, laid at multiples of 16 samples;
  (b) per recording, net_params_load of its network's blob and net_model_compute_windows on the
      recording's own array (every set loaded once before timing, the blobs serialised beforehand,
      the C entries called directly);
  (c) one net_model_compute_epochs_bank call on the same array and onsets with set_of per window:
      one launch, but layer 1 runs once per window;
  (d) one set loaded and one net_model_compute_windows_at call over the same array and onsets: the
      floor with no switching (its logits are one network's, so only the rows of that network's
      recordings are compared).
The recordings are int8 [C][L_r], lengths uniform in the case's range, hop 8, recording r under set
r.  a, b, c and d alternate within every repeat and report medians; gates: a < b and a < c.  bci_12
then runs five rounds in the order D A D A D, each the median of --reps calls of one candidate; gate:
every A round at most 1.05 x the mean of its two neighbouring D medians plus their difference (the
rule of tools/bench_bank.py).  Every logit row of (b) and (c) must equal (a)'s.  One JSON line per
case goes to <out-dir>/windows_bank_<name>.json and to stdout.  There is no CPU path.

  python tools/bench_windows_bank.py [--cases mmmi_64,bci_12] [--limit R] [--reps 7] [--warmup 2]
                                     [--variant canonical|plain_bn] [--out-dir profiles]
"""
import ctypes
import statistics

from bench_common import main, medians, min_max, time_alternating

HOP = 8
CASES = {  # name: (recordings = sets, shortest and longest recording, C, T, N, rounds D A D A D)
    "mmmi_64": (64, 18500, 21500, 64, 480, 2, False),
    "bci_12": (12, 89000, 101000, 22, 1125, 4, True),
}


def run_case(name, limit, reps, warmup, variant, seed=2026):
    import numpy as np
    import torch

    from mibminet import lib
    from mibminet.params import ParamSet

    R, lo, hi, C, T, N, rounds = CASES[name]
    R = min(R, limit)  # --limit: fewer recordings, for a quick look
    sets = [ParamSet.synthetic(seed=seed + s, C=C, T=T, N=N, reorder_bn=variant != "plain_bn") for s in range(R)]
    blobs = [ps.to_blob() for ps in sets]
    bufs = [ctypes.create_string_buffer(b, len(b)) for b in blobs]
    lengths = [int(v) for v in np.random.default_rng(seed).integers(lo, hi + 1, size=R)]
    bank = lib.Bank(blobs)
    starts, Lx, blk_set, onsets, first = lib.bank_windows_lists(bank, lengths, list(range(R)), HOP)
    W = len(onsets)
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randint(-128, 128, (C, Lx), dtype=torch.int8, device="cuda", generator=g)
    recs = [x[:, int(starts[r]): int(starts[r]) + lengths[r]].contiguous() for r in range(R)]
    ond = torch.from_numpy(onsets).cuda()
    bsd = torch.from_numpy(blk_set).cuda()
    set_of = torch.from_numpy(np.repeat(np.arange(R, dtype=np.int32), np.diff(first))).cuda()
    A = lib.load()
    st = torch.cuda.current_stream().cuda_stream
    ya, yc, yd = (torch.empty((W, N), dtype=torch.int8, device="cuda") for _ in range(3))
    yb = [torch.empty((int(first[r + 1] - first[r]), N), dtype=torch.int8, device="cuda") for r in range(R)]
    wsb = lib.windows_workspace(Lx)
    ws = torch.empty((wsb,), dtype=torch.int8, device="cuda")

    def a():
        rc = A.net_model_compute_windows_bank(bank.handle, x.data_ptr(), 1, Lx, bsd.data_ptr(), ond.data_ptr(), W,
                                              ya.data_ptr(), None, ws.data_ptr(), wsb, 0, st)
        assert rc == 0, rc

    def b():
        for r in range(R):
            rc = A.net_params_load(bufs[r], len(blobs[r]))
            rc = rc or A.net_model_compute_windows(recs[r].data_ptr(), 1, lengths[r], HOP, yb[r].data_ptr(), ws.data_ptr(),
                                                   wsb, 0, st)
            assert rc == 0, rc

    def c():
        rc = A.net_model_compute_epochs_bank(bank.handle, x.data_ptr(), x.numel(), Lx, None, ond.data_ptr(),
                                             set_of.data_ptr(), W, yc.data_ptr(), None, 0, st)
        assert rc == 0, rc

    def d():  # on whichever set (b) loaded last: they all have the case's geometry
        rc = A.net_model_compute_windows_at(x.data_ptr(), 1, Lx, ond.data_ptr(), W, yd.data_ptr(), None, ws.data_ptr(), wsb,
                                            0, st)
        assert rc == 0, rc

    a()
    b()  # loads every set once
    c()
    d()
    torch.cuda.synchronize()
    mis_b = int((ya != torch.cat(yb, dim=0)).any(dim=1).sum().item())
    mis_c = int((ya != yc).any(dim=1).sum().item())
    tail = slice(int(first[R - 1]), W)  # the rows of the set (d) runs on
    mis_d = int((ya[tail] != yd[tail]).any(dim=1).sum().item())
    info = bank.info()
    res = {"name": name, "recordings": R, "sets": R, "samples": Lx, "windows": W, "hop": HOP, "C": C, "T": T, "N": N,
           "variant": variant, "exact_division": bool(info[4]), "bank_bytes": info[0] * info[6], "reps": reps,
           "warmup": warmup, "mismatched_rows": {"b": mis_b, "c": mis_c, "d_own_recording": mis_d},
           "device": torch.cuda.get_device_name(0)}
    ms = time_alternating({"a": a, "b": b, "c": c, "d": d}, reps, warmup)
    med = medians(ms)
    res.update({"ms_windows_bank": round(med["a"], 4), "ms_load_and_windows_per_recording": round(med["b"], 4),
                "ms_epochs_bank": round(med["c"], 4), "ms_one_set_windows_at": round(med["d"], 4),
                "ms_windows_bank_min_max": min_max(ms["a"]), "ms_load_and_windows_per_recording_min_max": min_max(ms["b"]),
                "ms_epochs_bank_min_max": min_max(ms["c"]), "ms_one_set_windows_at_min_max": min_max(ms["d"]),
                "a_over_b": round(med["a"] / med["b"], 4), "a_over_c": round(med["a"] / med["c"], 4),
                "a_over_d": round(med["a"] / med["d"], 4), "windows_per_s": round(W / med["a"] * 1e3),
                "gates": {"a < b": med["a"] < med["b"], "a < c": med["a"] < med["c"]}})
    ok = med["a"] < med["b"] and med["a"] < med["c"]
    if rounds:
        rmed = []
        for k in "DADAD":
            v = time_alternating({k: d if k == "D" else a}, reps, warmup)[k]
            rmed.append(round(statistics.median(v), 4))
        verdicts = []
        for i in (1, 3):
            lo_, hi_ = sorted((rmed[i - 1], rmed[i + 1]))
            limit_ms = 1.05 * (lo_ + hi_) / 2 + (hi_ - lo_)
            verdicts.append({"round": f"A{(i + 1) // 2}", "bank_ms": rmed[i], "one_set_ms": [rmed[i - 1], rmed[i + 1]],
                             "limit_ms": round(limit_ms, 4), "over_one_set_mean": round(rmed[i] / ((lo_ + hi_) / 2) - 1, 4),
                             "pass": rmed[i] <= limit_ms})
        res.update({"order": "D A D A D", "round_medians_ms": rmed, "verdicts": verdicts,
                    "floor_gate": "each A <= 1.05 x mean of its neighbouring D + their difference",
                    "floor_pass": all(v["pass"] for v in verdicts)})
        ok = ok and res["floor_pass"]
    res["pass"] = ok
    bank.close()
    lib.params_unload()
    return res


if __name__ == "__main__":
    main(__doc__, CASES, run_case, "limit", "windows_bank",
         lambda res: res["mismatched_rows"]["b"] + res["mismatched_rows"]["c"] + res["mismatched_rows"]["d_own_recording"])
