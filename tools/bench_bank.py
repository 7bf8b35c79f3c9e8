#!/usr/bin/env python3
"""Many networks in one bank call against one parameter load and one epochs call per network.

For each case (one MI355X, one process, HIP events around each candidate, host work included):
  (a) one net_model_compute_epochs_bank call over all sets' epochs;
  (b) what a caller does without banks: per set, net_params_load of its blob and
      net_model_compute_epochs on its slice of the epochs (every set loaded once before timing, the
      blobs serialised beforehand, the C entries called directly);
  (c) one set loaded and one net_model_compute_epochs call over all epochs: the floor with no
      switching (its logits are another network's, so only (a) and (b) are compared).
The epochs are a contiguous int8 batch [E][C][T] (onset e C T, row stride T), grouped by set unless
the case shuffles set_of.  bci_63x288, mmmi_105x84 and bci_shuffled alternate a, b, c within every
repeat and report medians; gate: a <= b.  big_4x16384 runs five rounds in the order C A C A C, each
the median of --reps calls of one candidate; gate: every A round at most 1.05 x the mean of its two
neighbouring C medians plus their difference (the rule of profiles/binding_speed.json).  One JSON
line per case goes to <out-dir>/bank_<name>.json and to stdout.  There is no CPU path.

bci_63x288_feat (report only, no gate): on bci_63x288's epochs, (a) the plain bank call, (a2) the same
call again, so that the run-to-run spread of one candidate stands beside the numbers, and (f)
net_model_compute_epochs_bank_feat, which also stores 16 T64 bytes of layer-4 activations per epoch;
the three alternate within every repeat.  Verified first: (f)'s logits equal (a)'s.  Then
net_bank_replace of one slot, --reps times, the queue drained before each: the host's time per call
(a clock around it) and the device's time of the slot update (HIP events around it).

  python tools/bench_bank.py [--cases bci_63x288,mmmi_105x84,big_4x16384,bci_shuffled,bci_63x288_feat] [--limit N]
                             [--reps 7] [--warmup 2] [--variant canonical|plain_bn] [--out-dir profiles]
"""
import ctypes
import statistics
import time

from bench_common import main, medians, min_max, time_alternating

CASES = {  # name: (sets, epochs per set, C, T, N, shuffled, rounds C A C A C)
    "bci_63x288": (63, 288, 22, 1125, 4, False, False),
    "mmmi_105x84": (105, 84, 64, 480, 4, False, False),
    "big_4x16384": (4, 16384, 22, 1125, 4, False, True),
    "bci_shuffled": (63, 288, 22, 1125, 4, True, False),
}
FEAT_CASES = {"bci_63x288_feat": (63, 288, 22, 1125, 4)}  # name: (sets, epochs per set, C, T, N)


def run_feat(name, limit, reps, warmup, variant, seed=2026):
    import torch

    from mibminet import lib
    from mibminet.params import ParamSet

    S, per, C, T, N = FEAT_CASES[name]
    per = min(per, limit)
    E = S * per
    sets = [ParamSet.synthetic(seed=seed + s, C=C, T=T, N=N, reorder_bn=variant != "plain_bn") for s in range(S)]
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randint(-128, 128, (E, C, T), dtype=torch.int8, device="cuda", generator=g)
    onsets = torch.arange(E, dtype=torch.int64, device="cuda") * (C * T)
    set_of = torch.arange(E, dtype=torch.int32, device="cuda") // per
    L = lib.load()
    st = torch.cuda.current_stream().cuda_stream
    ya, yf = (torch.empty((E, N), dtype=torch.int8, device="cuda") for _ in range(2))
    bank = lib.Bank(sets)
    fb = bank.feature_bytes()
    feat = torch.empty((E, fb), dtype=torch.int8, device="cuda")

    def a():
        rc = L.net_model_compute_epochs_bank(bank.handle, x.data_ptr(), x.numel(), T, None, onsets.data_ptr(),
                                             set_of.data_ptr(), E, ya.data_ptr(), None, 0, st)
        assert rc == 0, rc

    def f():
        rc = L.net_model_compute_epochs_bank_feat(bank.handle, x.data_ptr(), x.numel(), T, None, onsets.data_ptr(),
                                                  set_of.data_ptr(), E, yf.data_ptr(), feat.data_ptr(), None, 0, st)
        assert rc == 0, rc

    a()
    f()
    torch.cuda.synchronize()
    mismatches = int((ya != yf).any(dim=1).sum().item())
    ms = time_alternating({"a": a, "f": f, "a2": a}, reps, warmup)
    med = medians(ms)
    # net_bank_replace of slot S // 2 by another set of the geometry
    blob = ParamSet.synthetic(seed=seed + S, C=C, T=T, N=N, reorder_bn=variant != "plain_bn").to_blob()
    buf = ctypes.create_string_buffer(blob, len(blob))
    host_ms, dev_ms = [], []
    for r in range(warmup + reps):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        t0 = time.perf_counter()
        rc = L.net_bank_replace(bank.handle, S // 2, buf, len(blob), 0.0, 0, st)
        t1 = time.perf_counter()
        e1.record()
        e1.synchronize()
        assert rc == 0, rc
        if r >= warmup:
            host_ms.append((t1 - t0) * 1e3)
            dev_ms.append(e0.elapsed_time(e1))
    info = bank.info()
    res = {"name": name, "sets": S, "epochs_per_set": per, "epochs": E, "C": C, "T": T, "N": N, "variant": variant,
           "feature_bytes_per_epoch": fb, "input_bytes_per_epoch": C * T, "reps": reps, "warmup": warmup,
           "mismatched_epochs": mismatches, "device": torch.cuda.get_device_name(0),
           "ms_plain": round(med["a"], 4), "ms_plain_again": round(med["a2"], 4), "ms_feat": round(med["f"], 4),
           "ms_plain_min_max": min_max(ms["a"]), "ms_plain_again_min_max": min_max(ms["a2"]), "ms_feat_min_max": min_max(ms["f"]),
           "feat_over_plain": round(med["f"] / med["a"], 4), "plain_again_over_plain": round(med["a2"] / med["a"], 4),
           "replace_bytes": info[6], "replace_host_ms": round(statistics.median(host_ms), 4),
           "replace_host_ms_min_max": min_max(host_ms), "replace_events_ms": round(statistics.median(dev_ms), 4),
           "replace_events_ms_min_max": min_max(dev_ms), "gate": "none: report only", "pass": mismatches == 0}
    bank.close()
    return res


def run_case(name, limit, reps, warmup, variant, seed=2026):
    if name in FEAT_CASES:
        return run_feat(name, limit, reps, warmup, variant, seed)
    import torch

    from mibminet import lib
    from mibminet.params import ParamSet

    S, per, C, T, N, shuffled, rounds = CASES[name]
    per = min(per, limit)  # --limit: fewer epochs per set, for a quick look
    E = S * per
    sets = [ParamSet.synthetic(seed=seed + s, C=C, T=T, N=N, reorder_bn=variant != "plain_bn") for s in range(S)]
    blobs = [ps.to_blob() for ps in sets]
    bufs = [ctypes.create_string_buffer(b, len(b)) for b in blobs]
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randint(-128, 128, (E, C, T), dtype=torch.int8, device="cuda", generator=g)
    onsets = torch.arange(E, dtype=torch.int64, device="cuda") * (C * T)
    set_of = torch.arange(E, dtype=torch.int32, device="cuda") // per
    if shuffled:
        set_of = set_of[torch.randperm(E, device="cuda", generator=g)].contiguous()
    L = lib.load()
    st = torch.cuda.current_stream().cuda_stream
    ya, yb, yc = (torch.empty((E, N), dtype=torch.int8, device="cuda") for _ in range(3))
    bank = lib.Bank(blobs)

    def a():
        rc = L.net_model_compute_epochs_bank(bank.handle, x.data_ptr(), x.numel(), T, None, onsets.data_ptr(),
                                             set_of.data_ptr(), E, ya.data_ptr(), None, 0, st)
        assert rc == 0, rc

    if shuffled:  # (b) per set on that set's epochs, gathered beforehand (outside the timing)
        order = torch.argsort(set_of.to(torch.int64), stable=True)
        on_b = onsets[order].contiguous()
    else:
        order, on_b = None, onsets

    def b():
        for s in range(S):
            rc = L.net_params_load(bufs[s], len(blobs[s]))
            lo = s * per
            rc = rc or L.net_model_compute_epochs(x.data_ptr(), x.numel(), T, None, on_b.data_ptr() + 8 * lo, per,
                                                  yb.data_ptr() + N * lo, None, 0, st)
            assert rc == 0, rc

    def c():  # on whichever set (b) loaded last: they all have the case's geometry
        rc = L.net_model_compute_epochs(x.data_ptr(), x.numel(), T, None, onsets.data_ptr(), E, yc.data_ptr(), None, 0, st)
        assert rc == 0, rc

    a()
    b()  # loads every set once
    torch.cuda.synchronize()
    got_b = yb if order is None else torch.empty_like(yb).index_copy_(0, order, yb)
    mismatches = int((ya != got_b).any(dim=1).sum().item())
    info = bank.info()
    res = {"name": name, "sets": S, "epochs_per_set": per, "epochs": E, "C": C, "T": T, "N": N, "shuffled": shuffled,
           "variant": variant, "exact_division": bool(info[4]), "bank_bytes": info[0] * info[6], "reps": reps,
           "warmup": warmup, "mismatched_epochs": mismatches, "device": torch.cuda.get_device_name(0)}
    if rounds:
        med = []
        for k in "CACAC":
            ms = time_alternating({k: c if k == "C" else a}, reps, warmup)[k]
            med.append(round(statistics.median(ms), 4))
        verdicts = []
        for i in (1, 3):
            lo, hi = sorted((med[i - 1], med[i + 1]))
            limit_ms = 1.05 * (lo + hi) / 2 + (hi - lo)
            verdicts.append({"round": f"A{(i + 1) // 2}", "bank_ms": med[i], "one_set_ms": [med[i - 1], med[i + 1]],
                             "limit_ms": round(limit_ms, 4), "over_one_set_mean": round(med[i] / ((lo + hi) / 2) - 1, 4),
                             "pass": med[i] <= limit_ms})
        res.update({"order": "C A C A C", "medians_ms": med, "verdicts": verdicts,
                    "gate": "each A <= 1.05 x mean of its neighbouring C + their difference",
                    "pass": all(v["pass"] for v in verdicts), "epochs_per_s": round(E / med[1] * 1e3)})
    else:
        ms = time_alternating({"a": a, "b": b, "c": c}, reps, warmup)
        med = medians(ms)
        res.update({"ms_bank": round(med["a"], 4), "ms_load_and_epochs_per_set": round(med["b"], 4),
                    "ms_one_set": round(med["c"], 4), "ms_bank_min_max": min_max(ms["a"]),
                    "ms_load_and_epochs_per_set_min_max": min_max(ms["b"]),
                    "ms_one_set_min_max": min_max(ms["c"]),
                    "bank_over_per_set": round(med["a"] / med["b"], 4), "bank_over_one_set": round(med["a"] / med["c"], 4),
                    "epochs_per_s": round(E / med["a"] * 1e3)})
        if not shuffled:
            res.update({"gate": "bank <= load + epochs per set", "pass": med["a"] <= med["b"]})
    bank.close()
    lib.params_unload()
    return res


if __name__ == "__main__":
    main(__doc__, {**CASES, **FEAT_CASES}, run_case, "limit", "bank", lambda res: res["mismatched_epochs"])
