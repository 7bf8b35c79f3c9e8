#!/usr/bin/env python3
"""The bank and stream entries of this build against another build of the library (the parent commit's,
tools/build_base.sh), on one box, in one process: the time gate of a change to bank::set_loop or to the
ring layer-1 body (diagnostic).

Three libraries take turns on the same inputs: the other build, this build, and the other build loaded a
second time from a copy of its file, so that every case carries its own A/A measurement.  Their order
rotates from repeat to repeat; every call lies between two HIP events.  Per case and library the median,
min-max and interquartile range; the case's margin is the disagreement of the two copies of the other
build, the larger of the difference of their medians and the wider of their interquartile ranges; the
case passes when this build's median is at most the other build's plus the margin.  Verified first in
every case: the three libraries' outputs agree byte for byte.

The cases, at the sizes of tools/bench_bank.py, bench_windows_bank.py and bench_streams.py:
  ep_bank_63x288, ep_bank_63x288_shuffled, ep_bank_105x84, each plain and _feat   (bank::k_forward_ep_bank[_feat])
  windows_bank_mmmi_64, windows_bank_bci_12     (bank::k_forward_y1_bank)
  push_bci_1024, push_bci_1024_shuffled         (stream::k_layer1_ring, k_forward_ring)
  push_raw                                      (stream::k_layer1_ring_decim, k_history_update, k_forward_ring; q 2, K 41)
  each_equal, each_ragged                       (stream::k_layer1_ring_each, k_forward_ring_each)
  at_cues, at_feat                              (stream::k_forward_ring_at, k_forward_ring_at_feat)
One JSON document goes to stdout and to <out.json>; the exit status is 1 if any output differs (a failed
time gate is reported, not an error).  There is no CPU path.

  python tools/bench_set_loop_parent.py <the other build's libmibminet.so> <out.json> [--variant canonical|plain_bn]
                                        [--reps 60] [--cases a,b,...]
"""
import argparse
import ctypes
import json
import os
import shutil
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "mi-bminet_amd"), os.path.join(ROOT, "tools")]
import numpy as np
import torch

from mibminet import decimate, lib
from mibminet.params import ParamSet

HOP = 8
KEYS = ("parent", "new", "parent_again")
NAMES = ["net_bank_create", "net_bank_destroy", "net_model_compute_epochs_bank", "net_model_compute_epochs_bank_feat",
         "net_model_compute_windows_bank", "net_streams_create", "net_streams_create_each", "net_streams_destroy",
         "net_streams_push", "net_streams_push_each", "net_streams_windows_at", "net_streams_windows_at_feat",
         "net_streams_set_decimator", "net_streams_push_raw_f32_tm"]


def rotate(fns, reps, warmup, before=None):
    """{key: [ms]}: the candidates in turn within every repeat, the order rotating; `before(r)` runs
    untimed ahead of repeat r."""
    keys = list(fns)
    ms = {k: [] for k in keys}
    for r in range(warmup + reps):
        if before:
            before(r)
        for k in keys[r % len(keys):] + keys[: r % len(keys)]:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fns[k]()
            e1.record()
            e1.synchronize()
            if r >= warmup:
                ms[k].append(e0.elapsed_time(e1))
    return ms


def iqr(v):
    q = statistics.quantiles(v, n=4)
    return q[2] - q[0]


def verdict(ms):
    med = {k: statistics.median(v) for k, v in ms.items()}
    margin = max(abs(med["parent"] - med["parent_again"]), iqr(ms["parent"]), iqr(ms["parent_again"]))
    out = {f"ms_{k}": round(med[k], 4) for k in KEYS}
    out.update({f"ms_{k}_min_max": [round(min(ms[k]), 4), round(max(ms[k]), 4)] for k in KEYS})
    out.update({f"ms_{k}_iqr": round(iqr(ms[k]), 4) for k in KEYS})
    out.update({"margin_ms": round(margin, 4), "new_over_parent": round(med["new"] / med["parent"], 4),
                "pass": med["new"] <= med["parent"] + margin})
    return out


class Libs:
    def __init__(self, other):
        self.tmp = tempfile.mkdtemp()
        again = shutil.copy(other, os.path.join(self.tmp, "libparent_again.so"))
        self.L = {"parent": lib.bind(ctypes.CDLL(other), NAMES), "new": lib.load(),
                  "parent_again": lib.bind(ctypes.CDLL(again), NAMES)}
        self.st = torch.cuda.current_stream().cuda_stream

    def banks(self, sets, scales=None):
        blobs = [ps.to_blob() for ps in sets]
        bufs = [ctypes.create_string_buffer(b, len(b)) for b in blobs]
        ptrs = (ctypes.c_void_p * len(blobs))(*[ctypes.addressof(b) for b in bufs])
        sizes = (ctypes.c_size_t * len(blobs))(*[len(b) for b in blobs])
        sc = None if scales is None else (ctypes.c_float * len(blobs))(*scales)
        out = {}
        for k, L in self.L.items():
            h = ctypes.c_void_p()
            assert L.net_bank_create(ptrs, sizes, sc, len(blobs), ctypes.byref(h), None) == 0
            out[k] = h.value
        return out

    def groups(self, banks, set_of, hop, max_push, each=False):
        arr = (ctypes.c_int32 * len(set_of))(*[int(v) for v in set_of])
        out = {}
        for k, L in self.L.items():
            h = ctypes.c_void_p()
            fn = L.net_streams_create_each if each else L.net_streams_create
            assert fn(banks[k], arr, len(set_of), hop, max_push, 0, ctypes.byref(h)) == 0
            out[k] = h.value
        return out

    def close(self, banks, *groups):
        torch.cuda.synchronize()
        for g in groups:
            for k, L in self.L.items():
                L.net_streams_destroy(g[k])
        for k, L in self.L.items():
            L.net_bank_destroy(banks[k])


def synthetic(n, C, T, N, variant, seed=2026):
    return [ParamSet.synthetic(seed=seed + s, C=C, T=T, N=N, reorder_bn=variant != "plain_bn") for s in range(n)]


def same(ys):
    return int(torch.equal(ys["parent"], ys["new"]) and torch.equal(ys["parent"], ys["parent_again"]))


def ep_bank(X, S, per, C, T, N, shuffled, variant, reps, seed=2026):
    """(plain, _feat): one epochs call over S sets x per epochs, grouped by set or shuffled."""
    E = S * per
    banks = X.banks(synthetic(S, C, T, N, variant))
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randint(-128, 128, (E, C, T), dtype=torch.int8, device="cuda", generator=g)
    onsets = torch.arange(E, dtype=torch.int64, device="cuda") * (C * T)
    set_of = torch.arange(E, dtype=torch.int32, device="cuda") // per
    if shuffled:
        set_of = set_of[torch.randperm(E, device="cuda", generator=g)].contiguous()
    ys = {k: torch.zeros((E, N), dtype=torch.int8, device="cuda") for k in KEYS}
    fs = {k: torch.zeros((E, 16 * (T // 64)), dtype=torch.int8, device="cuda") for k in KEYS}
    res = []
    for feat in (False, True):
        def call(k, feat=feat):
            L = X.L[k]
            lead = (banks[k], x.data_ptr(), x.numel(), T, None, onsets.data_ptr(), set_of.data_ptr(), E, ys[k].data_ptr())
            rc = (L.net_model_compute_epochs_bank_feat(*lead, fs[k].data_ptr(), None, 0, X.st) if feat
                  else L.net_model_compute_epochs_bank(*lead, None, 0, X.st))
            assert rc == 0, rc
        for k in KEYS:
            ys[k].zero_()
            call(k)
        torch.cuda.synchronize()
        ok = same(ys) and (not feat or same(fs)) and bool(ys["new"].any())
        r = verdict(rotate({k: (lambda k=k: call(k)) for k in KEYS}, reps, 5))
        r.update({"items": E, "outputs_agree": bool(ok)})
        res.append(r)
    X.close(banks)
    return res


def windows_bank(X, R, lo, hi, C, T, N, variant, reps, seed=2026):
    sets = synthetic(R, C, T, N, variant)
    banks = X.banks(sets)
    lengths = [int(v) for v in np.random.default_rng(seed).integers(lo, hi + 1, size=R)]
    with lib.Bank(sets) as b:  # the layout and lists are host arithmetic
        starts, Lx, blk_set, onsets, first = lib.bank_windows_lists(b, lengths, list(range(R)), HOP)
    W = len(onsets)
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randint(-128, 128, (C, Lx), dtype=torch.int8, device="cuda", generator=g)
    ond, bsd = torch.from_numpy(onsets).cuda(), torch.from_numpy(blk_set).cuda()
    wsb = int(X.L["new"].net_windows_workspace(Lx))
    ws = torch.empty((wsb,), dtype=torch.int8, device="cuda")
    ys = {k: torch.zeros((W, N), dtype=torch.int8, device="cuda") for k in KEYS}

    def call(k):
        rc = X.L[k].net_model_compute_windows_bank(banks[k], x.data_ptr(), 1, Lx, bsd.data_ptr(), ond.data_ptr(), W,
                                                   ys[k].data_ptr(), None, ws.data_ptr(), wsb, 0, X.st)
        assert rc == 0, rc
    for k in KEYS:
        call(k)
    torch.cuda.synchronize()
    r = verdict(rotate({k: (lambda k=k: call(k)) for k in KEYS}, reps, 5))
    r.update({"items": W, "outputs_agree": bool(same(ys) and bool(ys["new"].any()))})
    X.close(banks)
    return r


def sessions(X, S, n_sets, C, T, N, variant, shuffled=False, seed=2026, scales=None):
    banks = X.banks(synthetic(n_sets, C, T, N, variant), scales)
    set_of = np.sort(np.arange(S) * n_sets // S)
    if shuffled:
        set_of = np.random.default_rng(seed).permutation(set_of)
    return banks, [int(v) for v in set_of]


def push(X, S, n_sets, C, T, N, n, shuffled, variant, reps, seed=2026):
    """One tick of S sessions, n samples each: layer 1 into the rings, then the n / hop windows per session."""
    banks, set_of = sessions(X, S, n_sets, C, T, N, variant, shuffled)
    grp = X.groups(banks, set_of, HOP, n)
    k_ = n // HOP
    lead = T % HOP
    g = torch.Generator(device="cuda").manual_seed(seed)
    xa = torch.randint(-128, 128, (S, C, n), dtype=torch.int8, device="cuda", generator=g)
    ys = {k: torch.zeros((S, k_, N), dtype=torch.int8, device="cuda") for k in KEYS}
    nbad = torch.zeros((1,), dtype=torch.int32, device="cuda")

    def call(k, m=n):
        rc = X.L[k].net_streams_push(grp[k], xa.data_ptr(), 1, m, ys[k].data_ptr(), nbad.data_ptr(), X.st)
        assert rc == 0, rc
    for m in [lead] * (lead > 0) + [n] * (-(-(T - lead) // n) + 2):  # to the grid, then until every push returns n / hop windows
        for k in KEYS:
            call(k, m)
    torch.cuda.synchronize()
    ok = same(ys) and bool(ys["new"].any()) and int(nbad.item()) == 0

    def before(r):  # new samples every tick, the same for the three
        xa.copy_(torch.randint(-128, 128, (S, C, n), dtype=torch.int8, device="cuda", generator=g))
    r = verdict(rotate({k: (lambda k=k: call(k)) for k in KEYS}, reps, 20, before))
    torch.cuda.synchronize()
    r.update({"items": S * k_, "outputs_agree": bool(ok and same(ys))})
    X.close(banks, grp)
    return r


def push_raw(X, S, n_sets, C, T, N, n, q, K, variant, reps, seed=2026):
    """One tick of S sessions through a decimator: q n raw float32 frames each, [S][q n][C], filtered by K taps
    in layer 1, then the n / hop windows per session (bench_streams.py's f32_tm_decim)."""
    banks, set_of = sessions(X, S, n_sets, C, T, N, variant, scales=[1.0 + 0.25 * s for s in range(n_sets)])
    grp = X.groups(banks, set_of, HOP, n)
    taps = decimate.firwin_taps(q, K)
    for k in KEYS:
        assert X.L[k].net_streams_set_decimator(grp[k], q, taps.ctypes.data, K, X.st) == 0
    k_ = n // HOP
    lead = T % HOP
    g = torch.Generator(device="cuda").manual_seed(seed)
    xa = torch.randn((S, q * n, C), dtype=torch.float32, device="cuda", generator=g)
    ys = {k: torch.zeros((S, k_, N), dtype=torch.int8, device="cuda") for k in KEYS}
    nbad = torch.zeros((1,), dtype=torch.int32, device="cuda")

    def call(k, m=n):  # the first q m frames of xa: a tick of m decimated samples
        rc = X.L[k].net_streams_push_raw_f32_tm(grp[k], xa.data_ptr(), q * m, ys[k].data_ptr(), nbad.data_ptr(), X.st)
        assert rc == 0, rc
    for m in [lead] * (lead > 0) + [n] * (-(-(T - lead) // n) + 2):  # to the grid, then until every push returns n / hop windows
        for k in KEYS:
            call(k, m)
    torch.cuda.synchronize()
    ok = same(ys) and bool(ys["new"].any()) and int(nbad.item()) == 0

    def before(r):  # new frames every tick, the same for the three
        xa.copy_(torch.randn((S, q * n, C), dtype=torch.float32, device="cuda", generator=g))
    r = verdict(rotate({k: (lambda k=k: call(k)) for k in KEYS}, reps, 20, before))
    torch.cuda.synchronize()
    r.update({"items": S * k_, "q": q, "K": K, "outputs_agree": bool(ok and same(ys))})
    X.close(banks, grp)
    return r


def push_each(X, S, n_sets, C, T, N, n_max, ragged, variant, reps, seed=2026):
    """One tick of an each-group: every count n_max, or counts drawn from 0 .. n_max anew every tick."""
    banks, set_of = sessions(X, S, n_sets, C, T, N, variant)
    grp = X.groups(banks, set_of, HOP, n_max, each=True)
    kmax = -(-n_max // HOP)
    rng = np.random.default_rng(seed)
    g = torch.Generator(device="cuda").manual_seed(seed)
    xs = torch.randint(-128, 128, (S, C, n_max), dtype=torch.int8, device="cuda", generator=g)
    cin = torch.full((S,), n_max, dtype=torch.int32, device="cuda")
    couts = {k: torch.zeros((S,), dtype=torch.int32, device="cuda") for k in KEYS}
    ys = {k: torch.zeros((S, kmax, N), dtype=torch.int8, device="cuda") for k in KEYS}
    nbad = torch.zeros((1,), dtype=torch.int32, device="cuda")

    def call(k):
        rc = X.L[k].net_streams_push_each(grp[k], xs.data_ptr(), 1, cin.data_ptr(), n_max, ys[k].data_ptr(),
                                          couts[k].data_ptr(), None, nbad.data_ptr(), X.st)
        assert rc == 0, rc

    def before(r):
        if ragged:
            cin.copy_(torch.from_numpy(rng.integers(0, n_max + 1, size=S).astype(np.int32)))
        xs.copy_(torch.randint(-128, 128, (S, C, n_max), dtype=torch.int8, device="cuda", generator=g))
    for r in range(-(-T // (n_max // 2 if ragged else n_max)) + 30):  # until every session returns windows
        before(r)
        for k in KEYS:
            call(k)
    torch.cuda.synchronize()
    ok = same(ys) and same(couts) and bool(ys["new"].any()) and int(couts["new"].sum().item()) > 0 and int(nbad.item()) == 0
    res = verdict(rotate({k: (lambda k=k: call(k)) for k in KEYS}, reps, 20, before))
    torch.cuda.synchronize()
    res.update({"items_last_tick": int(couts["new"].sum().item()), "outputs_agree": bool(ok and same(ys) and same(couts))})
    X.close(banks, grp)
    return res


def windows_at(X, S, n_sets, C, T, N, n, variant, reps, seed=2026):
    """(plain, _feat): one cue per session out of full rings, at an onset drawn inside the span, sorted by session."""
    banks, set_of = sessions(X, S, n_sets, C, T, N, variant)
    grp = X.groups(banks, set_of, HOP, n)
    cap = 16 * -(-(T + n) // 16)
    fill = -(-cap // n) + 2
    g = torch.Generator(device="cuda").manual_seed(seed)
    yp = torch.empty((S, n // HOP + 1, N), dtype=torch.int8, device="cuda")
    nbad = torch.zeros((1,), dtype=torch.int32, device="cuda")
    for _ in range(fill):
        xs = torch.randint(-128, 128, (S, C, n), dtype=torch.int8, device="cuda", generator=g)
        for k in KEYS:
            assert X.L[k].net_streams_push(grp[k], xs.data_ptr(), 1, n, yp.data_ptr(), nbad.data_ptr(), X.st) == 0
    pos = fill * n
    ses = torch.arange(S, dtype=torch.int32, device="cuda")
    ons = torch.from_numpy(np.random.default_rng(seed).integers(0, cap - T + 1, size=S) + (pos - cap)).cuda()
    ys = {k: torch.zeros((S, N), dtype=torch.int8, device="cuda") for k in KEYS}
    fs = {k: torch.zeros((S, 16 * (T // 64)), dtype=torch.int8, device="cuda") for k in KEYS}
    res = []
    for feat in (False, True):
        def call(k, feat=feat):
            L = X.L[k]
            lead = (grp[k], ses.data_ptr(), ons.data_ptr(), S, ys[k].data_ptr())
            rc = (L.net_streams_windows_at_feat(*lead, fs[k].data_ptr(), nbad.data_ptr(), X.st) if feat
                  else L.net_streams_windows_at(*lead, nbad.data_ptr(), X.st))
            assert rc == 0, rc
        for k in KEYS:
            ys[k].zero_()
            call(k)
        torch.cuda.synchronize()
        ok = same(ys) and (not feat or same(fs)) and bool(ys["new"].any()) and int(nbad.item()) == 0
        r = verdict(rotate({k: (lambda k=k: call(k)) for k in KEYS}, 5 * reps, 50))
        r.update({"items": S, "outputs_agree": bool(ok)})
        res.append(r)
    X.close(banks, grp)
    return res


BCI, MMMI = (22, 1125, 4), (64, 480, 4)
CASES = {  # name(s): the run; a pair of names: (plain, _feat)
    ("ep_bank_63x288", "ep_bank_63x288_feat"): lambda X, v, r: ep_bank(X, 63, 288, *BCI, False, v, r),
    ("ep_bank_63x288_shuffled", "ep_bank_63x288_shuffled_feat"): lambda X, v, r: ep_bank(X, 63, 288, *BCI, True, v, r),
    ("ep_bank_105x84", "ep_bank_105x84_feat"): lambda X, v, r: ep_bank(X, 105, 84, *MMMI, False, v, r),
    ("windows_bank_mmmi_64",): lambda X, v, r: [windows_bank(X, 64, 18500, 21500, 64, 480, 2, v, r)],
    ("windows_bank_bci_12",): lambda X, v, r: [windows_bank(X, 12, 89000, 101000, *BCI, v, r)],
    ("push_bci_1024",): lambda X, v, r: [push(X, 1024, 16, *BCI, 16, False, v, 10 * r)],
    ("push_bci_1024_shuffled",): lambda X, v, r: [push(X, 1024, 16, *BCI, 16, True, v, 10 * r)],
    ("push_raw",): lambda X, v, r: [push_raw(X, 1024, 16, *BCI, 16, 2, 41, v, 10 * r)],
    ("each_equal",): lambda X, v, r: [push_each(X, 1024, 16, *BCI, 16, False, v, 10 * r)],
    ("each_ragged",): lambda X, v, r: [push_each(X, 1024, 16, *BCI, 32, True, v, 10 * r)],
    ("at_cues", "at_feat"): lambda X, v, r: windows_at(X, 1024, 16, *BCI, 16, v, r),
}
FAMILY = {"ep_bank": "bank::k_forward_ep_bank + _feat", "windows_bank": "bank::k_forward_y1_bank",
          "push": "stream::k_layer1_ring + k_forward_ring",
          "push_raw": "stream::k_layer1_ring_decim + k_history_update + k_forward_ring", "each": "stream::k_layer1_ring_each + k_forward_ring_each",
          "at": "stream::k_forward_ring_at + _feat"}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("other")
    ap.add_argument("out")
    ap.add_argument("--variant", default="canonical", choices=("canonical", "plain_bn"))
    ap.add_argument("--reps", type=int, default=60)
    ap.add_argument("--cases", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_set_loop_parent.py needs a GPU (there is no CPU path)")
    X = Libs(a.other)
    only = [c for c in a.cases.split(",") if c]
    out = {"device": torch.cuda.get_device_name(0), "variant": a.variant, "reps": a.reps,
           "margin": "max(|median parent - median parent_again|, IQR parent, IQR parent_again), per case",
           "gate": "median new <= median parent + margin", "cases": {}}
    for names, run in CASES.items():
        if only and not set(names) & set(only):
            continue
        for name, r in zip(names, run(X, a.variant, a.reps)):
            out["cases"][name] = r
            print(name, json.dumps(r), flush=True)
        torch.cuda.empty_cache()
    fams = {}
    for name, r in out["cases"].items():
        fam = FAMILY[next(p for p in sorted(FAMILY, key=len, reverse=True) if name.startswith(p))]
        fams.setdefault(fam, []).append(r["pass"])
    out["families"] = {f: all(v) for f, v in fams.items()}
    line = json.dumps(out)
    print(line)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    shutil.rmtree(X.tmp, ignore_errors=True)
    sys.exit(0 if all(r["outputs_agree"] for r in out["cases"].values()) else 1)


if __name__ == "__main__":
    main()
