#!/usr/bin/env python3
"""The plain entries of another build of the library (the parent commit's) beside this build's plain
and _feat entries, on one box, in one process (diagnostic, report only): bci_63x288's epochs through a
bank, and 1,024 cue-locked windows out of the rings of 1,024 sessions of 22 x 1125 under 16 sets.  The
four candidates (the other build's plain entry, this build's, this build's _feat entry, the other
build's again) alternate within every repeat, each between two HIP events; medians and min-max go as
one JSON line to stdout and to <out.json>.  Verified first: all logits agree.  There is no CPU path.

  python tools/bench_feat_parent.py <the other build's libmibminet.so> <out.json> [reps]
"""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "mi-bminet_amd"), os.path.join(ROOT, "tools")]
import numpy as np
import torch

from bench_common import medians, min_max, time_alternating
from mibminet import lib
from mibminet.params import ParamSet

reps = int(sys.argv[3]) if len(sys.argv) > 3 else 200
NAMES = ["net_bank_create", "net_bank_destroy", "net_model_compute_epochs_bank", "net_streams_create", "net_streams_destroy",
         "net_streams_push", "net_streams_windows_at"]
new = lib.load()
old = lib.bind(ctypes.CDLL(sys.argv[1]), NAMES)
st = torch.cuda.current_stream().cuda_stream


def make_bank(L, blobs):
    bufs = [ctypes.create_string_buffer(b, len(b)) for b in blobs]
    ptrs = (ctypes.c_void_p * len(blobs))(*[ctypes.addressof(b) for b in bufs])
    sizes = (ctypes.c_size_t * len(blobs))(*[len(b) for b in blobs])
    h = ctypes.c_void_p()
    assert L.net_bank_create(ptrs, sizes, None, len(blobs), ctypes.byref(h), None) == 0
    return h.value


out = {"device": torch.cuda.get_device_name(0), "reps": reps}
# ---- epochs through a bank: 63 sets x 288 epochs of 22 x 1125
S, per, C, T, N = 63, 288, 22, 1125, 4
E = S * per
blobs = [ParamSet.synthetic(seed=2026 + s, C=C, T=T, N=N).to_blob() for s in range(S)]
g = torch.Generator(device="cuda").manual_seed(2026)
x = torch.randint(-128, 128, (E, C, T), dtype=torch.int8, device="cuda", generator=g)
onsets = torch.arange(E, dtype=torch.int64, device="cuda") * (C * T)
set_of = torch.arange(E, dtype=torch.int32, device="cuda") // per
ys = {k: torch.empty((E, N), dtype=torch.int8, device="cuda") for k in ("old", "new", "feat")}
feat = torch.empty((E, 16 * (T // 64)), dtype=torch.int8, device="cuda")
banks = {"old": make_bank(old, blobs), "new": make_bank(new, blobs)}


def plain(L, key):
    def f():
        assert L.net_model_compute_epochs_bank(banks[key], x.data_ptr(), x.numel(), T, None, onsets.data_ptr(), set_of.data_ptr(),
                                               E, ys[key].data_ptr(), None, 0, st) == 0
    return f


def with_feat():
    assert new.net_model_compute_epochs_bank_feat(banks["new"], x.data_ptr(), x.numel(), T, None, onsets.data_ptr(),
                                                  set_of.data_ptr(), E, ys["feat"].data_ptr(), feat.data_ptr(), None, 0, st) == 0


fns = {"parent_plain": plain(old, "old"), "plain": plain(new, "new"), "feat": with_feat, "parent_plain_again": plain(old, "old")}
for f in fns.values():
    f()
torch.cuda.synchronize()
assert torch.equal(ys["old"], ys["new"]) and torch.equal(ys["old"], ys["feat"])
ms = time_alternating(fns, reps, 20)
med = medians(ms)
out["epochs_bank_63x288"] = {**{f"ms_{k}": round(v, 4) for k, v in med.items()}, **{f"ms_{k}_min_max": min_max(v) for k, v in ms.items()}}
old.net_bank_destroy(banks["old"])
new.net_bank_destroy(banks["new"])
del x

# ---- cue-locked windows out of the rings: 1,024 sessions of 22 x 1125 under 16 sets, one cue each
S, n_sets, HOP, n = 1024, 16, 8, 16
blobs = blobs[:n_sets]
sets = np.sort(np.arange(S) * n_sets // S).astype(np.int32)
arr = (ctypes.c_int32 * S)(*[int(v) for v in sets])
grp, bk = {}, {}
for key, L in (("old", old), ("new", new)):
    bk[key] = make_bank(L, blobs)
    h = ctypes.c_void_p()
    assert L.net_streams_create(bk[key], arr, S, HOP, n, 0, ctypes.byref(h)) == 0
    grp[key] = h.value
cap = 16 * -(-(T + n) // 16)
fill = -(-cap // n) + 2
xs = torch.randint(-128, 128, (S, C, n), dtype=torch.int8, device="cuda", generator=g)
yp = torch.empty((S, n // HOP + 1, N), dtype=torch.int8, device="cuda")
nbad = torch.zeros((1,), dtype=torch.int32, device="cuda")
for _ in range(fill):
    for key, L in (("old", old), ("new", new)):
        assert L.net_streams_push(grp[key], xs.data_ptr(), 1, n, yp.data_ptr(), nbad.data_ptr(), st) == 0
pos = fill * n
ses = torch.arange(S, dtype=torch.int32, device="cuda")
ons = torch.from_numpy(np.random.default_rng(1).integers(0, cap - T + 1, size=S) + (pos - cap)).cuda()
yw = {k: torch.empty((S, N), dtype=torch.int8, device="cuda") for k in ("old", "new", "feat")}
fw = torch.empty((S, 16 * (T // 64)), dtype=torch.int8, device="cuda")


def at(L, key):
    def f():
        assert L.net_streams_windows_at(grp[key], ses.data_ptr(), ons.data_ptr(), S, yw[key].data_ptr(), nbad.data_ptr(), st) == 0
    return f


def at_feat():
    assert new.net_streams_windows_at_feat(grp["new"], ses.data_ptr(), ons.data_ptr(), S, yw["feat"].data_ptr(), fw.data_ptr(),
                                           nbad.data_ptr(), st) == 0


fns = {"parent_plain": at(old, "old"), "plain": at(new, "new"), "feat": at_feat, "parent_plain_again": at(old, "old")}
for f in fns.values():
    f()
torch.cuda.synchronize()
assert int(nbad.item()) == 0 and torch.equal(yw["old"], yw["new"]) and torch.equal(yw["old"], yw["feat"]) and bool(yw["old"].any())
ms = time_alternating(fns, 5 * reps, 50)
med = medians(ms)
out["windows_at_1024"] = {**{f"ms_{k}": round(v, 4) for k, v in med.items()}, **{f"ms_{k}_min_max": min_max(v) for k, v in ms.items()}}
for key, L in (("old", old), ("new", new)):
    L.net_streams_destroy(grp[key])
    L.net_bank_destroy(bk[key])
line = json.dumps(out)
print(line)
with open(sys.argv[2], "w") as f:
    f.write(line + "\n")
