"""Every kernel family on parameter sets whose logits see every parameter element.

A weight, factor or offset reaches a kernel through the fragment and table builders of
csrc/images.hpp.  The entries of param_faults.PCASES are certified on the CPU
(tests/test_param_observability_cpu.py): a weight or bias off by one, a zeroed weight, two
neighbouring elements of an array exchanged along any axis, two neighbouring filters' factor or
offset exchanged, or a scalar factor off by one changes some logit of some trial of the batch
("Observability of the parameters").  Here each batch runs through every entry that
computes the forward pass, against the C oracle, byte for byte; and a sample of single faults is
loaded one after the other, each of which must give the faulted set's logits, not the base set's.
"""
import numpy as np
import pytest

import oracle
import param_faults as pf
from mibminet import lib
from mibminet.params import pack_trials
from support import NTH, at_offset, run_entries

pytestmark = pytest.mark.gpu
NAMES = [c.name for c in pf.PCASES]
_COMPILED = {(C, T) for C, T, _ in pf.COMPILED}
_COMPILED_NAMES = [c.name for c in pf.PCASES if c.dims[:2] in _COMPILED]
PER_GROUP = 2  # faults per (array, family): 25 groups, about 48 faults
TRIES = 24  # candidates per group looked at for ones the first 64 trials see


def _path(case):
    return ("exact" if case.exact else "float") if case.dims[:2] in _COMPILED and case.dims[2] == 4 else "general"


@pytest.mark.parametrize("name", NAMES)
def test_certified_case(name, gpu):
    """Every forward entry of support.run_entries on the certified batch.  The
    compiled geometries run their compiled kernels here."""
    case = pf.PCASES[NAMES.index(name)]
    try:
        run_entries(case, _path(case))
    finally:
        case.drop()


@pytest.mark.parametrize("name", _COMPILED_NAMES)
def test_certified_case_forced_general(name, gpu):
    """The compiled geometries' certified batches on the general kernels."""
    case = pf.PCASES[NAMES.index(name)]
    try:
        lib.force_general(True)
        run_entries(case, "general")
    finally:
        lib.force_general(False)
        case.drop()


def _sample(case, xp, base):
    """About 48 faults from a fixed seed, PER_GROUP of every (array, family), each with the faulted
    set and its oracle logits on the trials xp; only faults that those trials see (the oracle's
    logits differ from the base set's) and that the case does not exclude."""
    ps = case.ps
    groups = {}
    for ft in pf.faults(ps):
        groups.setdefault(ft[:2], []).append(ft)
    rng = np.random.default_rng([case.seed, *case.dims, 48])
    out = []
    for key, fts in groups.items():
        got = 0
        for i in rng.permutation(len(fts))[:TRIES]:
            ft = fts[int(i)]
            q = None if case.excluded(ft) else pf.apply(ps, ft)
            if q is None:
                continue
            want = oracle.COracle(q).batch(xp, nthreads=NTH)
            if (want != base).any():
                out.append((ft, q, want))
                got += 1
                if got == PER_GROUP:
                    break
    return out


def _differential(case, path):
    import torch

    name, ps, x = case
    x = x[:64]
    xp = pack_trials(x)
    base = oracle.COracle(ps).batch(xp, nthreads=NTH)
    faults = _sample(case, xp, base)
    fam = {f: sum(1 for ft, _, _ in faults if ft[1] == f) for f in pf.FAMILIES}
    assert len(faults) >= 40 and all(n >= 4 for n in fam.values()), (len(faults), fam)
    xd, xc = torch.from_numpy(xp).cuda(), at_offset(torch, x, 1)

    def check(want, what):
        for entry, got in (("time-major", lib.forward_torch(xd)), ("channel-major", lib.forward_ct_torch(xc))):
            bad = np.flatnonzero((got.cpu().numpy() != want).any(1))
            assert bad.size == 0, f"{name} {what} {entry}: {bad.size} of 64 trials differ, first {bad[:5]}"

    lib.params_load(ps)
    assert lib.params_info()["path"] == path
    check(base, "base set")
    for ft, q, want in faults:
        lib.params_load(q)
        assert lib.params_info()["path"] == path, ft[:3]
        check(want, f"fault {ft[:3]} (changes {ft[3]})")
    lib.params_load(ps)
    check(base, "base set loaded again")


@pytest.mark.parametrize("name", NAMES)
def test_single_faults_reach_the_device(name, gpu):
    """About 48 single faults of the certified set, at least four of every family, each visible on
    the first 64 trials: the set with that one change loaded gives the oracle's logits for it in
    the time-major and the channel-major entry (the element reaches the device, and a set that
    differs from a cached one in a single element gets its own image); the base set loaded last
    gives the base logits again."""
    case = pf.PCASES[NAMES.index(name)]
    try:
        _differential(case, _path(case))
    finally:
        case.drop()


@pytest.mark.parametrize("name", [f"{C}x{T}" for C, T, _ in pf.COMPILED])
def test_single_faults_reach_the_device_forced_general(name, gpu):
    """The same on the general kernels' images of the compiled geometries."""
    case = pf.PCASES[NAMES.index(name)]
    try:
        lib.force_general(True)
        _differential(case, "general")
    finally:
        lib.force_general(False)
        case.drop()
