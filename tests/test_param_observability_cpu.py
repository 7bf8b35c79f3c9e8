"""Certifies the inputs of tests/test_gpu_param_observability.py on the CPU: for every entry of
param_faults.PCASES each single fault of the parameter set (one weight or bias +-1, one weight
zeroed, two neighbouring elements of an array exchanged along one axis, two neighbouring filters'
factor or offset exchanged, a scalar factor +-1) changes some logit of some trial of the golden
model, and no fault leaves the set as it was.  Only then does ``logits == oracle`` on the GPU say
that every parameter element reached the place the kernels read it from.  This is a condition on
the inputs, met by the reference alone; no kernel runs here.

One module fixture runs the audits, split into shards, in a spawn process pool (at most 16
workers).  With OBSERVABILITY_RECORD=1 the measured figures are written to
profiles/param_observability.txt.
"""
import concurrent.futures
import multiprocessing
import os
import time

import numpy as np
import pytest

import oracle
import param_faults as pf
from mibminet.params import ParamSet, pack_trials
from oracle import golden_np as G
from support import NTH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = [c.name for c in pf.PCASES]
SHARDS = 4


def _rng_x(ps, B, seed):
    return np.random.default_rng(seed).integers(-127, 128, size=(B, ps.dims.C, ps.dims.T)).astype(np.int8)


@pytest.mark.parametrize("make", ["ident", "ident-plain-int4", "synthetic-balanced"])
def test_audit_matches_brute_force(make):
    """The row-wise recomputation against "build the faulted set, run golden_np.forward on every
    trial": the same verdict on every fault of every family (an identifiable and a calibrated set,
    both BN branches, both clips, both weight widths) on every sixth fault; and the shards of an
    audit are a partition of the faults."""
    if make == "ident":
        ps = pf.ident_set(3, C=3, T=77, N=3)
    elif make == "ident-plain-int4":
        ps = pf.ident_set(5, C=2, T=130, N=2, reorder_bn=False, weight_bits=4)
    else:
        ps = ParamSet.synthetic(3, C=3, T=77, N=3, clip_balanced=True)
    x = _rng_x(ps, 6, 1)
    same = lambda a, b: all({k: v if k != "unseen_list" else sorted(v) for k, v in a[key].items()} ==
                            {k: v if k != "unseen_list" else sorted(v) for k, v in b[key].items()} for key in b)
    parts = [pf.audit_params(ps, x, chunk=4, shard=(k, 6)) for k in range(6)]
    slow = pf.audit_params(ps, x, brute=True, shard=(1, 6))  # every sixth fault the plain way
    assert set(k[1] for k in slow) == set(pf.FAMILIES)
    assert same(parts[1], slow)
    tot, whole = pf.totals(slow), pf.totals(pf.merge(parts))
    assert tot["seen"] and tot["unseen"]  # six trials see some faults and miss others
    assert sum(whole.values()) == sum(1 for _ in pf.faults(ps))  # the shards are a partition
    assert (whole["identical"] > 0) == (make == "synthetic-balanced")


def test_fault_model():
    """The faults are what the module says: counts per (array, family), pad bytes untouched, the
    LSB faults go inwards at the storage limits, and a swap of equal neighbours is identical."""
    ps = pf.ident_set(7, C=5, T=130, N=3, weight_bits=4)
    d = ps.dims
    ps.l1_weight_align[0, 0], ps.l1_weight_align[0, 1] = 7, -8
    ps.l4_weight[2, 3] = ps.l4_weight[2, 4]
    n, identical = {}, []
    for ft in pf.faults(ps):
        n[ft[:2]] = n.get(ft[:2], 0) + 1
        q = pf.apply(ps, ft)
        if q is None:  # only a swap of equal neighbours
            assert ft[1] == "swap" and ft[3][0][1] == ft[3][1][1]
            identical.append(ft[:3])
            continue
        assert q.to_blob() != ps.to_blob()
        assert not q.l1_weight_align[:, d.C:].any()
        assert not q.l5_weight.reshape(d.N, d.F2, d.T64_ALIGN)[:, :, d.T64:].any()
        if ft[:3] == ("w1", "lsb", (0, 0, 1)):
            assert q.l1_weight_align[0, 0] == 6
        if ft[:3] == ("w1", "lsb", (0, 1, -1)):
            assert q.l1_weight_align[0, 1] == -7
    assert ("w4", "swap", (2, 3, 1)) in identical
    F, C, N, T64 = d.F2, d.C, d.N, d.T64
    assert n[("w1", "lsb")] == 2 * F * C and n[("w1", "zero")] == F * C
    assert n[("w1", "swap")] == (F - 1) * C + F * (C - 1)
    assert n[("w2", "swap")] == 15 * 64 + 16 * 63 and n[("w3", "swap")] == 15 * 16 + 16 * 15
    assert n[("w4", "swap")] == 2 * 15 * 16
    assert n[("w5", "swap")] == (N - 1) * F * T64 + N * (F - 1) * T64 + N * F * (T64 - 1)
    assert n[("l5_bias", "lsb")] == 2 * N and n[("l5_bias", "swap")] == N - 1
    assert all(n[(a, "swap")] == F - 1 for a in pf.CONSTS) and all(n[(a, "scalar")] == 2 for a in pf.SCALARS)


def test_ident_sets_differ_from_their_neighbours_by_construction():
    """Whatever the seed: no weight is zero, and no element of any array equals its successor along
    any axis (plain BN: after the shift by 3 that branch applies to factors and offsets)."""
    for seed in range(6):
        for kw in ({}, dict(reorder_bn=False), dict(weight_bits=4)):
            ps = pf.ident_set(seed, C=6, T=200, N=4, **kw)
            for a in pf.WEIGHTS + ("l5_bias",) + pf.CONSTS:
                v = pf.view(ps, a).astype(np.int64)
                if a in pf.WEIGHTS:
                    assert (v != 0).all(), a
                if not ps.reorder_bn and a[:2] in ("l2", "l4"):
                    v = v >> 3
                for ax in range(v.ndim):
                    assert (np.diff(v, axis=ax) != 0).all(), (a, ax, kw)


def _jobs():
    return [(pf.audit_pcase, i, (k, SHARDS)) for i in range(len(pf.PCASES)) for k in range(SHARDS)] + \
           [(pf.audit_record, i, (k, SHARDS)) for i in range(len(pf.RECORD)) for k in range(SHARDS)]


@pytest.fixture(scope="module")
def audits():
    t0 = time.perf_counter()
    jobs = _jobs()
    workers = min(16, os.cpu_count() or 1, len(jobs))
    # fresh interpreters (spawn), which inherit sys.path but nothing this process has opened
    with pf.single_threaded_children():
        with concurrent.futures.ProcessPoolExecutor(workers, mp_context=multiprocessing.get_context("spawn")) as pool:
            futs = [pool.submit(fn, i, shard) for fn, i, shard in jobs]
            parts = [f.result() for f in futs]
    res = {}
    for i, name in enumerate(NAMES):
        res[name] = pf.merge_pcase(parts[i * SHARDS: (i + 1) * SHARDS])
    base = len(NAMES) * SHARDS
    for i, name in enumerate(pf.RECORD):
        ps_ = parts[base + i * SHARDS: base + (i + 1) * SHARDS]
        res[name] = dict(ps_[0], res=pf.merge(p["res"] for p in ps_), seconds=sum(p["seconds"] for p in ps_))
    res["__wall__"] = time.perf_counter() - t0
    res["__workers__"] = workers
    return res


@pytest.mark.parametrize("name", NAMES)
def test_every_fault_is_seen(name, audits):
    """No identical and no unseen fault in any family, with the trials of the case and no more (at
    most 4096); at most 5 % of the logits on a rail; the C oracle, the GPU tests' reference,
    returns the golden model's logits on the first 64 trials.  Exact division: what is excluded
    are faults on the three moved filters alone."""
    r = audits[name]
    case = pf.PCASES[NAMES.index(name)]
    _, ps, x = case
    try:
        assert set(k[1] for k in r["res"]) == set(pf.FAMILIES)
        bad = {k: (v["unseen"], v["identical"], v["unseen_list"]) for k, v in r["res"].items() if v["unseen"] or v["identical"]}
        assert not bad, f"(unseen, identical, first unseen) per (array, family): {bad}"
        assert r["trials"] <= len(x) <= 4096 and len(x) % 64 == 0
        assert r["excluded"] <= r["moved_faults"] and (case.exact or r["excluded"] == 0)
        z = oracle.COracle(ps).batch(pack_trials(x), nthreads=NTH)
        np.testing.assert_array_equal(z[:64], r["z64"])
        rail = float(((z == 127) | (z <= G._lo(ps))).mean())
        print(f"{name}: B {len(x)}, trials used {r['trials']}, faults {pf.totals(r['res'])}, excluded {r['excluded']}, "
              f"logits on a rail {rail:.4f}, {r['seconds']:.1f} s")
        assert rail <= 0.05
        r["rail"] = rail
    finally:
        case.drop()


def test_variant_cases_have_their_flags():
    """The variants are what their names say (the kernel families they select are asserted on the
    GPU), and the geometries cover what they are there for."""
    for case in pf.PCASES:
        ps = case.ps
        assert ps.reorder_bn == ("plain" not in case.name)
        assert ps.weight_bits == (4 if "int4" in case.name else 8)
        assert not ps.clip_balanced
        if case.exact:
            moved = [int((np.abs(getattr(ps, f"l{k}_offset").astype(np.int64)) >= 1 << 22).sum()) for k in (1, 2, 4)]
            assert moved == [1, 1, 1] and len(case.moved) == 3
        case.drop()
    dims = [c.dims for c in pf.PCASES]
    # the four arms of the general layer-1 loader, layer 2 with tail tiles only, a full tile only,
    # and both (NB2 = ceil(T8 / 4) = 4, 17, 33), one, three and sixteen classes
    assert {5, 24, 40, 64} <= {C for C, _, _ in dims}
    assert {4, 17, 33} <= {-(-(T // 8) // 4) for _, T, _ in dims}
    assert {1, 3, 16} <= {N for _, _, N in dims}


def _line(name, res):
    arr = lambda a: " ".join(f"{fam} {res[(a, fam)]['seen']}/{res[(a, fam)]['seen'] + res[(a, fam)]['unseen']}"
                             f"({res[(a, fam)]['identical']} id)" for fam in pf.FAMILIES if (a, fam) in res)
    return f"{name}\n" + "".join(f"    {a:<10} {arr(a)}\n" for a in pf.WEIGHTS + ("l5_bias",) + pf.CONSTS + pf.SCALARS)


def test_record_baseline(audits):
    """A record, not a gate: what the inputs of existing tests let the logits see of the same
    faults (the certified activation cases 5x77 and 17x130, and two calibrated sets with the 37
    trials of test_other_geometries_and_variants).  Asserts only that the new cases see strictly
    more: each of them sees every fault, each of those misses some."""
    frac = {}
    for name in pf.RECORD:
        t = pf.totals(audits[name]["res"])
        frac[name] = t["seen"] / (t["seen"] + t["unseen"] + t["identical"])
        print(f"{name}: {t}")
        assert t["unseen"] + t["identical"] > 0
    for name in NAMES:
        t = pf.totals(audits[name]["res"])
        mine = t["seen"] / (t["seen"] + t["unseen"] + t["identical"] + audits[name]["excluded"])
        assert mine > max(frac.values())
    if os.environ.get("OBSERVABILITY_RECORD") == "1":
        with open(os.path.join(ROOT, "profiles", "param_observability.txt"), "w") as f:
            f.write("Observability of the parameters (tests/param_faults.py), written by\n"
                    "OBSERVABILITY_RECORD=1 pytest tests/test_param_observability_cpu.py\n\n"
                    f"whole audit fixture: {audits['__wall__']:.1f} s wall on {audits['__workers__']} worker processes, "
                    f"{SHARDS} shards per audit\n\n"
                    "certified cases: B = trials of the case (what the audit needed, in chunks of 64), faults seen /\n"
                    "unseen / identical over all families, excluded (exact division: unseen faults on the moved\n"
                    "filters alone, of so many such faults), logits on a rail, audit seconds (all shards, one thread each)\n")
            for name in NAMES:
                r = audits[name]
                t = pf.totals(r["res"])
                f.write(f"{name:<14} B {r['B']:5d}  used {r['trials']:5d}  seen {t['seen']:6d}  unseen {t['unseen']}  "
                        f"identical {t['identical']}  excluded {r['excluded']:3d} of {r['moved_faults']:4d}  "
                        f"rail {r.get('rail', float('nan')):.4f}  {r['seconds']:6.1f} s\n")
            f.write("\nbaseline: the same faults on the inputs of existing tests, per array and family seen/testable"
                    " (identical)\n")
            for name in pf.RECORD:
                r = audits[name]
                f.write(_line(f"{name} ({r['B']} trials, {r['seconds']:.1f} s)", r["res"]))
