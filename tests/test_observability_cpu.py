"""Certifies the inputs of tests/test_gpu_observability.py on the CPU: for every entry of
observability.CASES the logits of the NumPy golden model change under a one-LSB mutation (+1 and
-1) of every audited live element of every intermediate layer, in some trial.  Only then does
``logits == oracle`` on the GPU say that every such element was computed right.  This is a
condition on the inputs, met by the reference alone; no kernel runs here.

The audits are independent and take seconds each, so one module fixture runs them in a process
pool (at most 16 workers).  With OBSERVABILITY_RECORD=1 the measured figures are written to
profiles/observability.txt.
"""
import concurrent.futures
import multiprocessing
import os
import time

import numpy as np
import pytest

import observability as ob
import oracle
from mibminet.params import ParamSet, pack_trials
from oracle import golden_np as G
from support import NTH, tile_sweep

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = [c.name for c in ob.CASES]


def _rng_x(ps, B, seed):
    return np.random.default_rng(seed).integers(-128, 128, size=(B, ps.dims.C, ps.dims.T)).astype(np.int8)


@pytest.mark.parametrize("make", ["probe", "probe-plain-exact", "synthetic-balanced"])
def test_audit_matches_brute_force(make):
    """The local recomputation against "mutate one element, run golden_np downstream": the same
    verdict on every site of every layer for both deltas (probe and calibrated sets, both BN
    branches, both clips, a w4 that is no permutation)."""
    if make == "probe":
        ps, x = ob.probe_set(3, C=3, T=77, N=3), None
    elif make == "probe-plain-exact":
        base = ob.probe_set(5, C=4, T=90, N=2, reorder_bn=False)
        x = _rng_x(base, 128, 2)
        ps, x = ob.exact_probe_set(base, x, 5), x[:6]
    else:
        ps, x = ParamSet.synthetic(3, C=3, T=77, N=3, clip_balanced=True), None
    x = _rng_x(ps, 6, 1) if x is None else x
    sites = ob.full_sites(ps)
    sites[3][:] = True  # the dropped y3 tail too: never seen, in both versions
    fast, slow = ob.audit(ps, x, sites, chunk=4), ob.audit_brute(ps, x, sites)
    for key in slow:
        np.testing.assert_array_equal(fast[key], slow[key], err_msg=str(key))
        if key[0] == 3:
            assert not slow[key][:, 8 * ps.dims.T64:].any()
    assert any(m.any() for m in slow.values()) and not all(m.all() for m in slow.values())


@pytest.fixture(scope="module")
def audits():
    t0 = time.perf_counter()
    workers = min(16, os.cpu_count() or 1, len(ob.CASES))
    # fresh interpreters (spawn), which inherit sys.path but nothing this process has opened
    with concurrent.futures.ProcessPoolExecutor(workers, mp_context=multiprocessing.get_context("spawn")) as pool:
        res = {r["name"]: r for r in pool.map(ob.audit_case, range(len(ob.CASES)))}
    res["__wall__"] = time.perf_counter() - t0
    res["__workers__"] = workers
    return res


@pytest.mark.parametrize("name", NAMES)
def test_every_audited_site_is_seen(name, audits):
    """Zero unseen audited live sites for +1 and for -1, with the trials of the case and no more;
    the weights leave nothing but the y3 tail without a path to a logit; at most 5 % of the
    logits sit on a rail; and the C oracle, the GPU tests' reference, returns the golden model's
    logits on these inputs."""
    r = audits[name]
    case = ob.CASES[NAMES.index(name)]
    _, ps, x = case
    try:
        assert all(r["live"].values()), r["live"]
        assert r["unseen"] == {key: 0 for key in r["unseen"]}, f"unseen audited sites {r['unseen']} of {r['sites']}"
        assert r["trials"] <= len(x) <= 4096
        z = oracle.COracle(ps).batch(pack_trials(x), nthreads=NTH)
        np.testing.assert_array_equal(z[:64], r["z64"])
        rail = float(((z == 127) | (z <= G._lo(ps))).mean())
        print(f"{name}: B {len(x)}, trials used {r['trials']}, audited {r['sites']}, logits on a rail {rail:.4f}, "
              f"{r['seconds']:.1f} s")
        assert rail <= 0.05
        r["rail"] = rail
    finally:
        case.drop()


def test_variant_cases_have_their_flags():
    """The variants are what their names say (the kernel families they select are asserted on the
    GPU)."""
    for case in ob.CASES:
        ps = case.ps
        assert ps.reorder_bn == case.kw.get("reorder_bn", "plain" not in case.name)
        assert ps.weight_bits == (4 if "int4" in case.name else 8)
        if "balanced" in case.name:
            assert ps.clip_balanced
        if case.exact:
            moved = [int((np.abs(getattr(ps, f"l{k}_offset").astype(np.int64)) >= 1 << 22).sum()) for k in (1, 2, 4)]
            assert moved == [1, 1, 1]
        case.drop()


def _baseline():
    """test_gpu_general.test_layer2_tile_sweep's own inputs (its parameter and input seeds, 7
    trials) at the residues the certified cases share with it: sites of the last 16 y1 samples and
    the last 4 y2 columns that a one-LSB mutation makes visible (both deltas counted)."""
    out = {}
    for r in ob.SWEEP_RESIDUES:
        C, T, N, kw = tile_sweep()[r]
        ps = ParamSet.synthetic(seed=7 * C + T + N, C=C, T=T, N=N, **kw)
        x = _rng_x(ps, 7, C * N)
        sites = {k: np.zeros_like(m) for k, m in ob.full_sites(ps).items()}
        sites[1][:, -16:] = True
        sites[2][:, -4:] = True
        seen = ob.audit(ps, x, sites)
        out[r] = {k: (int(sum(seen[(k, s)].sum() for s in ob.DELTAS)), 2 * int(sites[k].sum())) for k in (1, 2)}
    return out


def test_record_baseline(audits):
    """A record, not a gate: what the calibrated sets of test_layer2_tile_sweep let the logits see
    of layer 2's tail tiles, beside the certified cases of the same geometries.  Asserts only that
    the certified cases see strictly more."""
    base = _baseline()
    lines = []
    tot = {1: [0, 0], 2: [0, 0]}
    for r in ob.SWEEP_RESIDUES:
        cert = next(v for k, v in audits.items() if k.startswith(f"sweep{r}-"))
        for k in (1, 2):
            seen, of = base[r][k]
            assert cert["tail"][k] >= seen
            tot[k][0] += seen
            tot[k][1] += cert["tail"][k]
            lines.append(f"{cert['name']:<18} y{k} tail: test_layer2_tile_sweep inputs {seen:4d} of {of}, "
                         f"certified case {cert['tail'][k]:4d} of {of}")
    # a calibrated set at the certified 5x77 geometry: what 8 and 256 uniform trials make visible
    ps = ParamSet.synthetic(seed=5 * 77 + 16, C=5, T=77, N=16)
    cert = audits["5x77"]
    for B in (8, 256):
        seen = ob.audit(ps, _rng_x(ps, B, 5 + 77))
        n = {k: sum(int(seen[(k, s)].sum()) for s in ob.DELTAS) for k in (1, 2, 3, 4)}
        assert all(n[k] <= 2 * cert["sites"][k] for k in n) and (B > 8 or n[1] < 2 * cert["sites"][1])
        lines.append(f"5x77 ParamSet.synthetic, {B:3d} trials: " +
                     ", ".join(f"y{k} {n[k]} of {2 * cert['sites'][k]}" for k in n) + " (certified case: all)")
    print("\n".join(lines))
    assert tot[1][0] < tot[1][1] and tot[2][0] < tot[2][1]
    if os.environ.get("OBSERVABILITY_RECORD") == "1":
        with open(os.path.join(ROOT, "profiles", "observability.txt"), "w") as f:
            f.write("Observability of the parity tests (tests/observability.py), written by\n"
                    "OBSERVABILITY_RECORD=1 pytest tests/test_observability_cpu.py\n\n"
                    f"whole audit fixture: {audits['__wall__']:.1f} s wall on {audits['__workers__']} worker processes\n\n"
                    "certified cases: B = trials of the case (what the audit needed, in chunks of 64), audited\n"
                    "live sites per layer, unseen sites (both deltas), logits on a rail, audit seconds (one process)\n")
            for name in NAMES:
                r = audits[name]
                f.write(f"{name:<18} B {r['B']:5d}  sites y1 {r['sites'][1]:5d} y2 {r['sites'][2]:5d} y3 {r['sites'][3]:5d} "
                        f"y4 {r['sites'][4]:4d}  unseen {sum(r['unseen'].values())}  rail {r.get('rail', float('nan')):.4f}  "
                        f"{r['seconds']:5.1f} s\n")
            f.write("\nbaseline: sites (x 2 deltas) of the last 16 y1 samples and the last 4 y2 columns that change a logit\n")
            f.write("\n".join(lines) + "\n")
