"""TEST INFRASTRUCTURE ONLY — how much of each parameter array the logits can see.

A weight, factor or offset reaches a kernel through hand-laid MFMA fragments and lane-indexed
tables (csrc/images.hpp), so what can go wrong is a band edge, a tap or channel taken from its
neighbour, or a constant read for the wrong filter.  A parity test ``logits == oracle`` notices
such an error only if the parameter set makes it visible.  ``faults`` lists single changes of a
ParamSet, ``audit_params`` measures on the reference alone (no kernel is involved) which of them
change a logit of some trial, ``ident_set`` builds sets whose neighbours differ along every axis
of every array by construction, and ``PCASES`` is the fixed list that
tests/test_param_observability_cpu.py certifies and tests/test_gpu_param_observability.py runs.

A fault is (array, family, index, changes): ``changes`` are (index, new value) pairs of that
array.  Arrays: w1 [F][C], w2 [F][64], w3 [F][16] (storage order), w4 [out][in],
w5 [N][F][T64], l5_bias, l{1,2,4}_factor, l{1,2,4}_offset, l3_factor, l5_factor.  Families:

* lsb     every weight and bias element +1 and -1 (inwards at the storage limit);
* zero    every weight element replaced by 0 (a dropped band edge or tap);
* swap    every weight element exchanged with its successor along each axis of its array, and
          every per-filter factor or offset and every bias with its successor;
* scalar  l3_factor and l5_factor +-1.

Pad bytes are never touched.  A fault that leaves the set equal to the original, or that
ParamSet.__post_init__ rejects, is *identical*: no test on that set can see it.
"""
from __future__ import annotations

import copy
import functools
import time
from types import SimpleNamespace
from typing import Dict, Iterator, List, Optional, Tuple

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

import observability as ob
from mibminet.params import L2_TAPS, L3_TAPS, ParamSet
from oracle import golden_np as G

WEIGHTS = ("w1", "w2", "w3", "w4", "w5")
CONSTS = ("l1_factor", "l1_offset", "l2_factor", "l2_offset", "l4_factor", "l4_offset")
SCALARS = ("l3_factor", "l5_factor")
FAMILIES = ("lsb", "zero", "swap", "scalar")
_LAYER = {"w1": 1, "l1_factor": 1, "l1_offset": 1, "w2": 2, "l2_factor": 2, "l2_offset": 2, "w3": 3, "l3_factor": 3,
          "w4": 4, "l4_factor": 4, "l4_offset": 4, "w5": 5, "l5_bias": 5, "l5_factor": 5}
_ATTR = {"w1": "l1_weight_align", "w2": "l2_weight_reverse", "w3": "l3_weight", "w4": "l4_weight", "w5": "l5_weight"}
Fault = Tuple[str, str, tuple, tuple]


def view(ps: ParamSet, array: str) -> np.ndarray:
    """The live elements of ``array`` as a writable view of the ParamSet's storage."""
    d = ps.dims
    if array == "w1":
        return ps.l1_weight_align[:, : d.C]
    if array == "w2":
        return ps.l2_weight_reverse
    if array == "w3":
        return ps.l3_weight
    if array == "w4":
        return ps.l4_weight
    if array == "w5":
        return ps.l5_weight.reshape(d.N, d.F2, d.T64_ALIGN)[:, :, : d.T64]
    return getattr(ps, array)


def faults(ps: ParamSet) -> Iterator[Fault]:
    """Every fault of the model, in a fixed order."""
    wlim = (-8, 7) if ps.weight_bits == 4 else (-128, 127)
    for array in WEIGHTS + ("l5_bias",):
        a = view(ps, array).astype(np.int64)
        lo, hi = wlim if array != "l5_bias" else (-128, 127)
        for idx in np.ndindex(a.shape):
            v = int(a[idx])
            yield array, "lsb", idx + (+1,), ((idx, v - 1 if v == hi else v + 1),)
            yield array, "lsb", idx + (-1,), ((idx, v + 1 if v == lo else v - 1),)
            if array != "l5_bias":
                yield array, "zero", idx, ((idx, 0),)
        for axis in range(a.ndim):
            for idx in np.ndindex(a.shape):
                if idx[axis] + 1 < a.shape[axis]:
                    nxt = idx[:axis] + (idx[axis] + 1,) + idx[axis + 1:]
                    yield array, "swap", idx + (axis,), ((idx, int(a[nxt])), (nxt, int(a[idx])))
    for array in CONSTS:
        a = getattr(ps, array).astype(np.int64)
        for f in range(len(a) - 1):
            yield array, "swap", (f,), (((f,), int(a[f + 1])), ((f + 1,), int(a[f])))
    for array in SCALARS:
        for s in (+1, -1):
            yield array, "scalar", (s,), (((), getattr(ps, array) + s),)


def apply(ps: ParamSet, fault: Fault) -> Optional[ParamSet]:
    """The faulted copy of ``ps``; None if it equals ``ps`` or is no valid ParamSet."""
    array, _, _, changes = fault
    if array in SCALARS:
        if changes[0][1] == 0:
            return None
        q = copy.copy(ps)
        setattr(q, array, int(changes[0][1]))
        return q
    if all(int(view(ps, array)[idx]) == val for idx, val in changes):
        return None
    q = copy.copy(ps)  # the other arrays are shared, none is written
    setattr(q, _ATTR.get(array, array), getattr(ps, _ATTR.get(array, array)).copy())
    a = view(q, array)
    for idx, val in changes:
        a[idx] = val
    try:
        ParamSet.__post_init__(q)
    except ValueError:
        return None
    return q


def rows_of(ps: ParamSet, fault: Fault) -> Tuple[int, ...]:
    """The filters (layer 4: outputs) whose parameters the fault changes; () for layer 5."""
    array, _, _, changes = fault
    if array == "l3_factor":
        return tuple(range(ps.dims.F2))
    if _LAYER[array] == 5:
        return ()
    return tuple(sorted({idx[0] for idx, _ in changes}))


# ---- the audit ----------------------------------------------------------------------------------
def _shim(q, R):
    """What ob._post2 / ob._post4 read of a ParamSet, for the filters R."""
    return SimpleNamespace(reorder_bn=q.reorder_bn, clip_balanced=q.clip_balanced,
                           l2_factor=q.l2_factor[R], l2_offset=q.l2_offset[R],
                           l4_factor=q.l4_factor[R], l4_offset=q.l4_offset[R])


def _taps(xpad, w, n):
    """sum_j w[r][j] xpad[b][r][u + j] for u < n: the depthwise cross-correlation of a few rows
    (xpad [B][R][n + taps - 1], w [R][taps]).  Where every sum stays below 2^24 it runs as float32
    GEMMs, exactly: blocks of ``taps`` outputs, each the product of its 2 taps - 1 inputs with the
    banded matrix of the filter."""
    B, R, taps = xpad.shape[0], xpad.shape[1], w.shape[1]
    if int(np.abs(w).sum(1).max()) * int(np.abs(xpad).max(initial=0)) >= 1 << 24:
        out = np.zeros((B, R, n), np.int64)
        for j in range(taps):
            out += w[None, :, j: j + 1] * xpad[..., j: j + n]
        return out
    nb = -(-n // taps)
    xp = np.zeros((B, R, (nb + 1) * taps - 1), np.float32)
    xp[..., : n + taps - 1] = xpad[..., : n + taps - 1]
    win = sliding_window_view(xp, 2 * taps - 1, axis=-1)[:, :, ::taps]  # [B][R][nb][2 taps - 1]
    out = np.empty((B, R, nb * taps), np.int64)
    for r in range(R):
        band = np.zeros((2 * taps - 1, taps), np.float32)  # band[k][u] = w[r][k - u]
        for u in range(taps):
            band[u: u + taps, u] = w[r]
        out[:, r] = (win[:, r].reshape(B * nb, 2 * taps - 1) @ band).reshape(B, nb * taps)
    return out[..., :n]


class _Trials:
    """The unfaulted forward of some trials, and the forward of a faulted set from the first layer
    the fault touches on, for the filters it touches (the layers before the pointwise one are
    depthwise, so the other rows keep their values)."""

    def __init__(self, p, x):
        d = p.dims
        self.p = p
        x = np.asarray(x, np.int64)
        self.B = len(x)
        # layer 1 as a float32 GEMM: |dot| <= 64 x 128 x 128 = 2^20 is exact
        assert d.C <= 64
        self.xf = np.ascontiguousarray(x.transpose(1, 0, 2).reshape(d.C, -1), np.float32)
        self.y1 = G.layer1(p, x)
        self.y1pad = np.pad(self.y1, ((0, 0), (0, 0), (31, 32)))
        self.a2 = G.xcorr_same(self.y1, p.l2_weight_reverse, 31, 32)[..., : 8 * d.T8]
        self.y2 = G.layer2(p, self.y1)
        self.y3 = G.layer3(p, self.y2)
        self.b4 = np.einsum("bft,kf->bkt", self.y3, p.l4_weight.astype(np.int64), optimize=True)[..., : 8 * d.T64]
        self.y4 = G.layer4(p, self.y3)
        self.z = G.layer5(p, self.y4)

    def _y1(self, q, R):
        d = q.dims
        acc = (q.w1()[R].astype(np.float32) @ self.xf).reshape(len(R), self.B, d.T).transpose(1, 0, 2)
        return G.apply_factor_offset(acc.astype(np.int64), q.l1_factor[R], q.l1_offset[R], G._lo(q))

    def _y2(self, q, R, y1):
        d = q.dims
        a = _taps(np.pad(y1, ((0, 0), (0, 0), (31, 32))), q.l2_weight_reverse[R].astype(np.int64), 8 * d.T8)
        return ob._post2(_shim(q, R), a)

    def _y3(self, q, R, y2):
        a = _taps(np.pad(y2, ((0, 0), (0, 0), (7, 8))), q.w3_torch()[R].astype(np.int64), q.dims.T8)
        return G.apply_factor_offset(a, np.int64(q.l3_factor), lo=G._lo(q))

    def _y2_w2(self, q, R, changes):
        """Layer 2 of the rows R after ``changes`` of w2 alone: the cached sums plus one shifted copy
        of y1 per changed tap."""
        n = 8 * q.dims.T8
        a = self.a2[:, R].copy()
        for (f, j), val in changes:
            a[:, R.index(f)] += (val - int(self.p.l2_weight_reverse[f, j])) * self.y1pad[:, f, j: j + n]
        return ob._post2(_shim(q, R), a)

    def logits(self, q, fault):
        """The logits of the faulted set q = apply(p, fault) on these trials."""
        layer, R = _LAYER[fault[0]], list(rows_of(q, fault))
        if layer == 5:
            return G.layer5(q, self.y4)
        n4 = 8 * q.dims.T64
        y4 = self.y4.copy()
        if layer == 4:
            b = np.einsum("bft,kf->bkt", self.y3[..., :n4], q.l4_weight[R].astype(np.int64), optimize=True)
            y4[:, R] = ob._post4(_shim(q, R), b)
            return G.layer5(q, y4)
        if fault[0] == "w2":
            y = self._y2_w2(q, R, fault[3])
        else:
            y = self._y1(q, R) if layer == 1 else self.y1[:, R]
            y = self._y2(q, R, y) if layer <= 2 else self.y2[:, R]
        y = self._y3(q, R, y)
        dy3 = (y - self.y3[:, R])[..., :n4]
        b = self.b4 + np.einsum("brt,kr->bkt", dy3, q.l4_weight[:, R].astype(np.int64), optimize=True)
        return G.layer5(q, ob._post4(q, b))


def audit_params(ps: ParamSet, x, chunk: int = 64, stats: Optional[dict] = None, brute: bool = False,
                 excluded=lambda fault: False, shard: Tuple[int, int] = (0, 1)) -> Dict[Tuple[str, str], dict]:
    """x: int8 [B][C][T].  Per (array, family): ``seen`` (some logit of some trial differs under
    the fault), ``unseen`` and ``identical`` counts, and under ``unseen_list`` the unseen faults.
    Every fault is evaluated on the first ``chunk`` trials and only the unseen ones are carried on
    to later chunks; ``stats["trials"]`` receives the trials consumed until all were seen (B if
    some never was).  Faults for which ``excluded`` holds are audited too, but no chunk is run for
    their sake alone.  ``shard`` = (k, n): every n-th fault from the k-th on (the shards of one set
    are independent; ``merge`` adds them up).  ``brute``: the plain version, golden_np.forward of every faulted set on
    every trial."""
    out = {}
    todo: List[Tuple[Fault, ParamSet]] = []
    for i, ft in enumerate(faults(ps)):
        r = out.setdefault(ft[:2], dict(seen=0, unseen=0, identical=0, unseen_list=[]))
        if i % shard[1] != shard[0]:
            continue
        q = apply(ps, ft)
        if q is None:
            r["identical"] += 1
        else:
            todo.append((ft, q))
    used = 0
    if brute:
        z = G.forward(ps, np.asarray(x, np.int64))
        left = []
        for ft, q in todo:
            if (G.forward(q, np.asarray(x, np.int64)) != z).any():
                out[ft[:2]]["seen"] += 1
            else:
                left.append((ft, q))
        todo, used = left, len(x)
    for b0 in range(0, 0 if brute else len(x), chunk):
        if all(excluded(ft) for ft, _ in todo):
            break
        c = _Trials(ps, x[b0: b0 + chunk])
        used = min(len(x), b0 + chunk)
        left = []
        for ft, q in todo:
            if (c.logits(q, ft) != c.z).any():
                out[ft[:2]]["seen"] += 1
            else:
                left.append((ft, q))
        todo = left
    for ft, _ in todo:
        out[ft[:2]]["unseen"] += 1
        out[ft[:2]]["unseen_list"].append(ft)
    if stats is not None:
        stats["trials"] = used
    return out


def merge(parts):
    """The sum of the per-(array, family) results of the shards of one audit."""
    out = {}
    for res in parts:
        for key, r in res.items():
            o = out.setdefault(key, {k: type(v)() for k, v in r.items()})
            for k, v in r.items():
                o[k] += v
    return out


def totals(res) -> Dict[str, int]:
    return {k: sum(r[k] for r in res.values()) for k in ("seen", "unseen", "identical")}


# ---- parameter sets whose every element is identifiable -------------------------------------------
def _steps(rng, n, m):
    """n residues mod m whose neighbours differ: a walk with steps in 1 .. m - 1."""
    return np.cumsum(rng.integers(1, m, size=n)) % m


def _magnitudes(rng, shape, m=3):
    """1 .. m over ``shape`` with different values at any two neighbours along any axis: the sum
    of one neighbour-distinct walk per axis, mod m."""
    tot = np.zeros(shape, np.int64)
    for ax, n in enumerate(shape):
        tot += _steps(rng, n, m).reshape([-1 if i == ax else 1 for i in range(len(shape))])
    return 1 + tot % m


def _untie(a, lo, hi, zero_ok=False):
    """``a`` with every element that equals its predecessor along some axis (or is 0) stepped on
    to the next value in lo .. hi that does not, in index order (each element is compared with the
    elements before it, so one pass leaves no tie)."""
    a = np.array(a, np.int64)
    for idx in np.ndindex(a.shape):
        prev = {int(a[idx[:ax] + (idx[ax] - 1,) + idx[ax + 1:]]) for ax in range(a.ndim) if idx[ax] > 0}
        if not zero_ok:
            prev.add(0)
        v = int(a[idx])
        while v in prev:
            v = lo if v >= hi else v + 1
        a[idx] = v
    return a


def ident_set(seed: int, C: int, T: int, N: int, reorder_bn: bool = True, weight_bits: int = 8,
              l5_factor: Optional[int] = None) -> ParamSet:
    """observability.probe_set turned into a set whose every parameter element can be told from
    its neighbours and from zero: w1 keeps its calibrated values with ties and zeros stepped on;
    w2 and w3 keep their balanced signs and get magnitudes 1..3, w4 and w5 are dense over +-1..3,
    in each array the magnitude being a sum of one neighbour-distinct walk per axis mod 3, so two
    neighbours along any axis differ by construction; the factors and offsets of layers 2 and 4 are
    affine in a permutation of the filters (|l2_factor| = 16 + 2 perm, l2_offset = 1024 + 64 perm,
    |l4_factor| = 128 + 8 perm, l4_offset = 8192 + 512 perm, an offset of 64 factors each; the
    plain-BN branches, which divide by factor >> 3 and add offset >> 3, get |factor| = 8 (2 + a
    neighbour-distinct walk mod 3) with offset = 64 factor and 8 (20 + a walk mod 8) with offset =
    40 factor, so that neighbours still differ after the shift and a layer-4 element, a dense sum
    over 16 rows of y3, stays below 127, where the golden model clips and the reference C does
    not); layer 1's factors and offsets are stepped
    apart; the bias is a neighbour-distinct walk over -2 .. 2; l3_factor is doubled and l5_factor
    is about 1.5 sqrt(16 T64) unless given."""
    ps = ob.probe_set(seed, C, T, N, reorder_bn=reorder_bn, weight_bits=weight_bits)
    d = ps.dims
    F = d.F2
    rng = np.random.default_rng(seed + 7368787)
    wlo, whi = (-8, 7) if weight_bits == 4 else (-127, 127)
    ps.l1_weight_align[:, :C] = _untie(ps.w1(), wlo, whi)
    ps.l1_factor = _untie(ps.l1_factor, -(1 << 30), 1 << 30)
    ps.l1_offset = _untie(ps.l1_offset, -(1 << 30), 1 << 30, zero_ok=True)
    ps.l2_weight_reverse = np.sign(ps.l2_weight_reverse) * _magnitudes(rng, (F, L2_TAPS))
    ps.l3_weight = np.sign(ps.l3_weight) * _magnitudes(rng, (F, L3_TAPS))
    ps.l4_weight = rng.choice([-1, 1], (F, F)) * _magnitudes(rng, (F, F))
    w5 = np.zeros((N, F, d.T64_ALIGN), np.int64)
    w5[:, :, : d.T64] = rng.choice([-1, 1], (N, F, d.T64)) * _magnitudes(rng, (N, F, d.T64))
    ps.l5_weight = w5.reshape(N, -1)
    s2, s4 = np.sign(ps.l2_factor.astype(np.int64)), np.sign(ps.l4_factor.astype(np.int64))
    p2, p4 = rng.permutation(F), rng.permutation(F)
    if reorder_bn:
        ps.l2_factor, ps.l2_offset = s2 * (16 + 2 * p2), 1024 + 64 * p2
        ps.l4_factor, ps.l4_offset = s4 * (128 + 8 * p4), 8192 + 512 * p4
    else:  # per element, before the ReLU at 0: the offset carries the factor's sign
        f2, f4 = 2 + _steps(rng, F, 3), 20 + _steps(rng, F, 8)
        ps.l2_factor, ps.l2_offset = s2 * 8 * f2, s2 * 8 * 64 * f2
        ps.l4_factor, ps.l4_offset = s4 * 8 * f4, s4 * 8 * 40 * f4
    ps.l3_factor = 2 * ps.l3_factor
    ps.l5_bias = _steps(rng, N, 5) - 2
    ps.l5_factor = int(l5_factor) if l5_factor else max(1, int(round(1.5 * np.sqrt(F * d.T64))))
    ParamSet.__post_init__(ps)
    return ps


def calibrate_l5(ps: ParamSet, x, rail: float = 0.02) -> int:
    """The smallest l5_factor that keeps all but ``rail`` of the logits of the trials x strictly
    inside -120 .. 120: the dense w5 sums 16 T64 values of y4 whose mean does not cancel, so the
    factor follows the data (the golden model's y4 on x), not a formula."""
    y4 = G.layer4(ps, G.layer3(ps, G.layer2(ps, G.layer1(ps, np.asarray(x, np.int64)))))
    z = y4.reshape(len(y4), -1) @ ps.w5_flat().astype(np.int64).T + ps.l5_bias.astype(np.int64)
    return max(1, int(np.ceil(np.percentile(np.abs(z), 100.0 * (1.0 - rail)) / 120.0)))


def ident_exact_set(base: ParamSet, x, seed: int) -> Tuple[ParamSet, Tuple[int, int, int]]:
    """``base`` with one filter each of layers 1, 2 and 4 moved out of the float envelope by
    observability.exact_probe_set; w4 keeps its dense values (the second reader that function
    plants serves a permutation).  Returns the set and the moved filters (layer 1, 2, 4)."""
    ps = ob.exact_probe_set(base, x, seed)
    ps.l4_weight = base.l4_weight.copy()
    ParamSet.__post_init__(ps)
    moved = tuple(int(np.flatnonzero(np.abs(getattr(ps, f"l{k}_offset").astype(np.int64)) >= 1 << 22)[0])
                  for k in (1, 2, 4))
    return ps, moved


# ---- the certified cases --------------------------------------------------------------------------
class PCase(ob.Case):
    """(name, ps, x) as observability.Case, the set from ident_set."""

    @functools.cached_property
    def _built(self):
        C, T, N = self.dims
        ps = ident_set(self.seed + 1000 * C + T + N, C, T, N, **self.kw)
        head = ob.Case("", C, T, N, 128, seed=self.seed).x  # the first trials of x, whatever B is
        ps, moved = ident_exact_set(ps, head, self.seed) if self.exact else (ps, ())
        if "l5_factor" not in self.kw:
            ps.l5_factor = calibrate_l5(ps, head[:64])
        return ps, moved

    @property
    def ps(self) -> ParamSet:
        return self._built[0]

    @property
    def moved(self) -> Tuple[int, ...]:
        """Exact division: the moved filters of layers 1, 2 and 4."""
        return self._built[1]

    def excluded(self, fault: Fault) -> bool:
        """Exact division: a fault that touches only parameters of a moved filter of its own
        layer (such a filter's output takes two adjacent values, so its own weights are
        two-valued in effect)."""
        if not self.exact:
            return False
        layer, rows = _LAYER[fault[0]], rows_of(self.ps, fault)
        own = {1: {self.moved[0]}, 2: {self.moved[0], self.moved[1]}, 3: {self.moved[0], self.moved[1]},
               4: {self.moved[2]}}.get(layer, set())
        return bool(rows) and fault[0] != "l3_factor" and set(rows) <= own


GENERAL = ((5, 130, 16), (24, 544, 1), (40, 1056, 3), (64, 130, 3))
COMPILED = ((22, 1125, 4), (64, 480, 4))
VARIANT_GEOMETRIES = ((17, 130, 3), (64, 480, 4))
VARIANTS = {"plain": dict(reorder_bn=False), "int4": dict(weight_bits=4), "exact": dict(exact=True)}
# trials per case: what the audit needed (profiles/param_observability.txt), rounded up to chunks of 64
_B: Dict[str, int] = {"5x130": 64, "24x544": 64, "40x1056": 128, "64x130": 704, "22x1125": 256, "64x480": 128,
                      "17x130-plain": 64, "17x130-int4": 128, "17x130-exact": 320,
                      "64x480-plain": 64, "64x480-int4": 128, "64x480-exact": 128}
# per case, what the audit made necessary beside the recipe (seed, l5_factor): nothing so far
_TUNE: Dict[str, dict] = {}


def _pcases():
    out = []
    for C, T, N in GENERAL + COMPILED:
        out.append((f"{C}x{T}", C, T, N, {}))
    for C, T, N in VARIANT_GEOMETRIES:
        for v, kw in VARIANTS.items():
            out.append((f"{C}x{T}-{v}", C, T, N, kw))
    cases = []
    for name, C, T, N, kw in out:
        kw = dict(kw, **_TUNE.get(name, {}))
        cases.append(PCase(name, C, T, N, _B.get(name, 1024), seed=kw.pop("seed", 0), **kw))
    return cases


PCASES = _pcases()


def audit_pcase(i: int, shard: Tuple[int, int] = (0, 1)) -> dict:
    """One shard of the audit of PCASES[i] as plain numbers (a process-pool worker)."""
    t0 = time.perf_counter()
    case = PCASES[i]
    name, ps, x = case
    stats = {}
    res = audit_params(ps, x, stats=stats, excluded=case.excluded, shard=shard)
    excluded = 0
    for r in res.values():
        ex = [ft for ft in r["unseen_list"] if case.excluded(ft)]
        r["excluded"] = len(ex)
        r["unseen"] -= len(ex)
        r["unseen_list"] = [ft[:3] for ft in r["unseen_list"] if not case.excluded(ft)][:8]
        excluded += len(ex)
    moved_faults = sum(1 for ft in faults(ps) if case.excluded(ft)) if case.exact and shard[0] == 0 else 0
    return dict(name=name, res=res, trials=stats["trials"], B=len(x), seconds=time.perf_counter() - t0,
                excluded=excluded, moved_faults=moved_faults,
                z64=G.forward(ps, x[:64]) if shard[0] == 0 else None)


def merge_pcase(parts) -> dict:
    """The shards of one case's audit as one result: counts and seconds added, trials the largest."""
    parts = list(parts)
    return dict(parts[0], res=merge(p["res"] for p in parts), trials=max(p["trials"] for p in parts),
                seconds=sum(p["seconds"] for p in parts), excluded=sum(p["excluded"] for p in parts),
                moved_faults=sum(p["moved_faults"] for p in parts),
                z64=next(p["z64"] for p in parts if p["z64"] is not None))


# ---- the record: the same faults on the inputs of existing tests ------------------------------------
def _calibrated(C, T, N, B=37):
    """test_gpu_general.test_other_geometries_and_variants' own set and batch at (C, T, N)."""
    ps = ParamSet.synthetic(seed=C * T + N, C=C, T=T, N=N)
    return ps, np.random.default_rng(T + N).integers(-128, 128, size=(B, C, T)).astype(np.int8)


RECORD = ("certified 5x77", "certified 17x130", "ParamSet.synthetic 5x100 N=16", "ParamSet.synthetic 17x480 N=3")


def audit_record(i: int, shard: Tuple[int, int] = (0, 1)) -> dict:
    """The fault model on the inputs of existing tests (a process-pool worker): the certified
    activation cases 5x77 and 17x130 with their batches, and two calibrated sets with the 37 trials
    test_other_geometries_and_variants gives them."""
    t0 = time.perf_counter()
    if i < 2:
        _, ps, x = next(c for c in ob.CASES if c.name == ("5x77", "17x130")[i])
    else:
        ps, x = _calibrated(*((5, 100, 16), (17, 480, 3))[i - 2])
    res = audit_params(ps, x, shard=shard)
    for r in res.values():
        del r["unseen_list"]
    return dict(name=RECORD[i], res=res, B=len(x), seconds=time.perf_counter() - t0)


def single_threaded_children():
    """Context: worker processes started inside it run NumPy's BLAS on one thread each (a pool of
    single-row GEMMs on every core at once otherwise spends its time in the BLAS threads' waits)."""
    import contextlib
    import os

    @contextlib.contextmanager
    def ctx():
        names = ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS")
        old = {n: os.environ.get(n) for n in names}
        os.environ.update({n: "1" for n in names})
        try:
            yield
        finally:
            for n, v in old.items():
                os.environ.pop(n, None) if v is None else os.environ.__setitem__(n, v)
    return ctx()
