"""What the parameter-bank test modules share (tests/test_bank_cpu.py, tests/test_gpu_bank.py,
tests/test_bank_host_sanitizers.py): the geometries, the five sets of each, the set_of patterns, one
source of epochs per geometry and, computed once per geometry, the C oracle's logits of every epoch
under every set, from which the reference of any set_of list is read off.  The reference is always
the oracle of set set_of[e] on the materialised epoch e, never another GPU entry."""
import dataclasses
import functools

import numpy as np
import pytest

from mibminet import lib
from mibminet.params import ParamSet
from support import epochs_of, want

# C, T, N: the smallest shapes at which each mechanism can go wrong (minimum T and one layer-2 tail
# tile; tail tiles at two workgroups per CU; a compiled shape on the general image; every lane a
# channel; one workgroup per CU, groups of four layer-1 blocks and the largest layer-5 reload)
GEOMETRIES = [(8, 64, 2), (19, 480, 3), (22, 1125, 4), (64, 480, 2), (4, 4096, 16)]
SEEDS = (101, 102, 103, 104, 105)
E_MAX = 48
SIZES = (23, 48)  # a list takes the first E epochs of the geometry's source
LAYERS = {k: tuple(f.name for f in dataclasses.fields(ParamSet) if f.name.startswith(f"l{k}_")) for k in range(1, 6)}


@functools.lru_cache(maxsize=None)
def sets(C, T, N, **kw):
    """The five sets of a geometry (kw as ParamSet.synthetic takes it)."""
    return tuple(ParamSet.synthetic(seed=s, C=C, T=T, N=N, **kw) for s in SEEDS)


@pytest.fixture(scope="module")
def banks(gpu):
    """The five-set banks of the module, by geometry, built once and closed at the end."""
    cache = {}

    def get(C, T, N):
        if (C, T, N) not in cache:
            cache[(C, T, N)] = lib.Bank(sets(C, T, N))
        return cache[(C, T, N)]

    yield get
    for b in cache.values():
        b.close()


def _extreme(C, T, N, **kw):
    return tuple(ParamSet.synthetic_extreme(seed=s, C=C, T=T, N=N, mids=3, **kw) for s in SEEDS)


# the build variants of a bank, by name: the five sets of a geometry
VARIANTS = {
    "plain-bn": lambda C, T, N: sets(C, T, N, reorder_bn=False),
    "plain-bn-balanced": lambda C, T, N: sets(C, T, N, reorder_bn=False, clip_balanced=True),
    "balanced": lambda C, T, N: sets(C, T, N, clip_balanced=True),
    "int4": lambda C, T, N: sets(C, T, N, weight_bits=4),
    "all-exact": _extreme,
    "all-exact-plain-bn": lambda C, T, N: _extreme(C, T, N, reorder_bn=False),
    # two float sets among three that need exact division: every slice runs the exact form
    "mixed": lambda C, T, N: sets(C, T, N)[:1] + _extreme(C, T, N)[1:3] + sets(C, T, N)[3:4] + _extreme(C, T, N)[4:],
}
VARIANT_GEOMETRIES = [(19, 480, 3), (4, 4096, 16)]
VARIANT_E = 23
EXACT = ("all-exact", "all-exact-plain-bn", "mixed")


def hybrid(a, b, k):
    """Set a with layer k's arrays from set b."""
    return dataclasses.replace(a, **{name: getattr(b, name) for name in LAYERS[k]})


@functools.lru_cache(maxsize=None)
def case(C, T):
    """The epochs of a geometry: (source [C + 2][L] int8, E_MAX unsorted onsets, channel rows).  The
    source is two rows taller than the network and its epochs overlap.  Uniform int8 samples from
    the first seed (of 77, 78, ...) with which every geometry passes the certification of
    tests/test_bank_cpu.py: at 8 x 64 with two classes seeds 77 and 78 give all-zero logit rows."""
    rng = np.random.default_rng([C, T, 79])
    R, L = C + 2, T + 211
    src = rng.integers(-127, 128, size=(R, L), dtype=np.int8)
    channels = tuple(int(c) for c in rng.permutation(R)[:C])
    last = R * L - (max(channels) * L + T)
    onsets = [int(v) for v in rng.integers(0, last + 1, size=E_MAX)]
    onsets[1], onsets[2] = last, 0
    return src, tuple(onsets), channels


def last_onset(C, T):
    src, _, channels = case(C, T)
    return src.size - (max(channels) * src.shape[1] + T)


@functools.lru_cache(maxsize=None)
def epochs(C, T):
    src, onsets, channels = case(C, T)
    e = epochs_of(src, onsets, channels, src.shape[1], T)
    e.setflags(write=False)
    return e


@functools.lru_cache(maxsize=None)
def table(C, T, N, **kw):
    """[set][epoch][N]: the oracle's logits of every epoch of case(C, T) under every set of
    sets(C, T, N, **kw).  Computed once, read-only."""
    t = np.stack([want(ps, epochs(C, T)) for ps in sets(C, T, N, **kw)])
    t.setflags(write=False)
    return t


def reference(tab, set_of):
    """Row e of the result: the logits of epoch e under set set_of[e]."""
    so = np.asarray(set_of, np.int64)
    return tab[so, np.arange(len(so))]


def patterns(E, n=len(SEEDS)):
    """The set_of lists of E epochs over n sets, by name."""
    rng = np.random.default_rng([E, n])
    grouped = np.sort(np.arange(E) * n // E)
    unused = grouped.copy()
    unused[unused == 2] = 4  # set 2 unused, set 4 in two groups
    return {
        "grouped": grouped,
        "alternating": np.arange(E) % n,
        "random": rng.integers(0, n, size=E),
        "all-on-3": np.full(E, 3),
        "one-unused": unused,
        "groups-of-one": np.concatenate([np.arange(n), np.sort(rng.integers(0, n, size=E - n))]),
    }


def adjacent_pairs(E_list=SIZES):
    """Every ordered pair (a, b), a != b, of sets that some pattern places next to each other."""
    out = set()
    for E in E_list:
        for so in patterns(E).values():
            out |= {(int(a), int(b)) for a, b in zip(so, so[1:]) if a != b}
    return sorted(out)
