"""What the windows-through-a-bank test modules share (tests/test_windows_bank_cpu.py,
tests/test_gpu_windows_bank.py): seven recordings per geometry laid along time at multiples of 16
samples, each under its own set of support_bank's five, their sliding windows at hop 3, a NumPy
restatement of the layout and lists (net_bank_windows_starts, net_bank_windows_lists) and, computed
once per geometry, the C oracle's logits of every window under every set and its layer-1 output of
every sample under every set.  The reference of a row is always the oracle of the window's set on
the materialised window, never another GPU entry."""
import functools

import numpy as np

import oracle
import support_bank as sb
from support import want, windows_at

GEOMETRIES = sb.GEOMETRIES
HOP = 3  # from the aligned starts: every onset residue mod 4, thirteen of the sixteen mod 16
# an equal-set neighbour (1, 1), a set that comes back (0), one recording of exactly T and one
# shorter than T (blocks but no window)
SETS = (0, 1, 1, 3, 4, 0, 2)
DELTAS = (17, 0, -1, 38, 9, 16, 31)
W = 41


def lengths(T):
    return [T + d for d in DELTAS]


def layout(lens, sets, T, hop, n_sets=len(sb.SEEDS)):
    """NumPy restatement of the C helpers: (starts int64[R], L, blk_set int32[ceil(L / 16)], onsets
    int64[W], first int64[R + 1])."""
    R = len(lens)
    starts = np.zeros(R, np.int64)
    for r in range(1, R):
        starts[r] = (int(starts[r - 1]) + lens[r - 1] + 15) // 16 * 16
    L = int(starts[-1]) + lens[-1]
    nb = (L + 15) // 16
    blk_set = np.full(nb, -7, np.int32)
    onsets, first = [], [0]
    for r in range(R):
        assert 0 <= sets[r] < n_sets
        hi = nb if r == R - 1 else int(starts[r + 1]) // 16
        blk_set[int(starts[r]) // 16: hi] = sets[r]
        n = 0 if lens[r] < T else (lens[r] - T) // hop + 1
        onsets += [int(starts[r]) + k * hop for k in range(n)]
        first.append(len(onsets))
    assert (blk_set != -7).all()
    return starts, L, blk_set, np.array(onsets, np.int64), np.array(first, np.int64)


@functools.lru_cache(maxsize=None)
def case(C, T):
    """(x [C][L] int8 with the pad samples random too, starts, L, blk_set, onsets, first, the set of
    every window), read-only."""
    starts, L, blk_set, onsets, first = layout(lengths(T), SETS, T, HOP)
    x = np.random.default_rng([C, T, 79]).integers(-127, 128, size=(C, L), dtype=np.int8)
    set_of = np.concatenate([np.full(int(first[r + 1] - first[r]), SETS[r], np.int64) for r in range(len(SETS))])
    assert len(onsets) == W == len(set_of) and L % 16 != 0
    for a in (x, starts, blk_set, onsets, first, set_of):
        a.setflags(write=False)
    return x, starts, L, blk_set, onsets, first, set_of


def tabulate(sets, x, onsets, T):
    """[set][window][N]: the oracle's logits of the windows of x at `onsets` under every set."""
    wins = windows_at(x, onsets, T)
    return np.stack([want(ps, wins) for ps in sets])


@functools.lru_cache(maxsize=None)
def table(C, T, N):
    """tabulate for the geometry's case and support_bank.sets(C, T, N).  Computed once, read-only."""
    x, _, _, _, onsets, _, _ = case(C, T)
    t = tabulate(sb.sets(C, T, N), x, onsets, T)
    t.setflags(write=False)
    return t


def reference(tab, set_of):
    """Row i: the logits of window i under set set_of[i]."""
    so = np.asarray(set_of, np.int64)
    return tab[so, np.arange(len(so))]


def layer1_of(ps, x_ct):
    """[16][L]: the oracle's net_layer1 output of every sample of x_ct [C][L] under ps (layer 1 sees
    one sample at a time; the oracle takes T of them per call, the last call zero-padded)."""
    d = ps.dims
    co = oracle.COracle(ps)
    L = x_ct.shape[1]
    out = np.zeros((16, L), np.int8)
    for t0 in range(0, L, d.T):
        n = min(d.T, L - t0)
        chunk = np.zeros((d.C, d.T), np.int8)
        chunk[:, :n] = x_ct[:, t0: t0 + n]
        out[:, t0: t0 + n] = co.layer1(oracle.to_tc_align(chunk, d.C_ALIGN))[:, :n]
    return out


def workspace(sets, x_ct, blk_set, n_sets=None):
    """[16][16 ceil(L / 16)]: what the entry leaves in ws: layer 1 of each block's samples under the
    block's set, zeros for a block whose entry is outside the bank and from sample L on."""
    L = x_ct.shape[1]
    n_sets = len(sets) if n_sets is None else n_sets
    out = np.zeros((16, len(blk_set) * 16), np.int8)
    per_set = {}
    for b, s in enumerate(np.asarray(blk_set).tolist()):
        if 0 <= s < n_sets:
            if s not in per_set:
                per_set[s] = layer1_of(sets[s], x_ct)
            hi = min(16 * b + 16, L)
            out[:, 16 * b: hi] = per_set[s][:, 16 * b: hi]
    return out


def adjacent_pairs():
    """Every ordered pair (a, b), a != b, of sets whose recordings lie next to each other."""
    out = set()
    for a, b in zip(SETS, SETS[1:]):
        if a != b:
            out |= {(a, b), (b, a)}
    return sorted(out)
