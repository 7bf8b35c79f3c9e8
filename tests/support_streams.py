"""What the live-stream test modules share (tests/test_streams_cpu.py, tests/test_gpu_streams.py,
tests/test_streams_host_sanitizers.py): a NumPy restatement of the arithmetic of a stream group (ring
size, the windows of a push, their onsets, validity by origin), five sessions per geometry under
sets (0, 1, 1, 3, 0) of support_bank's five, one fixed push schedule per geometry and, computed once
per geometry, the C oracle's logits of every sliding window of every session's concatenated chunks.
The reference of a row is always the oracle of the session's set on the materialised window, never
another GPU entry."""
import functools

import numpy as np

import support_bank as sb
from support import sliding_windows, want

GEOMETRIES = sb.GEOMETRIES
SETS = (0, 1, 1, 3, 0)  # an equal-set neighbour (1, 1) and a set that comes back (0)
S = len(SETS)
HOP = 3
MAX_PUSH = 37
RESTART = (2, 4)  # the restart test: session 2 goes on under set 4
# the first of 77, 78, ... that passes the certification of tests/test_streams_cpu.py at every
# geometry: 77 gives session 2 of 8 x 64 (two classes) two all-zero logit rows
SEED = 78


# ---- the arithmetic, restated ---------------------------------------------------------------------
def cap(T, max_push):
    """net_streams_ring_samples; 0 for a max_push outside 1 .. 65,536."""
    return (T + max_push + 15) // 16 * 16 if 1 <= max_push <= 65536 else 0


def windows_count(T, L, hop):
    return 0 if hop == 0 or L < T else (L - T) // hop + 1


def push_windows(T, hop, pos, n):
    """net_streams_push_windows; 0 for hop == 0 or pos + n past 2^64 - 1."""
    if hop == 0 or pos + n > 2**64 - 1:
        return 0
    return windows_count(T, pos + n, hop) - windows_count(T, pos, hop)


def plan(T, hop, ns, pos=0):
    """Per push of the list ns from position pos: (position, n, k, W0, the k onsets)."""
    out = []
    for n in ns:
        k, W0 = push_windows(T, hop, pos, n), windows_count(T, pos, hop)
        out.append((pos, n, k, W0, [(W0 + j) * hop for j in range(k)]))
        pos += n
    return out


def answered(onset, origin):
    """A window is answered iff it starts at or after its session's origin."""
    return onset >= origin


# ---- the cases --------------------------------------------------------------------------------------
# every n from 1 to MAX_PUSH but the multiples of 16 is in the cycle, most of them no multiple of 4; two
# pushes of one sample early in it, of which at hop 3 at least one completes no window
_HEAD = (1, 1, 1, MAX_PUSH, 2, 3, 5, 36)
_CYCLE = (37, 35, 1, 1, 33, 31, 29, 26, 37, 23, 22, 19, 37, 18, 15, 13, 37, 11, 10, 7, 37, 6, 34, 30, 27, 25, 21, 17, 14,
          9, 4, 8, 12, 20, 24, 28, 2)


@functools.lru_cache(maxsize=None)
def schedule(T, max_push=MAX_PUSH):
    """The fixed list of n of a geometry: the head, then the cycle until the ring has wrapped twice,
    two pushes have crossed its seam while writing, the pushes have started at thirteen residues mod
    16 and one that came after the first window returned none."""
    c = cap(T, max_push)
    ns, pos, crossed, i, res, late0 = [], 0, 0, 0, set(), False
    while True:
        n = _HEAD[i] if i < len(_HEAD) else _CYCLE[(i - len(_HEAD)) % len(_CYCLE)]
        n = min(n, max_push)
        ns.append(n)
        crossed += pos % c + n > c
        res.add(pos % 16)
        late0 = late0 or (pos >= T and push_windows(T, HOP, pos, n) == 0)
        pos += n
        i += 1
        if i >= len(_HEAD) and pos >= 2 * c + 16 and crossed >= 2 and len(res) >= 13 and late0:
            return tuple(ns)


def total(T):
    return sum(schedule(T))


@functools.lru_cache(maxsize=None)
def chunks(C, T, seed=SEED):
    """[S][C][total]: every session's samples, the pushes' chunks end to end, read-only."""
    x = np.random.default_rng([C, T, seed]).integers(-127, 128, size=(S, C, total(T)), dtype=np.int8)
    x.setflags(write=False)
    return x


def rows_of(ps, x_ct, T, hop=HOP):
    """[W][N]: the oracle's logits of the sliding windows of one session's samples [C][L] under ps."""
    return want(ps, sliding_windows(np.ascontiguousarray(x_ct), T, hop))


def pairs():
    """The (session, set) pairs the tests read: each session under its own set, under the set of
    each neighbour that has another, and session RESTART[0] under the set it restarts to."""
    out = {(i, SETS[i]) for i in range(S)}
    out |= {(i, SETS[j]) for i in range(S) for j in (i - 1, i + 1) if 0 <= j < S and SETS[j] != SETS[i]}
    out.add(RESTART)
    return sorted(out)


@functools.lru_cache(maxsize=None)
def table(C, T, N, seed=SEED):
    """{(session, set): [W][N]} for pairs().  Computed once, read-only."""
    x, sets = chunks(C, T, seed), sb.sets(C, T, N)
    out = {}
    for i, s in pairs():
        out[(i, s)] = rows_of(sets[s], x[i], T)
        out[(i, s)].setflags(write=False)
    return out


def expected(tab):
    """[S][W][N]: every session under its own set."""
    return np.stack([tab[(i, SETS[i])] for i in range(S)])
