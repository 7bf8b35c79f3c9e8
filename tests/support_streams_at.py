"""What the test modules of net_streams_windows_at share (tests/test_streams_at_cpu.py,
tests/test_gpu_streams_at.py): a restatement in Python's unbounded integers of when a queried window
is in a session's ring and where, the points of support_streams' push schedule at which the groups are
queried, the onset lists asked there, and the C oracle's logits of exactly the windows asked, computed
once and kept.  The sessions, sets, hop, max_push and chunks are support_streams'; the reference of a
row is always the oracle of the session's set on the materialised window x[i][:, o : o + T], never
another GPU entry."""
import functools

import numpy as np

import support_bank as sb
import support_streams as ss
from support import want, windows_at

I64_MIN, I64_MAX = -2**63, 2**63 - 1
I32_MIN, I32_MAX = -2**31, 2**31 - 1
# support_streams.SEED (78) passes the certification of tests/test_streams_at_cpu.py on the onset lists
# below at every geometry, so the chunks are support_streams' own
SEED = ss.SEED


# ---- the arithmetic, restated ---------------------------------------------------------------------
def valid(o, lo, pos, T, cap):
    """A window from sample o of a session at position pos, whose windows may start at lo (its
    origin; 0 for an each-group): complete and its first sample still in the ring."""
    return o >= 0 and o >= lo and T <= pos - o <= cap


def ring_at(o, cap):
    """The ring position of the window's first byte."""
    return o % cap


def span(T, cap, pos):
    """net_streams_at_span: (lo, hi); hi < lo when no window is there yet."""
    return max(pos - cap, 0), pos - T


def wraps(o, T, cap):
    """The window's T bytes cross the ring's seam (and are read from its second copy)."""
    return o % cap + T > cap


# ---- where the groups are queried -----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def points(T):
    """Indices j into support_streams.schedule(T), in order: the group is queried after push j.  The
    first push that takes the position to T + 3 or beyond (the ring is not full yet), the first two pushes that crossed
    the seam while writing (the ring has wrapped by then), and the last (past two laps)."""
    ns, c = ss.schedule(T), ss.cap(T, ss.MAX_PUSH)
    first, crossed, pos = None, [], 0
    for j, n in enumerate(ns):
        if pos % c + n > c:
            crossed.append(j)
        pos += n
        if first is None and pos >= T + 3:  # four onsets at least: every residue mod 4
            first = j
    return tuple(sorted({first, crossed[0], crossed[1], len(ns) - 1}))  # at 8 x 64 the last push is the second crossing


def crossings(T):
    """The first two pushes of the schedule that crossed the seam while writing."""
    ns, c = ss.schedule(T), ss.cap(T, ss.MAX_PUSH)
    pos = np.concatenate([[0], np.cumsum(ns)[:-1]])
    return tuple(int(j) for j in np.flatnonzero(pos % c + np.array(ns) > c)[:2])


def position(T, j):
    """The group's position after push j of the schedule."""
    return sum(ss.schedule(T)[: j + 1])


def onsets_at(T, pos, lo=0, cap=None):
    """The valid onsets asked of a session at position pos whose windows may start at lo: the newest
    (pos - T), the oldest still in the ring, and the first onset of the span at every residue mod 16
    (so at every residue mod 4).  In the span's order, no duplicates; empty when no window is there.
    cap: the ring's size if the group's max_push is not support_streams'."""
    cap = ss.cap(T, ss.MAX_PUSH) if cap is None else cap
    a, b = span(T, cap, pos)
    a = max(a, lo)
    if b < a:
        return []
    out = [b, a] + [o for o in range(a, min(a + 16, b + 1))]
    return sorted(set(out))


def shuffled(items, seed):
    """The items in a seeded order in which neighbours change sets in both directions."""
    items = list(items)
    order = np.random.default_rng(seed).permutation(len(items))
    return [items[k] for k in order]


def uniform_items(T, pos, origins=None, cap=None):
    """The (session, onset) items of one call on the uniform group at position pos: every session
    asked for onsets_at, the newest window of sessions 1 and 4 asked three times in all, shuffled."""
    items = []
    for i in range(ss.S):
        on = onsets_at(T, pos, origins[i] if origins else 0, cap)
        items += [(i, o) for o in on]
        if i in (1, 4) and on:
            items += [(i, on[-1])] * 2
    return shuffled(items, [T, pos])


# ---- the reference --------------------------------------------------------------------------------
_ROWS = {}


def rows_for(C, T, N, items, sets=None, x=None, tag=""):
    """[len(items)][N]: the oracle's logits of the windows x[i][:, o : o + T] under set s for the
    items (i, s, o).  Each window is computed once per process (by `tag` for other sets or samples
    than support_bank's and support_streams')."""
    sets = sb.sets(C, T, N) if sets is None else sets
    x = ss.chunks(C, T) if x is None else x
    todo = {}
    for i, s, o in items:
        if (C, T, N, tag, i, s, o) not in _ROWS:
            todo.setdefault((i, s), set()).add(o)
    for (i, s), on in todo.items():
        on = sorted(on)
        assert 0 <= on[0] and on[-1] + T <= x.shape[2], (i, s, on[0], on[-1])
        got = want(sets[s], windows_at(np.ascontiguousarray(x[i]), on, T))
        for o, r in zip(on, got):
            r.setflags(write=False)
            _ROWS[(C, T, N, tag, i, s, o)] = r
    return np.stack([_ROWS[(C, T, N, tag, i, s, o)] for i, s, o in items]) if items else np.zeros((0, N), np.int8)


def expected(C, T, N, items, sets_of=ss.SETS):
    """rows_for the (session, onset) items, every session under its own set."""
    return rows_for(C, T, N, [(i, sets_of[i], o) for i, o in items])


# ---- invalid items --------------------------------------------------------------------------------
def bad_onsets(T, cap, pos):
    """Onsets that are invalid for a session with origin 0 at position pos >= cap, by name."""
    good = pos - T
    out = {
        "one past the newest": pos - T + 1,
        "one before the oldest": pos - cap - 1,
        "-1": -1,
        "INT64_MIN": I64_MIN,
        "INT64_MAX": I64_MAX,
        "low 32 bits valid, + 2^32": good + 2**32,
        "low 32 bits valid, - 2^32": good - 2**32,
        "low 32 bits valid, sign bit": good - 2**63,
    }
    assert all(not valid(o, 0, pos, T, cap) and I64_MIN <= o <= I64_MAX for o in out.values())
    assert all((out[k] - good) % 2**32 == 0 for k in out if k.startswith("low"))
    return out


BAD_SESSIONS = {"-1": -1, "S": ss.S, "INT32_MIN": I32_MIN, "INT32_MAX": I32_MAX}
