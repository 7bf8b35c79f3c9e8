"""What the each-group test modules share (tests/test_streams_each_cpu.py,
tests/test_gpu_streams_each.py): a restatement of the per-session plan of a push (csrc/stream_host.hpp,
plan_each) in Python's unbounded integers, and one seeded count schedule per geometry for the five
sessions, sets, hop and max_push of support_streams.  Session i consumes a prefix of
support_streams.chunks(C, T)[i] at its own pace, so its expected rows are the first
windows_count(T, fed_i, HOP) rows of support_streams.expected(table)[i]: the reference stays the C
oracle on materialised windows.

The roles.  Session FULL gets n_max samples in every tick (n_max changes from tick to tick), sessions
1 .. 3 fall behind it by deficits of their own (a session never catches up with FULL: nobody gets more
than n_max), session SLOW stays below one lap of its ring: it runs to its first windows, gets nothing
for some ticks, then trickles.  The data end at support_streams.total(T), which at T = 4096 is 20
samples past two laps of the ring, so there the three ragged sessions may lose 20 samples in all
and are ragged mostly through n_max; the smaller geometries leave them a lap."""
import functools

import numpy as np

import support_streams as ss

S, HOP, MAX_PUSH = ss.S, ss.HOP, ss.MAX_PUSH
FULL, SLOW = 0, 4
I63 = 2**63 - 1
POS_LIMIT = I63 - 65536
# the first of 1, 2, ... whose schedules pass tests/test_streams_each_cpu.py at every geometry
SEED = 294


# ---- the arithmetic, restated ---------------------------------------------------------------------
def each_rows(hop, n_max):
    """net_streams_each_rows: ceil(n_max / hop); 0 for hop == 0 or n_max outside 1 .. 65,536."""
    return -(-n_max // hop) if hop >= 1 and 1 <= n_max <= 65536 else 0


def plan_each(T, hop, cap, pos, cnt, n_max):
    """(ok, n, p0, k, at0, W0) of a session at position pos that is handed cnt of at most n_max
    samples; cnt as the int32 the caller wrote."""
    ok = 0 <= cnt <= n_max and pos + cnt <= POS_LIMIT
    n = cnt if ok else 0
    W0 = ss.windows_count(T, pos, hop)
    k = ss.windows_count(T, pos + n, hop) - W0
    return ok, n, pos % cap, k, (W0 * hop) % cap if k else 0, W0


class Walk:
    """The plan of every tick of a schedule: arrays [ticks][S] of the position before the tick, the
    count, k, W0, p0, at0 and ok, and fed [S], the totals.  start: the sessions' positions before the
    first tick (0); refusals: a refused count (one that would pass POS_LIMIT) is recorded in ok and
    moves nothing, where otherwise it is an error of the schedule.  The plan itself is made in
    Python's integers; every value stored fits an int64."""

    def __init__(self, T, hop, max_push, n_max, counts, start=None, refusals=False):
        cap = ss.cap(T, max_push)
        counts = np.asarray(counts, np.int64)
        ticks = len(n_max)
        self.cap, self.n_max, self.counts = cap, tuple(int(v) for v in n_max), counts
        self.pos, self.k, self.W0, self.p0, self.at0 = (np.zeros((ticks, counts.shape[1]), np.int64) for _ in range(5))
        self.ok = np.ones((ticks, counts.shape[1]), bool)
        pos = [0] * counts.shape[1] if start is None else [int(p) for p in start]
        first = list(pos)
        for t in range(ticks):
            for s in range(counts.shape[1]):
                ok, n, p0, k, at0, W0 = plan_each(T, hop, cap, pos[s], int(counts[t, s]), self.n_max[t])
                assert ok or refusals, (t, s)
                self.ok[t, s] = ok
                self.pos[t, s], self.k[t, s], self.W0[t, s], self.p0[t, s], self.at0[t, s] = pos[s], k, W0, p0, at0
                pos[s] += n
        self.fed = np.array([p - a for p, a in zip(pos, first)], np.int64)


# ---- the schedule -----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def schedule(T, seed=SEED):
    """(n_max [ticks], counts [ticks][S]) of a geometry.  FULL's counts are the n_max, which add up to
    support_streams.total(T)."""
    rng = np.random.default_rng([T, seed])
    cap, total = ss.cap(T, MAX_PUSH), ss.total(T)
    slack = total - 2 * cap - 8           # what a ragged session may fall behind FULL and still wrap twice
    budget = {1: slack // 3, 2: 2 * slack // 3, 3: slack}
    slow_end = T + 30                     # < cap = 16 ceil((T + 37) / 16)
    n_max, counts = [], []
    pos = [0] * S
    zeros_left = 3
    while pos[FULL] < total:
        t = len(n_max)
        if t == 0:
            m = 4                          # the ragged sessions start 1, 2 and 3 behind, SLOW 4
        else:
            m = MAX_PUSH if rng.random() < 0.4 else int(rng.integers(1, MAX_PUSH + 1))
        m = min(m, total - pos[FULL])
        draws = {s: (rng.random() < 0.6, rng.random()) for s in (3, 2, 1)}

        def ragged(m):
            row = [0] * S
            row[FULL] = m
            for s in (3, 2, 1):
                lag = pos[FULL] - pos[s]
                d = s if t == 0 else 0 if draws[s][0] else 1 + int(draws[s][1] * m)
                d = min(d, m, budget[s] - lag)
                if s < 3:  # stay strictly ahead of the next one: positions differ
                    nxt = pos[FULL] + m - (pos[s + 1] + row[s + 1])
                    d = min(d, nxt - 1 - lag)
                row[s] = m - max(d, 0)
            return row

        # no push of a fast session ends exactly at the seam: the lap's last push crosses it
        row = ragged(m)
        while m > 1 and any(row[s] and (pos[s] + row[s]) % cap == 0 for s in range(S) if s != SLOW):
            m -= 1
            row = ragged(m)
        # SLOW: to its first windows, then nothing for three ticks, then a trickle up to slow_end
        if pos[SLOW] < T + 4:
            c = min(m, T + 4 - pos[SLOW]) if t else 0
        elif zeros_left:
            c, zeros_left = 0, zeros_left - 1
        else:
            c = min(int(rng.choice([0, 1, 2, 3, 5, 7])), m, slow_end - pos[SLOW])
        others = {pos[s] + row[s] for s in range(S) if s != SLOW}
        while c > 0 and pos[SLOW] + c in others:
            c -= 1
        row[SLOW] = c
        n_max.append(m)
        counts.append(row)
        pos = [p + c for p, c in zip(pos, row)]
    counts = np.array(counts, np.int32)
    counts.setflags(write=False)
    return tuple(n_max), counts


@functools.lru_cache(maxsize=None)
def walk(T):
    n_max, counts = schedule(T)
    return Walk(T, HOP, MAX_PUSH, n_max, counts)


def expected(tab, fed, T, hop=HOP):
    """[S] arrays [W_i][N]: session i's rows for the fed_i samples it consumed."""
    full = ss.expected(tab)
    return [full[i][: ss.windows_count(T, int(fed[i]), hop)] for i in range(len(fed))]
