"""What the tests of an each-group's decimator share (tests/test_decim_each_cpu.py,
tests/test_decim_each_host_sanitizers.py, tests/test_gpu_streams_each_decim.py): a restatement of the
per-session plan of a raw push (csrc/stream_host.hpp, plan_each_raw) in Python's unbounded integers,
one seeded ragged schedule of raw counts per (T, q, K) for the five sessions, sets, hop and max_push
of support_decim, the raw frames each session consumes and, computed once per case, the reference of
every row and ring byte.  The reference is never another stream entry: decimate.fir_decimate on the
CPU over the session's concatenated chunks, then support_decim.two_pass with its set's scale, then
the C oracle on the materialised sliding windows (support_streams.rows_of)."""
import functools

import numpy as np

import support_bank as sb
import support_decim as sd
import support_streams as ss
import support_streams_each as se
from mibminet import decimate, lib

SETS, S, HOP, MAX_PUSH, SCALES = sd.SETS, sd.S, sd.HOP, sd.MAX_PUSH, sd.SCALES
I63 = 2**63 - 1
RAW_LIMIT = I63 - 2**20
FULL = 0  # the session that gets n_raw_max frames in every tick of the tail
GUARD = 0x5A


# ---- the arithmetic, restated ---------------------------------------------------------------------
def each_raw_rows(hop, q, n_raw_max):
    """net_streams_each_raw_rows."""
    return se.each_rows(hop, -(-n_raw_max // q)) if 1 <= q <= 16 else 0


def plan_each_raw(T, hop, cap, q, K, P, cnt, n_raw_max):
    """(ok, m, n_raw, off, slot0, keep, then plan_each's n, p0, k, at0, W0) of a session at raw position
    P that is handed cnt of at most n_raw_max frames; cnt as the int32 the caller wrote."""
    ok = 0 <= cnt <= n_raw_max and P + cnt <= RAW_LIMIT
    n = cnt if ok else 0
    d0, d1 = decimate.raw_decimated(q, P), decimate.raw_decimated(q, P + n)
    m = d1 - d0
    ok_each, n_dec, p0, k, at0, W0 = se.plan_each(T, hop, cap, d0, m, -(-n_raw_max // q))
    assert ok_each and n_dec == m
    return ok, m, n, q * d0 - P, P % (K - 1) if K > 1 else 0, min(n, K - 1), m, p0, k, at0, W0


class Walk:
    """The plan of every tick of a schedule: arrays [ticks][S] of the raw position before the tick, m,
    off, slot0, k, W0 and ok, and fed [S], the raw totals.  start: the sessions' raw positions before
    the first tick (0)."""

    def __init__(self, T, q, K, n_raw_max, counts, hop=HOP, max_push=MAX_PUSH, start=None):
        cap = ss.cap(T, max_push)
        counts = np.asarray(counts, np.int64)
        ticks, n_s = counts.shape
        self.cap, self.q, self.n_raw_max, self.counts = cap, q, tuple(int(v) for v in n_raw_max), counts
        self.P, self.m, self.off, self.slot0, self.k, self.W0, self.ok = (np.zeros((ticks, n_s), np.int64) for _ in range(7))
        P = [0] * n_s if start is None else [int(p) for p in start]
        first = list(P)
        for t in range(ticks):
            for s in range(n_s):
                ok, m, n, off, slot0, _, _, _, k, _, W0 = plan_each_raw(T, hop, cap, q, K, P[s], int(counts[t, s]),
                                                                        self.n_raw_max[t])
                self.P[t, s], self.m[t, s], self.off[t, s], self.slot0[t, s] = P[s], m, off, slot0
                self.k[t, s], self.W0[t, s], self.ok[t, s] = k, W0, ok
                P[s] += n
        self.fed = np.array([p - a for p, a in zip(P, first)], np.int64)


# ---- the schedule -----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def schedule(T, q, K, max_push=MAX_PUSH):
    """(n_raw_max [ticks], counts [ticks][S]): a head that puts the sessions at different raw positions
    (so at different phases and history slots), hands session 1 three pushes in a row below K - 1 and
    single frames off the grid, and has a tick at q max_push; then a seeded tail in which FULL gets
    n_raw_max frames every tick and the others nothing, fewer than q or the upper half of 0 .. n_raw_max,
    until every session's ring has wrapped twice."""
    top = q * max_push
    head = [(q + 4, [q + 4, 1, 2, q + 1, 3]),
            (3, [3, 1, 0, 1, 2]),
            (max(q - 1, 1), [0, 1, max(q - 1, 1), 0, 1]),
            (2, [2, 2, 1, 0, 0]),
            (top, [top, top - 1, top // 2, 5, top]),
            (1, [1, 1, 1, 1, 0])]
    rng = np.random.default_rng([T, q, K, 17])
    n_max, counts = [h[0] for h in head], [h[1] for h in head]
    P = np.sum(counts, axis=0)
    goal = q * (2 * ss.cap(T, max_push) + 16)
    while P.min() < goal:
        m = top if len(n_max) % 4 == 0 else int(rng.integers(1, top + 1))
        row = [m]
        for _ in range(1, S):
            u = rng.random()
            row.append(0 if u < 0.1 else int(rng.integers(1, max(min(q, m + 1), 2))) if u < 0.2 else
                       int(rng.integers(m // 2, m + 1)))
        row = [min(c, m) for c in row]
        n_max.append(m)
        counts.append(row)
        P = P + row
    counts = np.array(counts, np.int32)
    counts.setflags(write=False)
    return tuple(n_max), counts


@functools.lru_cache(maxsize=None)
def walk(T, q, K):
    n_max, counts = schedule(T, q, K)
    return Walk(T, q, K, n_max, counts)


def certify(T, q, K):
    """What the issue asks of the ragged schedule, asserted."""
    n_max, counts = schedule(T, q, K)
    w = walk(T, q, K)
    assert w.ok.all() and (counts <= np.array(n_max)[:, None]).all()
    assert (counts == 0).any()
    assert ((counts == 1) & (w.m == 0)).any() or q == 1
    assert ((counts > 0) & (counts < q)).any() or q == 1
    assert K <= 2 or any(((counts[t: t + 3, s] < K - 1) & (counts[t: t + 3, s] > 0)).all()
                         for t in range(len(n_max) - 2) for s in range(S))
    assert q * MAX_PUSH in n_max and (counts == q * MAX_PUSH).any()
    live = counts > 0
    assert q == 1 or K <= 2 or any(live[t, a] and live[t, b] and w.off[t, a] != w.off[t, b] and w.slot0[t, a] != w.slot0[t, b]
                                   for t in range(len(n_max)) for a in range(S) for b in range(a))
    assert set(w.off[live].tolist()) == set(range(q))
    assert (-(-w.fed // q) >= 2 * w.cap + 16).all()  # every ring has wrapped twice
    return w


# ---- the frames and the reference -------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def frames(C, T, q, K):
    """[S][L][C] float32: every session's raw frames, L the largest total of the schedule; session i
    consumes the first walk.fed[i] of its own.  Read-only."""
    x = sd.inputs(np.random.default_rng([C, T, q, K, 5]), (S, int(walk(T, q, K).fed.max()), C))
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def reference(C, T, N, q, K):
    """(sets, taps, qd [S] arrays [C][Ld_i], rows [S] arrays [W_i][N]) of frames(C, T, q, K) cut to what
    each session consumes, every session under its own set and scale."""
    sets, h, x, fed = sb.sets(C, T, N), sd.taps(K, 11), frames(C, T, q, K), walk(T, q, K).fed
    both = [sd.session_reference(sets[s], SCALES[s], x[i][: int(fed[i])], h, q, T) for i, s in enumerate(SETS)]
    return sets, h, [b[0] for b in both], [b[1] for b in both]


# ---- the driver of the GPU tests ----------------------------------------------------------------------
class RawDriver:
    """Pushes x ([S][L][C] float32, NumPy) into the each-group `st` through the C entry, session i from
    its own cursor.  Each tick's slots [S][n_raw_max][C] are NaN beyond the session's count; y is
    prefilled with GUARD and every byte outside the completed rows held to it; cnt_out and win0 are
    held to the restatement of the plan, and positions() to D(raw_positions()).  A count outside
    0 .. n_raw_max is passed on as it is and consumes nothing.  start: the sessions' raw positions
    before the first tick (0)."""

    def __init__(self, torch, st, x, q, K, stream=None, start=None):
        self.torch, self.st, self.x, self.q, self.K, self.stream = torch, st, x, q, K, stream
        d = st.bank.dims
        self.S, self.C, self.T, self.N = st.S, int(x.shape[2]), d.T, d.N
        self.cur, self.P = [0] * self.S, [0] * self.S if start is None else [int(p) for p in start]
        self.rows = [[] for _ in range(self.S)]
        self.nb = torch.zeros((3,), dtype=torch.int32, device="cuda")

    def slots(self, n_raw_max, ns):
        slot = np.full((self.S, n_raw_max, self.C), np.nan, np.float32)
        for s, n in enumerate(ns):
            slot[s, :n] = self.x[s, self.cur[s]: self.cur[s] + n]
        return self.torch.from_numpy(slot).cuda()

    def push(self, n_raw_max, counts, expect=lib.NET_OK):
        torch, st = self.torch, self.st
        ns = [c if 0 <= c <= n_raw_max else 0 for c in counts]
        kmax = each_raw_rows(st.hop, self.q, n_raw_max)
        assert kmax == lib.each_raw_rows(st.hop, self.q, n_raw_max)
        xs = self.slots(n_raw_max, ns)
        cin = torch.tensor(counts, dtype=torch.int32, device="cuda")
        y = torch.full((self.S, kmax, self.N), GUARD, dtype=torch.int8, device="cuda")
        cout = torch.full((self.S,), -7, dtype=torch.int32, device="cuda")
        win0 = torch.full((self.S,), -7, dtype=torch.int64, device="cuda")
        s = torch.cuda.current_stream() if self.stream is None else self.stream
        torch.cuda.synchronize()
        rc = lib.load().net_streams_push_each_raw_f32_tm(st.handle, xs.data_ptr(), cin.data_ptr(), n_raw_max, y.data_ptr(),
                                                         cout.data_ptr(), win0.data_ptr(), self.nb.data_ptr() + 4, s.cuda_stream)
        assert rc == expect, (rc, n_raw_max)
        torch.cuda.synchronize()
        yh, ch, wh = y.cpu().numpy(), cout.tolist(), win0.tolist()
        for i in range(self.S):
            ok, m, n, _, _, _, _, _, k, _, W0 = plan_each_raw(self.T, st.hop, st.cap, self.q, self.K, self.P[i], counts[i],
                                                              n_raw_max)
            assert ch[i] == (k if ok else -1) and wh[i] == W0, (i, ch, wh, k, W0)
            assert (yh[i, k:] == GUARD).all(), f"session {i}: rows past its {k} were written"
            self.rows[i].append(yh[i, :k])
            self.cur[i] += n
            self.P[i] += n
        raw = st.raw_positions().tolist()
        assert raw == self.P and st.positions().tolist() == [decimate.raw_decimated(self.q, p) for p in raw]

    def run(self, n_raw_max, counts):
        for m, row in zip(n_raw_max, counts):
            self.push(int(m), [int(c) for c in row])
        return self

    def restarted(self, i):
        self.P[i] = 0

    def result(self):
        """([S] arrays [rows so far][N], the three counters)."""
        return [np.concatenate(p, axis=0) if p else np.zeros((0, self.N), np.int8) for p in self.rows], self.nb.tolist()
