"""Each-groups on the GPU (net_streams_push_each[_f32], forward_stream.hpp): the five sessions of
support_streams under sets (0, 1, 1, 3, 0), each fed a prefix of its certified chunks at its own pace
by the count schedule of support_streams_each (certified in tests/test_streams_each_cpu.py: a session
always at n_max, ragged ones, one that never wraps and skips ticks, every count residue mod 16, every
write position mod 4, seam crossings, ticks where one session gets kmax rows and another none).

The reference of every row is the C oracle of the session's set on the materialised window of the
samples the session was given (support_streams.table, computed once per geometry, or
support_streams.rows_of), never another GPU entry, and every comparison is byte-exact.  cnt_out and
win0 are held to the restatement of the plan in support_streams_each."""
import numpy as np
import pytest

import support_bank as sb
import support_streams as ss
import support_streams_each as se
import support_windows_bank as swb
from mibminet import lib
from mibminet.params import ParamSet
from support import CAPS, GUARD, capped, same_each, want  # noqa: F401 (capped: a fixture)
from support_bank import banks  # noqa: F401 (a fixture)

pytestmark = pytest.mark.gpu
JUNK = 0x33       # what the unused part of a slot holds
LEAD = 64         # guard bytes in front of the first tick's rows
INT32_MIN, INT32_MAX = -2**31, 2**31 - 1


def _ceil4(v):
    return (v + 3) // 4 * 4


class Driver:
    """Pushes x ([S][C][L]: a NumPy int8 array, or a float32 device tensor) into the each-group `st`
    through the C entry, session i from its own cursor.  Each tick's slots are staged at a byte offset
    that cycles through 0 .. 3 (float32: 0 and 4), the part of a slot past the session's count filled
    with JUNK (float32: NaN); each tick's rows go to their own 4-byte aligned region [S][kmax][N] of
    one logits buffer prefilled with GUARD (LEAD bytes of it before the first region), its cnt_out and win0 to their own rows of two tables, and
    the counter sits between two others.  `plan`: the n_max of every tick to come, which sizes the
    buffers.  rows() gives each session's rows so far after holding cnt_out and win0 to the
    restatement and every byte that must not be written to GUARD."""

    def __init__(self, torch, st, x, plan, layout="ct", stream=None):
        self.torch, self.st, self.layout, self.stream = torch, st, layout, stream
        self.f32 = not isinstance(x, np.ndarray)
        self.x = x
        self.S, self.C, self.L = (int(v) for v in x.shape)
        self.item = 4 if self.f32 else 1
        d = st.bank.dims
        self.T, self.N = d.T, d.N
        size = sum(_ceil4(self.S * se.each_rows(st.hop, m) * self.N) for m in plan)
        self.y = torch.full((LEAD + size + 128,), GUARD, dtype=torch.int8, device="cuda")
        self.stage = torch.zeros(8 + self.S * self.C * st.max_push * self.item + 64, dtype=torch.uint8, device="cuda")
        self.cin = torch.zeros((len(plan), self.S), dtype=torch.int32, device="cuda")
        self.cout = torch.full((len(plan), self.S), -7, dtype=torch.int32, device="cuda")
        self.win0 = torch.full((len(plan), self.S), -7, dtype=torch.int64, device="cuda")
        self.nb = torch.zeros((3,), dtype=torch.int32, device="cuda")
        self.ticks, self.used = [], LEAD  # guard bytes lie before the first region too
        self.cur, self.pos = [0] * self.S, [0] * self.S  # the data cursors and the group's positions

    def _slots(self, n_max, ns):
        torch = self.torch
        if self.f32:
            slot = torch.full((self.S, self.C, n_max), float("nan"), dtype=torch.float32, device="cuda")
            for s, n in enumerate(ns):
                slot[s, :, :n] = self.x[s, :, self.cur[s]: self.cur[s] + n]
            return slot.view(torch.uint8).reshape(-1)
        slot = np.full((self.S, self.C, n_max), JUNK, np.int8)
        for s, n in enumerate(ns):
            slot[s, :, :n] = self.x[s, :, self.cur[s]: self.cur[s] + n]
        if self.layout == "tc":
            slot = slot.transpose(0, 2, 1)
        return torch.from_numpy(np.ascontiguousarray(slot).reshape(-1).view(np.uint8)).cuda()

    def push(self, n_max, counts, expect=lib.NET_OK):
        """One tick; a count outside 0 .. n_max is passed on as it is and moves nothing."""
        torch, st, t = self.torch, self.st, len(self.ticks)
        ns = [c if 0 <= c <= n_max else 0 for c in counts]
        off = (t % 2) * 4 if self.f32 else t % 4
        s = torch.cuda.current_stream() if self.stream is None else self.stream
        with torch.cuda.stream(s):
            flat = self._slots(n_max, ns)
            self.stage[off: off + flat.numel()].copy_(flat)
            self.cin[t].copy_(torch.tensor(counts, dtype=torch.int32))
        kmax = se.each_rows(st.hop, n_max)
        start = _ceil4(self.used)
        assert start + self.S * kmax * self.N <= self.y.numel() - 64
        A = lib.load()
        args = (self.cin[t].data_ptr(), n_max, self.y.data_ptr() + start, self.cout[t].data_ptr(), self.win0[t].data_ptr(),
                self.nb.data_ptr() + 4, s.cuda_stream)
        if self.f32:
            rc = A.net_streams_push_each_f32(st.handle, self.stage.data_ptr() + off, *args)
        else:
            rc = A.net_streams_push_each(st.handle, self.stage.data_ptr() + off, 1 if self.layout == "ct" else 0, *args)
        assert rc == expect, (rc, t, n_max)
        self.ticks.append((start, kmax, n_max, list(counts), list(self.pos)))
        self.used = start + self.S * kmax * self.N
        self.cur = [a + n for a, n in zip(self.cur, ns)]
        self.pos = [a + n for a, n in zip(self.pos, ns)]

    def run(self, n_max, counts):
        for m, row in zip(n_max, counts):
            self.push(int(m), [int(c) for c in row])
        return self

    def restarted(self, i):
        self.pos[i] = 0

    def rows(self):
        """([S] arrays [rows so far][N], the three counters)."""
        self.torch.cuda.synchronize()
        y, cout, win0 = self.y.cpu().numpy(), self.cout.cpu().numpy(), self.win0.cpu().numpy()
        mask = np.ones(y.shape, bool)
        parts = [[] for _ in range(self.S)]
        cap = self.st.cap
        for t, (start, kmax, n_max, counts, pos) in enumerate(self.ticks):
            for s in range(self.S):
                ok, n, p0, k, at0, W0 = se.plan_each(self.T, self.st.hop, cap, pos[s], counts[s], n_max)
                assert cout[t, s] == (k if ok else -1), (t, s, cout[t].tolist())
                assert win0[t, s] == W0, (t, s, win0[t].tolist())
                a = start + s * kmax * self.N
                mask[a: a + k * self.N] = False
                parts[s].append(y[a: a + k * self.N].reshape(k, self.N))
        assert (cout[len(self.ticks):] == -7).all() and (win0[len(self.ticks):] == -7).all()
        assert (y[mask] == GUARD).all(), "bytes outside the completed rows were written"
        return [np.concatenate(p, axis=0) if p else np.zeros((0, self.N), np.int8) for p in parts], self.nb.cpu().tolist()

    def positions(self):
        return self.st.positions().cpu().tolist()


# ---- 1. every row of every push -------------------------------------------------------------------
@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("layout", ["ct", "tc"])
@pytest.mark.parametrize("C,T,N", ss.GEOMETRIES)
def test_every_row_of_every_push(C, T, N, layout, cap, banks, capped):
    import torch

    n_max, counts = se.schedule(T)
    w = se.walk(T)
    expect = se.expected(ss.table(C, T, N), w.fed, T)
    capped(cap)
    with lib.StreamsEach(banks(C, T, N), ss.SETS, ss.HOP, ss.MAX_PUSH) as st:
        assert st.cap == w.cap and st.info() == [ss.S, ss.HOP, ss.MAX_PUSH, st.cap, 0, -1]
        assert [st.origin(i) for i in range(ss.S)] == [(-1, s) for s in ss.SETS]
        d = Driver(torch, st, ss.chunks(C, T), n_max, layout).run(n_max, counts)
        rows, nb = d.rows()
        assert nb == [0, 0, 0]
        assert d.positions() == w.fed.tolist() == d.pos and st.info()[4:] == [len(n_max), -1]
        same_each(rows, expect)
    assert banks(C, T, N).device_copies() == 1


# ---- 2. the ring itself ---------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["ct", "tc"])
@pytest.mark.parametrize("C,T,N", ss.GEOMETRIES)
def test_ring_holds_layer1_of_each_sessions_last_samples(C, T, N, layout, banks, capped):
    """After a tick that leaves session i at position p its ring holds, at t mod cap and again at
    t mod cap + cap, the oracle's layer-1 output of sample t under its set for its last min(p, cap)
    samples, and zeros where nothing was written yet."""
    import torch

    x, sets = ss.chunks(C, T), sb.sets(C, T, N)
    n_max, counts = se.schedule(T)
    w = se.walk(T)
    y1 = [swb.layer1_of(sets[ss.SETS[i]], x[i]) for i in range(ss.S)]
    c, ticks = w.cap, len(n_max)
    # the first ticks, every tick in which some session crosses the seam and the one after it, every
    # 29th tick, and the last
    look = {0, 1, 2, 3, 4, 5, ticks - 1} | set(range(6, ticks, 29))
    for t in np.flatnonzero((w.p0 + w.counts >= c).any(axis=1)):
        look |= {int(t), min(int(t) + 1, ticks - 1)}
    capped(3)
    with lib.StreamsEach(banks(C, T, N), ss.SETS, ss.HOP, ss.MAX_PUSH) as st:
        d = Driver(torch, st, x, n_max, layout)
        for t in range(ticks):
            d.push(n_max[t], [int(v) for v in counts[t]])
            if t not in look:
                continue
            for i in range(ss.S):
                p = d.pos[i]
                at = np.arange(max(0, p - c), p)
                ring = lib.streams_ring(st, i)
                assert ring.shape == (16, 2 * c)
                np.testing.assert_array_equal(ring[:, :c], ring[:, c:], err_msg=f"the two copies, tick {t}, session {i}")
                np.testing.assert_array_equal(ring[:, at % c], y1[i][:, at], err_msg=f"tick {t} to {p}, session {i}")
                if p < c:
                    assert not ring[:, p:c].any(), f"tick {t}: positions never written"
        assert len(look) >= 12


# ---- 3. float input -------------------------------------------------------------------------------
_SCALES = [0.5, 1.3, 3.0, 7.25, 100.0]


@pytest.mark.parametrize("C,T,N", [(19, 480, 3), (64, 480, 2)])
def test_float_input_with_the_sets_scales(C, T, N, capped):
    """tests/test_gpu_streams.py's float construction: every session's samples as floats that its
    set's scale quantises to the int8 chunks, non-finite samples planted at the start, at the end and
    inside.  The reference is the oracle on the two-pass quantisation of each session with its set's
    scale, cut to what the session was given."""
    import torch

    sets, x = sb.sets(C, T, N), ss.chunks(C, T)
    n_max, counts = se.schedule(T)
    fed = se.walk(T).fed
    L = x.shape[2]
    v = np.arange(-127, 128)
    xf = np.zeros(x.shape, np.float32)
    for i, s in enumerate(ss.SETS):
        lut = ((v + 0.5 * np.sign(v)) * (_SCALES[s] / 127.0)).astype(np.float32)
        xf[i] = lut[x[i].astype(np.int16) + 127]
    xd = torch.from_numpy(xf).cuda()
    xd[:, 0, :7] = torch.tensor([float("nan"), float("inf"), -float("inf"), 3.0, -3.0, 0.0, -0.0], device="cuda")
    xd[:, C - 1, L - 3:] = torch.tensor([float("nan"), -float("inf"), float("inf")], device="cuda")
    mid = T + 101
    xd[1, C // 2, mid: mid + 3] = torch.tensor([float("inf"), float("nan"), -1e30], device="cuda")
    expect = []
    for i, s in enumerate(ss.SETS):
        q = lib.quantize_input_torch(xd[i: i + 1].contiguous(), _SCALES[s])
        q = np.ascontiguousarray(q.cpu().numpy()[0, : L * C].reshape(L, C).T)
        expect.append(ss.rows_of(sets[s], q, T)[: ss.windows_count(T, int(fed[i]), ss.HOP)])
    with lib.Bank(sets, _SCALES) as bank, lib.Bank(sets) as bare:
        for cap in (1, 0):
            capped(cap)
            with lib.StreamsEach(bank, ss.SETS, ss.HOP, ss.MAX_PUSH) as st:
                d = Driver(torch, st, xd, n_max).run(n_max, counts)
                rows, nb = d.rows()
                assert nb == [0, 0, 0] and d.positions() == fed.tolist()
                same_each(rows, expect, f"cap {cap}")
        cnt = torch.full((ss.S,), 5, dtype=torch.int32, device="cuda")
        with lib.StreamsEach(bank, ss.SETS, ss.HOP, ss.MAX_PUSH) as st:  # the Python entry
            y, cout, nbad = st.push_f32(xd[:, :, :5].contiguous(), cnt)
            assert tuple(y.shape) == (ss.S, 2, N) and cout.tolist() == [0] * ss.S and int(nbad.item()) == 0
        with lib.StreamsEach(bare, ss.SETS, ss.HOP, ss.MAX_PUSH) as st:  # no scales
            with pytest.raises(ValueError):
                st.push_f32(xd[:, :, :5].contiguous(), cnt)
            y = torch.zeros(64, dtype=torch.int8, device="cuda")
            assert lib.load().net_streams_push_each_f32(st.handle, xd.data_ptr(), cnt.data_ptr(), 5, y.data_ptr(),
                                                        cnt.data_ptr(), None, None, None) == lib.NET_ERR_INVALID
            assert st.positions().tolist() == [0] * ss.S and st.info()[4] == 0


# ---- 4. counts that are refused -------------------------------------------------------------------
@pytest.mark.parametrize("C,T,N", [(8, 64, 2), (19, 480, 3)])
def test_refused_counts_move_nothing(C, T, N, banks, capped):
    """In chosen ticks one session's count is -1, n_max + 1, INT32_MIN or INT32_MAX: that session gets
    cnt_out = -1 (Driver.rows holds every cnt_out to the restatement), writes nothing and stays where
    it is, n_bad rises by one each time, and its later rows go on as if the tick had not happened;
    the others are what they would have been."""
    import torch

    n_max, counts = se.schedule(T)
    counts = np.array(counts, np.int64)
    ticks = len(n_max)
    bad = {}
    for j, (t, s) in enumerate(((2, 0), (5, 3), (ticks // 3, 1), (ticks // 2, 4), (ticks // 2 + 1, 4), (ticks - 4, 2),
                                (ticks - 1, 0), (ticks - 1, 3))):
        bad[(t, s)] = (-1, n_max[t] + 1, INT32_MIN, INT32_MAX)[j % 4]
    fed = counts.sum(axis=0)
    for (t, s), v in bad.items():
        fed[s] -= counts[t, s]
        counts[t, s] = v
    assert all(fed[s] >= 2 * ss.cap(T, ss.MAX_PUSH) - 2 * ss.MAX_PUSH for s in (0, 1, 2, 3))
    expect = se.expected(ss.table(C, T, N), fed, T)
    for cap in (1, 0):
        capped(cap)
        with lib.StreamsEach(banks(C, T, N), ss.SETS, ss.HOP, ss.MAX_PUSH) as st:
            d = Driver(torch, st, ss.chunks(C, T), n_max, "tc" if cap else "ct").run(n_max, counts)
            rows, nb = d.rows()
            assert nb == [0, len(bad), 0]
            assert d.positions() == fed.tolist()
            same_each(rows, expect, f"cap {cap}")


# ---- 5. equal counts equal the uniform group ------------------------------------------------------
@pytest.mark.parametrize("C,T,N", ss.GEOMETRIES)
def test_equal_counts_give_the_uniform_groups_rows(C, T, N, banks, gpu):
    """Every count n and n_max = n over support_streams.schedule(T): the rows are the oracle table's,
    which is what tests/test_gpu_streams.py expects of the uniform group."""
    import torch

    ns = ss.schedule(T)
    with lib.StreamsEach(banks(C, T, N), ss.SETS, ss.HOP, ss.MAX_PUSH) as st:
        d = Driver(torch, st, ss.chunks(C, T), ns, "ct" if C % 2 else "tc").run(ns, [[n] * ss.S for n in ns])
        rows, nb = d.rows()
        assert nb == [0, 0, 0] and d.positions() == [ss.total(T)] * ss.S
        same_each(rows, list(ss.expected(ss.table(C, T, N))))
        assert [t[1] for t in d.ticks] == [se.each_rows(ss.HOP, n) for n in ns]


# ---- 6. hops --------------------------------------------------------------------------------------
@pytest.mark.parametrize("hop", [1, 50, 70])
def test_hops(hop, banks, capped):
    """hop = 1 (kmax = n_max: a session gets as many rows as samples once T are in), hop > max_push
    (kmax = 1 and most ticks return nothing) and hop > T (samples no window reads)."""
    import torch

    C, T, N = 8, 64, 2
    ns = (37, 26, 1, 1, 1, 5, 37, 16, 2, 37, 37, 9, 33, 37, 4)
    rng = np.random.default_rng([hop, 5])
    counts = np.stack([rng.integers(0, n + 1, size=ss.S) for n in ns])
    counts[:, 0] = ns
    fed = counts.sum(axis=0)
    x = ss.chunks(C, T)[:, :, : sum(ns)]
    sets = sb.sets(C, T, N)
    expect = [ss.rows_of(sets[ss.SETS[i]], x[i], T, hop)[: ss.windows_count(T, int(fed[i]), hop)] for i in range(ss.S)]
    w = se.Walk(T, hop, ss.MAX_PUSH, ns, counts)
    kmax = np.array([se.each_rows(hop, n) for n in ns])
    assert list(kmax) == (list(ns) if hop == 1 else [1] * len(ns))
    assert (hop != 1 or (w.k[3:, 0] == kmax[3:]).all()) and (hop == 1 or (w.k == 0).sum() > w.k.size // 2)
    assert all(len(e) > 0 for e in expect)
    for cap in (1, 0):
        capped(cap)
        with lib.StreamsEach(banks(C, T, N), ss.SETS, hop, ss.MAX_PUSH) as st:
            assert [st.rows(n) for n in ns] == list(kmax)
            d = Driver(torch, st, x, ns, "tc" if cap else "ct").run(ns, counts)
            rows, nb = d.rows()
            assert nb == [0, 0, 0] and d.positions() == fed.tolist()
            same_each(rows, expect, f"hop {hop}, cap {cap}")


# ---- 7. restart -----------------------------------------------------------------------------------
@pytest.mark.parametrize("C,T,N", ss.GEOMETRIES)
def test_restart(C, T, N, banks, capped):
    """Session 2 restarts under set 4 at a position that is no multiple of the hop: its later rows are
    the oracle's under set 4 on the samples it is given after the restart, on a grid that starts at
    0 (no unanswered window), positions() shows 0 and then the new count, and the others are what
    they were."""
    import torch

    i0, new = ss.RESTART
    n_max, counts = se.schedule(T)
    w = se.walk(T)
    sets, x, tab = sb.sets(C, T, N), ss.chunks(C, T), ss.table(C, T, N)
    # the first tick past the middle that session i0 enters at a position that is no multiple of the hop
    at = next(t for t in range(len(n_max) // 2, len(n_max)) if w.pos[t, i0] % ss.HOP and w.pos[t, i0] > T)
    p = int(w.pos[at, i0])
    expect = se.expected(tab, w.fed, T)
    before = tab[(i0, ss.SETS[i0])][: ss.windows_count(T, p, ss.HOP)]
    after = ss.rows_of(sets[new], x[i0][:, p: int(w.fed[i0])], T)
    expect[i0] = np.concatenate([before, after])
    assert len(before) > 0 and len(after) > 5 and p % ss.HOP
    for cap in (1, 0):
        capped(cap)
        with lib.StreamsEach(banks(C, T, N), ss.SETS, ss.HOP, ss.MAX_PUSH) as st:
            d = Driver(torch, st, x, n_max).run(n_max[:at], counts[:at])
            assert d.positions() == w.pos[at].tolist() and st.origin(i0) == (-1, ss.SETS[i0])
            st.restart(i0, new)
            d.restarted(i0)
            assert st.origin(i0) == (-1, new) and st.info()[4] == at
            assert d.positions() == [0 if i == i0 else int(v) for i, v in enumerate(w.pos[at])]
            d.run(n_max[at:], counts[at:])
            rows, nb = d.rows()
            assert nb == [0, 0, 0], cap
            assert d.positions() == [int(v) - (p if i == i0 else 0) for i, v in enumerate(w.fed)]
            same_each(rows, expect, f"cap {cap}")
            L = lib.load()
            for i, s in ((ss.S, 0), (2**40, 0), (0, -1), (0, 5), (0, 2**31 - 1)):
                assert L.net_streams_restart(st.handle, i, s, None) == lib.NET_ERR_INVALID
            assert st.origin(0) == (-1, 0) and d.positions()[0] == int(w.fed[0])


# ---- 8. a captured graph --------------------------------------------------------------------------
@pytest.mark.parametrize("C,T,N", [(8, 64, 2), (22, 1125, 4)])
def test_push_replayed_from_a_captured_graph(C, T, N, banks, gpu):
    """One eager push, then one push captured on a side stream and replayed for the rest of the
    schedule, x and cnt_in rewritten in place before each replay: the rows are the oracle's over all
    ticks and the positions the totals.  A uniform group's push on the capturing stream is still
    refused, and captures nothing."""
    import torch

    n_max, counts = se.schedule(T)
    w = se.walk(T)
    x = ss.chunks(C, T)
    expect = se.expected(ss.table(C, T, N), w.fed, T)
    M, hop = ss.MAX_PUSH, ss.HOP  # the graph's n_max: every count of the schedule is at most that
    kmax = se.each_rows(hop, M)
    A = lib.load()
    with lib.StreamsEach(banks(C, T, N), ss.SETS, hop, M) as st, lib.Streams(banks(C, T, N), ss.SETS, hop, M) as uni:
        xs = torch.zeros((ss.S, C, M), dtype=torch.int8, device="cuda")
        cin = torch.zeros((ss.S,), dtype=torch.int32, device="cuda")
        ybuf = torch.full((LEAD + ss.S * kmax * N + LEAD,), GUARD, dtype=torch.int8, device="cuda")
        y = ybuf[LEAD: LEAD + ss.S * kmax * N].view(ss.S, kmax, N)
        cout = torch.zeros((ss.S,), dtype=torch.int32, device="cuda")
        win0 = torch.zeros((ss.S,), dtype=torch.int64, device="cuda")
        nb = torch.zeros((3,), dtype=torch.int32, device="cuda")
        s = torch.cuda.Stream()
        args = (st.handle, xs.data_ptr(), 1, cin.data_ptr(), M, y.data_ptr(), cout.data_ptr(), win0.data_ptr(),
                nb.data_ptr() + 4)
        cur, got = [0] * ss.S, [[] for _ in range(ss.S)]

        def load(t):
            slot = np.full((ss.S, C, M), JUNK, np.int8)
            for i in range(ss.S):
                slot[i, :, : counts[t, i]] = x[i, :, cur[i]: cur[i] + counts[t, i]]
            xs.copy_(torch.from_numpy(slot))
            cin.copy_(torch.from_numpy(np.array(counts[t])))
            y.fill_(GUARD)

        def collect(t):
            torch.cuda.synchronize()
            yh, ch = y.cpu().numpy(), cout.cpu().tolist()
            assert bool((ybuf[:LEAD] == GUARD).all()) and bool((ybuf[-LEAD:] == GUARD).all()), t
            assert ch == w.k[t].tolist() and win0.cpu().tolist() == w.W0[t].tolist(), t
            for i in range(ss.S):
                got[i].append(yh[i, : ch[i]])
                assert (yh[i, ch[i]:] == GUARD).all(), (t, i)
                cur[i] += int(counts[t, i])

        load(0)
        torch.cuda.synchronize()
        assert A.net_streams_push_each(*args, s.cuda_stream) == lib.NET_OK  # eager
        collect(0)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(s):
            with torch.cuda.graph(g, stream=s):
                assert A.net_streams_push(uni.handle, xs.data_ptr(), 1, 5, y.data_ptr(), nb.data_ptr(), s.cuda_stream) \
                    == lib.NET_ERR_UNSUPPORTED
                assert A.net_streams_push_each(*args, s.cuda_stream) == lib.NET_OK
        torch.cuda.synchronize()
        assert st.positions().tolist() == w.pos[1].tolist()  # the capture ran nothing
        for t in range(1, len(n_max)):
            load(t)
            g.replay()
            collect(t)
        del g
        assert nb.tolist() == [0, 0, 0] and st.positions().tolist() == w.fed.tolist() == cur
        assert st.info()[4] == 2 and uni.info()[4:] == [0, 0]  # enqueues, not replays
        same_each([np.concatenate(p) for p in got], expect)


# ---- 9. the build variants ------------------------------------------------------------------------
@pytest.mark.parametrize("variant", list(sb.VARIANTS))
@pytest.mark.parametrize("C,T,N", sb.VARIANT_GEOMETRIES)
def test_variants(C, T, N, variant, capped):
    import torch

    sets = sb.VARIANTS[variant](C, T, N)
    mp = 1000
    ns = [mp] * ((T - 20) // mp) + [(T - 20) % mp, 37, 1, 30, 16, 5, 37, 23, 2]
    # session 0 always at n_max, the others behind it by their own deficits, the last one at half
    counts = np.array([[n] + [max(n - (t + i) % 3, 0) for i in (1, 2, 3)] + [n // 2] for t, n in enumerate(ns)])
    fed = counts.sum(axis=0)
    x = ss.chunks(C, T)[:, :, : sum(ns)]
    expect = [ss.rows_of(sets[ss.SETS[i]], x[i][:, : fed[i]], T) if fed[i] >= T else np.zeros((0, N), np.int8)
              for i in range(ss.S)]
    assert len(expect[0]) > 40 and len(expect[3]) > 25 and len(set(fed.tolist())) >= 4
    layout, cap = ("tc", 1) if list(sb.VARIANTS).index(variant) % 2 else ("ct", 0)
    with lib.Bank(sets) as bank:
        assert bank.exact_division == (variant in sb.EXACT)
        capped(cap)
        with lib.StreamsEach(bank, ss.SETS, ss.HOP, mp) as st:
            d = Driver(torch, st, x, ns, layout).run(ns, counts)
            rows, nb = d.rows()
            assert nb == [0, 0, 0] and d.positions() == fed.tolist()
            same_each(rows, expect, f"{variant} {layout} cap {cap}")


# ---- 10. isolation and refusals -------------------------------------------------------------------
def test_an_each_group_and_a_uniform_group_on_one_bank(banks, gpu):
    """An each-group and a uniform group on one bank, pushed alternately on one stream of their own:
    each gives its own rows (the uniform group's are the oracle table's).  The bank has one device
    copy, and the loaded set and the image cache are what they were."""
    import torch

    C, T, N = 19, 480, 3
    other = ParamSet.synthetic(seed=7, C=8, T=64, N=2)
    lib.params_load(other)
    trials = sb.epochs(8, 64)[:5]
    loaded = lib.forward_ct_torch(torch.from_numpy(np.array(trials)).cuda()).cpu().numpy()
    before = (lib.device_images(), lib.image_digest(), lib.params_info())
    bank, tab, x = banks(C, T, N), ss.table(C, T, N), ss.chunks(C, T)
    n_max, counts = se.schedule(T)
    w = se.walk(T)
    s = torch.cuda.Stream()
    xd = torch.from_numpy(np.array(x)).cuda()
    A = lib.load()
    with lib.StreamsEach(bank, ss.SETS, ss.HOP, ss.MAX_PUSH) as a, lib.Streams(bank, ss.SETS, ss.HOP, ss.MAX_PUSH) as b:
        da = Driver(torch, a, x, n_max, "ct", stream=s)
        torch.cuda.synchronize()  # the buffers were filled on the default stream
        ys, pos = [], 0
        with torch.cuda.stream(s):
            for t, m in enumerate(n_max):
                da.push(m, [int(v) for v in counts[t]])
                ys.append(b.push(xd[:, :, pos: pos + m].contiguous(), stream=s)[0])  # FULL's pace
                pos += m
        rows_a, nb_a = da.rows()
        assert nb_a == [0, 0, 0]
        same_each(rows_a, se.expected(tab, w.fed, T))
        np.testing.assert_array_equal(torch.cat(ys, dim=1).cpu().numpy(), ss.expected(tab))
        assert bank.device_copies() == 1
        # each kind of group refuses the other's push entry, and nothing moves
        cnt = torch.zeros(ss.S, dtype=torch.int32, device="cuda")
        y = torch.full((4096,), GUARD, dtype=torch.int8, device="cuda")
        nb = torch.zeros(4, dtype=torch.int32, device="cuda")
        INV = lib.NET_ERR_INVALID
        assert A.net_streams_push(a.handle, xd.data_ptr(), 1, 5, y.data_ptr(), nb.data_ptr(), None) == INV
        assert A.net_streams_push_f32(a.handle, xd.data_ptr(), 5, y.data_ptr(), nb.data_ptr(), None) == INV
        assert A.net_streams_push_each(b.handle, xd.data_ptr(), 1, cnt.data_ptr(), 5, y.data_ptr(), cnt.data_ptr(), None,
                                       nb.data_ptr(), None) == INV
        assert A.net_streams_push_each_f32(b.handle, xd.data_ptr(), cnt.data_ptr(), 5, y.data_ptr(), cnt.data_ptr(), None,
                                           nb.data_ptr(), None) == INV
        assert A.net_streams_positions(b.handle, y.data_ptr(), None) == INV
        assert not hasattr(a, "windows")  # an each-group's rows per push are per session
        torch.cuda.synchronize()
        assert a.positions().tolist() == w.fed.tolist() and b.info()[4] == ss.total(T) and a.info()[4] == len(n_max)
        assert bool((y == GUARD).all()) and nb.tolist() == [0, 0, 0, 0] and cnt.tolist() == [0] * ss.S
    assert (lib.device_images(), lib.image_digest(), lib.params_info()) == before
    again = lib.forward_ct_torch(torch.from_numpy(np.array(trials)).cuda()).cpu().numpy()
    np.testing.assert_array_equal(again, loaded)
    np.testing.assert_array_equal(loaded, want(other, trials))
    lib.params_unload()


def test_refused_pushes_leave_the_group_as_it_was(banks, gpu):
    """Every argument check of include/mibminet.h returns its code and leaves the positions, y and the
    counters as they were; the next valid pushes still give the right rows."""
    import torch

    C, T, N = 8, 64, 2
    n_max, counts = se.schedule(T)
    w = se.walk(T)
    expect = se.expected(ss.table(C, T, N), w.fed, T)
    A = lib.load()
    INV = lib.NET_ERR_INVALID
    with lib.StreamsEach(banks(C, T, N), ss.SETS, ss.HOP, ss.MAX_PUSH) as st:
        d = Driver(torch, st, ss.chunks(C, T), n_max)
        half = len(n_max) // 2
        d.run(n_max[:half], counts[:half])
        info, pos = st.info(), d.positions()
        xs = torch.zeros(4096, dtype=torch.int8, device="cuda")
        y = torch.full((4096,), GUARD, dtype=torch.int8, device="cuda")
        cin = torch.full((8,), 5, dtype=torch.int32, device="cuda")
        cout = torch.full((8,), -7, dtype=torch.int32, device="cuda")
        w0 = torch.full((8,), -7, dtype=torch.int64, device="cuda")
        nb = torch.zeros(4, dtype=torch.int32, device="cuda")
        h, x, ci, yp, co, wp, bp = (st.handle, xs.data_ptr(), cin.data_ptr(), y.data_ptr(), cout.data_ptr(), w0.data_ptr(),
                                    nb.data_ptr())
        push, f32 = A.net_streams_push_each, A.net_streams_push_each_f32
        assert push(None, x, 1, ci, 5, yp, co, wp, bp, None) == INV
        for n in (0, ss.MAX_PUSH + 1, 2**40):
            assert push(h, x, 1, ci, n, yp, co, wp, bp, None) == INV
        for layout in (2, -1, 7):
            assert push(h, x, layout, ci, 5, yp, co, wp, bp, None) == INV
        assert push(h, None, 1, ci, 5, yp, co, wp, bp, None) == INV
        assert push(h, x, 1, None, 5, yp, co, wp, bp, None) == INV
        assert push(h, x, 1, ci, 5, None, co, wp, bp, None) == INV
        assert push(h, x, 1, ci, 5, yp, None, wp, bp, None) == INV
        for off in (1, 2, 3):
            assert push(h, x, 1, ci + off, 5, yp, co, wp, bp, None) == INV
            assert push(h, x, 1, ci, 5, yp + off, co, wp, bp, None) == INV
            assert push(h, x, 1, ci, 5, yp, co + off, wp, bp, None) == INV
            assert push(h, x, 1, ci, 5, yp, co, wp + off, bp, None) == INV
            assert push(h, x, 1, ci, 5, yp, co, wp, bp + off, None) == INV
            assert f32(h, x + off, ci, 5, yp, co, wp, bp, None) == INV
        assert push(h, x, 1, ci, 5, yp, co, wp + 4, bp, None) == INV  # win0 is int64
        assert f32(h, x, ci, 5, yp, co, wp, bp, None) == INV            # a bank without scales
        assert A.net_streams_positions(None, wp, None) == INV
        assert A.net_streams_positions(h, None, None) == INV and A.net_streams_positions(h, wp + 4, None) == INV
        # a restart on a capturing stream is still refused
        g, s = torch.cuda.CUDAGraph(), torch.cuda.Stream()
        t = torch.zeros(8, device="cuda")
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            with torch.cuda.graph(g, stream=s):
                t += 1
                assert A.net_streams_restart(h, 0, 1, s.cuda_stream) == lib.NET_ERR_UNSUPPORTED
        g.replay()
        torch.cuda.synchronize()
        assert t.tolist() == [1.0] * 8
        del g
        assert st.info() == info and d.positions() == pos and st.origin(0) == (-1, ss.SETS[0])
        assert bool((y == GUARD).all()) and nb.tolist() == [0, 0, 0, 0]
        assert cout.tolist() == [-7] * 8 and w0.tolist() == [-7] * 8
        # the Python entry refuses what is no tensor of the group's shape
        good = torch.zeros((ss.S, C, 4), dtype=torch.int8, device="cuda")
        c5 = torch.zeros((ss.S,), dtype=torch.int32, device="cuda")
        for bad in (None, np.zeros((ss.S, C, 4), np.int8), torch.zeros((ss.S, C, 4), dtype=torch.int8),
                    torch.zeros((ss.S + 1, C, 4), dtype=torch.int8, device="cuda"),
                    torch.zeros((ss.S, C, 4), dtype=torch.float32, device="cuda")):
            with pytest.raises(ValueError):
                st.push(bad, c5)
        for bad in (None, [0] * ss.S, c5.cpu(), c5.to(torch.int64), torch.zeros((ss.S + 1,), dtype=torch.int32, device="cuda")):
            with pytest.raises(ValueError):
                st.push(good, bad)
        with pytest.raises(ValueError):
            st.push(good, c5, layout="tc")
        with pytest.raises(lib.NetError):
            st.push(torch.zeros((ss.S, C, ss.MAX_PUSH + 1), dtype=torch.int8, device="cuda"), c5)
        assert st.info() == info and d.positions() == pos
        # the next valid pushes still give the right rows
        rows, nbad = d.run(n_max[half:], counts[half:]).rows()
        assert nbad == [0, 0, 0] and d.positions() == w.fed.tolist()
        same_each(rows, expect)


def test_python_push_returns_rows_counts_and_counter(banks, gpu):
    """StreamsEach.push on the tensors alone: its own logits tensor [S][kmax][N], cnt_out and a device
    counter; a count past n_max is refused for its session alone."""
    import torch

    C, T, N = 8, 64, 2
    x = ss.chunks(C, T)
    n_max, counts = se.schedule(T)
    w = se.walk(T)
    expect = se.expected(ss.table(C, T, N), w.fed, T)
    with lib.StreamsEach(banks(C, T, N), ss.SETS, ss.HOP, ss.MAX_PUSH) as st:
        got, cur = [[] for _ in range(ss.S)], [0] * ss.S
        for t, m in enumerate(n_max):
            slot = np.full((ss.S, C, m), JUNK, np.int8)
            for i in range(ss.S):
                slot[i, :, : counts[t, i]] = x[i, :, cur[i]: cur[i] + counts[t, i]]
                cur[i] += int(counts[t, i])
            cnt = torch.from_numpy(np.array(counts[t])).cuda()
            if t % 2:
                y, cout, nbad = st.push(torch.from_numpy(slot).cuda(), cnt)
            else:
                y, cout, nbad = st.push(torch.from_numpy(np.ascontiguousarray(slot.transpose(0, 2, 1))).cuda(), cnt, layout="tc")
            assert tuple(y.shape) == (ss.S, st.rows(m), N) and int(nbad.item()) == 0
            assert cout.tolist() == w.k[t].tolist()
            for i in range(ss.S):
                got[i].append(y[i, : int(cout[i])].cpu().numpy())
        same_each([np.concatenate(p) for p in got], expect)
        cnt = torch.tensor([1, 2, 0, 1, 0], dtype=torch.int32, device="cuda")
        y, cout, nbad = st.push(torch.zeros((ss.S, C, 1), dtype=torch.int8, device="cuda"), cnt)
        assert cout.tolist()[1] == -1 and int(nbad.item()) == 1
        assert st.positions().tolist() == [int(v) + c for v, c in zip(w.fed, (1, 0, 0, 1, 0))]
