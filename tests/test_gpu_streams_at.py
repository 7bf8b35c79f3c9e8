"""Windows at given onsets, read from the live layer-1 rings (net_streams_windows_at,
forward_stream.hpp: k_forward_ring_at): the five sessions of support_streams under sets (0, 1, 1, 3, 0),
pushed by its schedule (each-groups: by support_streams_each's counts), and queried at the points and
with the onset lists of support_streams_at.

The reference of every row is the C oracle of the session's set on the materialised window
x[i][:, o : o + T] (support_streams_at.rows_for, each window computed once), never another GPU entry,
and every comparison is byte-exact.  tests/test_streams_at_cpu.py certifies the inputs: no expected
row is all zeros (zeros mark an invalid item), the rows one sample to either side differ for at least
half of the onsets, and a session's rows under a neighbour's set differ on at least 75 %.  MAX_PUSH is
37, so cap - T is small and almost every window wraps the ring's seam."""
import numpy as np
import pytest

import support_bank as sb
import support_streams as ss
import support_streams_at as sa
import support_streams_each as se
from mibminet import lib
from support import CAPS, GUARD, capped, same  # noqa: F401 (capped: a fixture)
from support_bank import banks  # noqa: F401 (a fixture)

pytestmark = pytest.mark.gpu
LEAD = 64         # guard bytes on either side of the logits
INV = lib.NET_ERR_INVALID


def query(st, items, expect=lib.NET_OK):
    """One call of the C entry on the (session, onset) items: the lists on the device, the logits
    between LEAD guard bytes on either side, the counter between two others.  Returns ([W][N], the
    count) after checking that nothing outside the rows and the counter was written."""
    import torch

    W, N = len(items), st.bank.dims.N
    ses = torch.tensor([int(i) for i, _ in items], dtype=torch.int32).cuda()
    ons = torch.tensor([int(o) for _, o in items], dtype=torch.int64).cuda()
    ybuf = torch.full((LEAD + W * N + LEAD,), GUARD, dtype=torch.int8, device="cuda")
    nb = torch.zeros((3,), dtype=torch.int32, device="cuda")
    rc = lib.load().net_streams_windows_at(st.handle, ses.data_ptr(), ons.data_ptr(), W, ybuf.data_ptr() + LEAD,
                                           nb.data_ptr() + 4, torch.cuda.current_stream().cuda_stream)
    assert rc == expect, rc
    torch.cuda.synchronize()
    y, nbl = ybuf.cpu().numpy(), nb.cpu().tolist()
    assert (y[:LEAD] == GUARD).all() and (y[LEAD + W * N:] == GUARD).all(), "bytes outside the rows were written"
    assert nbl[0] == 0 == nbl[2]
    return y[LEAD: LEAD + W * N].reshape(W, N), nbl[1]


class Feed:
    """The chunks of x ([S][C][L]: a NumPy int8 array, or a float32 device tensor) pushed into the
    uniform group `st` by the list ns through Streams.push / push_f32; rows[j] is what push j
    returned."""

    def __init__(self, st, x, ns, layout="ct"):
        import torch

        self.st, self.ns, self.layout, self.done, self.rows = st, ns, layout, 0, []
        self.f32 = not isinstance(x, np.ndarray)
        self.xd = x if self.f32 else torch.from_numpy(np.array(x)).cuda()

    def to(self, j):
        """Pushes up to and including push j; returns the position."""
        while self.done <= j:
            pos, n = self.st.info()[4], self.ns[self.done]
            x = self.xd[:, :, pos: pos + n]
            x = x.contiguous() if self.layout == "ct" else x.transpose(1, 2).contiguous()
            y, nbad = (self.st.push_f32(x, layout=self.layout) if self.f32 else self.st.push(x, layout=self.layout))
            self.rows.append((y, nbad))
            self.done += 1
        return self.st.info()[4]


# ---- 1. every kind of valid onset -----------------------------------------------------------------
@pytest.mark.parametrize("layout", ["ct", "tc"])
@pytest.mark.parametrize("C,T,N", ss.GEOMETRIES)
def test_every_kind_of_valid_onset(C, T, N, layout, banks, capped):
    """At every query point of the schedule (before the ring is full, right after the pushes that
    crossed the seam while writing, past two laps), under one workgroup, three and the normal grid:
    the newest and the oldest window of every session, onsets at every residue mod 16, windows that
    wrap and that do not, one window asked three times, the items shuffled."""
    with lib.Streams(banks(C, T, N), ss.SETS, ss.HOP, ss.MAX_PUSH) as st:
        f = Feed(st, ss.chunks(C, T), ss.schedule(T), layout)
        for j in sa.points(T):
            pos = f.to(j)
            assert pos == sa.position(T, j) and st.at_span() == sa.span(T, st.cap, pos)
            items = sa.uniform_items(T, pos)
            expect = sa.expected(C, T, N, items)
            for cap in CAPS:
                capped(cap)
                rows, nbad = query(st, items)
                assert nbad == 0, (j, cap)
                same(rows, expect, f"push {j}, cap {cap}")
            capped(0)


# ---- 2. invalid items -----------------------------------------------------------------------------
@pytest.mark.parametrize("C,T,N", [(8, 64, 2), (22, 1125, 4)])
def test_invalid_items_are_zero_rows_and_counted(C, T, N, banks, capped):
    """Session 2 restarts under set 4 after the last push that leaves T + 4 samples to come.  One call
    holds every kind of invalid item, the first and the last item among them, each between two valid
    items of different sets: zero rows, one count each, the valid rows right, the guard bytes
    untouched."""
    ns, cap = ss.schedule(T), ss.cap(T, ss.MAX_PUSH)
    at = max(j for j in range(len(ns)) if ss.total(T) - sa.position(T, j) >= T + 4)
    origin, pos = sa.position(T, at), ss.total(T)
    assert T + 4 <= pos - origin < cap and pos >= 2 * cap
    bad = [(1, o) for o in sa.bad_onsets(T, cap, pos).values()]
    bad += [(2, origin - 1), (2, pos - cap)]               # below the origin, inside the ring
    bad += [(s, pos - T) for s in sa.BAD_SESSIONS.values()]
    assert not sa.valid(pos - cap, origin, pos, T, cap) and sa.valid(pos - cap, 0, pos, T, cap)
    good = [(0, pos - T), (3, pos - cap), (1, pos - T - 5), (2, origin), (4, pos - cap + 7), (2, pos - T), (3, pos - T - 2)]
    new_sets = list(ss.SETS)
    new_sets[2] = 4
    items, is_bad = [], []
    for k, b in enumerate(bad):
        items += [b, good[k % len(good)]]
        is_bad += [True, False]
    items.append(bad[0])
    is_bad.append(True)
    sets_of = [new_sets[i] for (i, _), b in zip(items, is_bad) if not b]
    assert all(a != b for a, b in zip(sets_of, sets_of[1:])) and is_bad[0] and is_bad[-1]
    is_bad = np.array(is_bad)
    expect = np.zeros((len(items), N), np.int8)
    expect[~is_bad] = sa.expected(C, T, N, [it for it, b in zip(items, is_bad) if not b], new_sets)
    with lib.Streams(banks(C, T, N), ss.SETS, ss.HOP, ss.MAX_PUSH) as st:
        f = Feed(st, ss.chunks(C, T), ns)
        assert f.to(at) == origin
        st.restart(2, 4)
        assert f.to(len(ns) - 1) == pos and st.origin(2) == (origin, 4)
        for gc in CAPS:
            capped(gc)
            rows, nbad = query(st, items)
            assert nbad == int(is_bad.sum()) == len(bad) + 1, gc
            same(rows, expect, f"cap {gc}")
            rows, nbad = query(st, bad[:3])  # nothing but invalid items
            assert nbad == 3 and not rows.any()
        capped(0)
        # the Python entry: check=True names the count, check=False returns the rows
        with pytest.raises(ValueError, match="1 of 2"):
            st.windows_at([0, 0], [pos - T, pos - T + 1])
        y = st.windows_at([0, 0], [pos - T, pos - T + 1], check=False).cpu().numpy()
        same(y, np.stack([sa.expected(C, T, N, [(0, pos - T)])[0], np.zeros(N, np.int8)]), "check=False")


# ---- 3. agreement with the grid -------------------------------------------------------------------
@pytest.mark.parametrize("C,T,N", [(8, 64, 2), (22, 1125, 4)])
def test_grid_onsets_give_the_rows_the_pushes_gave(C, T, N, banks, gpu):
    ns = ss.schedule(T)
    plan = ss.plan(T, ss.HOP, ns)
    with lib.Streams(banks(C, T, N), ss.SETS, ss.HOP, ss.MAX_PUSH) as st:
        f = Feed(st, ss.chunks(C, T), ns)
        pos = f.to(len(ns) - 1)
        lo, hi = st.at_span()
        pushed = {}  # (session, onset): the row its push returned
        for (y, _), (_, _, k, _, onsets) in zip(f.rows, plan):
            yh = y.cpu().numpy()
            for i in range(ss.S):
                for j, o in enumerate(onsets):
                    pushed[(i, o)] = yh[i, j]
        items = [(i, o) for i in range(ss.S) for o in range(-(-lo // ss.HOP) * ss.HOP, hi + 1, ss.HOP)]
        assert pos == ss.total(T) and len(items) >= ss.S * ((st.cap - T) // ss.HOP)
        rows = st.windows_at([i for i, _ in items], [o for _, o in items]).cpu().numpy()
        same(rows, np.stack([pushed[it] for it in items]), "against the pushes")
        same(rows, sa.expected(C, T, N, items), "against the oracle")


# ---- 4. no side effect ----------------------------------------------------------------------------
@pytest.mark.parametrize("C,T,N", [(8, 64, 2), (19, 480, 3)])
def test_a_query_changes_nothing(C, T, N, banks, capped):
    """The rings, info() and the origins are what they were before a query (valid and invalid items
    in it), and the rest of the schedule, pushed after it, gives the expected rows."""
    ns = ss.schedule(T)
    expect = ss.expected(ss.table(C, T, N))
    half = sa.crossings(T)[0]
    with lib.Streams(banks(C, T, N), ss.SETS, ss.HOP, ss.MAX_PUSH) as st:
        f = Feed(st, ss.chunks(C, T), ns, "tc")
        pos = f.to(half)
        before = ([lib.streams_ring(st, i) for i in range(ss.S)], st.info(), [st.origin(i) for i in range(ss.S)])
        items = sa.uniform_items(T, pos) + [(1, pos - T + 1), (7, pos - T), (0, -1)]
        for gc in (1, 0):
            capped(gc)
            rows, nbad = query(st, items)
            assert nbad == 3
            same(rows[:-3], sa.expected(C, T, N, items[:-3]), f"cap {gc}")
        capped(0)
        after = ([lib.streams_ring(st, i) for i in range(ss.S)], st.info(), [st.origin(i) for i in range(ss.S)])
        assert before[1:] == after[1:]
        for a, b in zip(before[0], after[0]):
            np.testing.assert_array_equal(a, b)
        f.to(len(ns) - 1)
        rows = np.concatenate([y.cpu().numpy() for y, _ in f.rows], axis=1)
        assert sum(int(nb.item()) for _, nb in f.rows) == 0
        for i in range(ss.S):
            same(rows[i], expect[i], f"session {i} after the query")


# ---- 5. each-groups -------------------------------------------------------------------------------
class FeedEach:
    """support_streams_each's schedule pushed into the each-group `st` through StreamsEach.push, slot
    by slot from every session's own cursor into x [S][C][L]."""

    def __init__(self, st, x, T):
        self.st, self.x = st, x
        self.n_max, self.counts = se.schedule(T)
        self.done, self.cur, self.pos = 0, [0] * ss.S, [0] * ss.S

    def to(self, t):
        import torch

        C = self.x.shape[1]
        while self.done <= t:
            m, row = self.n_max[self.done], self.counts[self.done]
            slot = np.full((ss.S, C, m), 0x33, np.int8)
            for i in range(ss.S):
                slot[i, :, : row[i]] = self.x[i, :, self.cur[i]: self.cur[i] + row[i]]
                self.cur[i] += int(row[i])
                self.pos[i] += int(row[i])
            self.st.push(torch.from_numpy(slot).cuda(), torch.from_numpy(np.array(row)).cuda())
            self.done += 1
        return list(self.pos)


def _each_items(T, pos, base=None, seed=0):
    """(the (session, onset) items in each session's own count, the same as (session, data onset))."""
    items = [(i, o) for i in range(ss.S) for o in sa.onsets_at(T, pos[i])]
    items += [(i, o) for i, o in items if o == pos[i] - T and i in (1, 3)]  # asked twice
    items = sa.shuffled(items, [T, seed, 5])
    return items, [(i, o + (base[i] if base else 0)) for i, o in items]


@pytest.mark.parametrize("C,T,N", ss.GEOMETRIES)
def test_each_groups_in_every_sessions_own_count(C, T, N, banks, capped):
    """The sessions are at different positions; the onsets are each session's own count.  After a
    restart of session 2 under set 4 only onsets of its new count are valid: its old newest window is
    a zero row, and its new windows are set 4's on the samples it was given since."""
    w = se.walk(T)
    ticks, cap = len(w.n_max), w.cap
    x = ss.chunks(C, T)
    i0, new = ss.RESTART
    # session i0 restarts after the last tick that leaves it T + 20 samples to come
    at = max(t for t in range(ticks) if w.fed[i0] - (w.pos[t, i0] + w.counts[t, i0]) >= T + 20)
    # the first tick after which sessions 0 .. 3 all have four windows
    t1 = next(t for t in range(ticks) if all(w.pos[t, i] + w.counts[t, i] >= T + 3 for i in range(4)))
    assert t1 < at
    with lib.StreamsEach(banks(C, T, N), ss.SETS, ss.HOP, ss.MAX_PUSH) as st:
        f = FeedEach(st, x, T)
        for k, t in enumerate((t1, at)):
            pos = f.to(t)
            assert st.positions().tolist() == pos and len(set(pos)) >= 4
            items, data = _each_items(T, pos, seed=k)
            assert len({i for i, _ in items}) >= 4
            expect = sa.expected(C, T, N, data)
            for gc in CAPS:
                capped(gc)
                rows, nbad = query(st, items)
                assert nbad == 0
                same(rows, expect, f"tick {t}, cap {gc}")
            capped(0)
        old = f.pos[i0]
        st.restart(i0, new)
        f.pos[i0] = 0
        pos = f.to(ticks - 1)
        base = [0] * ss.S
        base[i0] = old
        assert pos[i0] == w.fed[i0] - old >= T + 20 and st.positions().tolist() == pos
        items, data = _each_items(T, pos, base, seed=2)
        sets_of = list(ss.SETS)
        sets_of[i0] = new
        # the old count's newest window, and the new count's one before its first
        stale = [(i0, old - T), (i0, pos[i0] - T + 1), (i0, -1)]
        assert not any(sa.valid(o, 0, pos[i0], T, cap) for _, o in stale)
        expect = np.concatenate([sa.expected(C, T, N, data, sets_of), np.zeros((len(stale), N), np.int8)])
        for gc in (1, 0):
            capped(gc)
            rows, nbad = query(st, items + stale)
            assert nbad == len(stale)
            same(rows, expect, f"after the restart, cap {gc}")
        capped(0)
        assert st.positions().tolist() == pos  # a query moves no position


# ---- 6. a captured graph --------------------------------------------------------------------------
@pytest.mark.parametrize("C,T,N", [(8, 64, 2), (22, 1125, 4)])
def test_push_and_query_replayed_from_a_captured_graph(C, T, N, banks, gpu):
    """net_streams_push_each and the query captured once on a side stream and replayed over three
    ticks, the slots, the counts and the device onset array rewritten before each replay: every row
    is the oracle's.  A session with no complete window asks for onset -1 and gets zeros and a count.
    The uniform group refuses the capturing stream."""
    import torch

    n_max, counts = se.schedule(T)
    w = se.walk(T)
    x = ss.chunks(C, T)
    M, hop = ss.MAX_PUSH, ss.HOP
    kmax = se.each_rows(hop, M)
    t0 = next(t for t in range(len(n_max)) if all(w.pos[t, i] >= T + 3 for i in range(4)))
    assert t0 + 3 <= len(n_max)
    A = lib.load()
    with lib.StreamsEach(banks(C, T, N), ss.SETS, hop, M) as st, lib.Streams(banks(C, T, N), ss.SETS, hop, M) as uni:
        xs = torch.zeros((ss.S, C, M), dtype=torch.int8, device="cuda")
        cin = torch.zeros((ss.S,), dtype=torch.int32, device="cuda")
        y = torch.zeros((ss.S, kmax, N), dtype=torch.int8, device="cuda")
        cout = torch.zeros((ss.S,), dtype=torch.int32, device="cuda")
        W = 3 * ss.S
        ses = torch.tensor([i for i in range(ss.S) for _ in range(3)][::-1], dtype=torch.int32).cuda()  # 4 4 4 3 3 3 ...
        ons = torch.full((W,), -1, dtype=torch.int64, device="cuda")
        qbuf = torch.full((LEAD + W * N + LEAD,), GUARD, dtype=torch.int8, device="cuda")
        nb = torch.zeros((3,), dtype=torch.int32, device="cuda")
        s = torch.cuda.Stream()
        push = (st.handle, xs.data_ptr(), 1, cin.data_ptr(), M, y.data_ptr(), cout.data_ptr(), None, None)
        ask = (st.handle, ses.data_ptr(), ons.data_ptr(), W, qbuf.data_ptr() + LEAD, nb.data_ptr() + 4)
        cur = [0] * ss.S

        def load(t):
            slot = np.full((ss.S, C, M), 0x33, np.int8)
            for i in range(ss.S):
                slot[i, :, : counts[t, i]] = x[i, :, cur[i]: cur[i] + counts[t, i]]
                cur[i] += int(counts[t, i])
            xs.copy_(torch.from_numpy(slot))
            cin.copy_(torch.from_numpy(np.array(counts[t])))

        for t in range(t0):  # eager pushes, and one eager query (all its onsets are -1)
            load(t)
            torch.cuda.synchronize()
            assert A.net_streams_push_each(*push, s.cuda_stream) == lib.NET_OK
        assert A.net_streams_windows_at(*ask, s.cuda_stream) == lib.NET_OK
        torch.cuda.synchronize()
        assert nb.tolist() == [0, W, 0] and not qbuf[LEAD: LEAD + W * N].any() and cur == w.pos[t0].tolist()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(s):
            with torch.cuda.graph(g, stream=s):
                assert A.net_streams_windows_at(uni.handle, ses.data_ptr(), ons.data_ptr(), W, qbuf.data_ptr() + LEAD,
                                                nb.data_ptr(), s.cuda_stream) == lib.NET_ERR_UNSUPPORTED
                assert A.net_streams_push_each(*push, s.cuda_stream) == lib.NET_OK
                assert A.net_streams_windows_at(*ask, s.cuda_stream) == lib.NET_OK
        torch.cuda.synchronize()
        assert st.positions().tolist() == w.pos[t0].tolist()  # the capture ran nothing
        for t in range(t0, t0 + 3):
            load(t)
            pos = list(cur)  # after the tick
            asked = []
            for i in ses.tolist()[::3]:
                a, b = sa.span(T, st.cap, pos[i])
                asked += [(i, b), (i, a), (i, min((a + b) // 2 + t % 2, b))] if b >= a else [(i, -1)] * 3
            assert [i for i, _ in asked] == ses.tolist()
            ons.copy_(torch.tensor([o for _, o in asked], dtype=torch.int64))
            nb.zero_()
            qbuf.fill_(GUARD)
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            q = qbuf.cpu().numpy()
            assert (q[:LEAD] == GUARD).all() and (q[LEAD + W * N:] == GUARD).all()
            ok = np.array([o >= 0 for _, o in asked])
            assert nb.tolist() == [0, int((~ok).sum()), 0] and ok.sum() >= 12
            expect = np.zeros((W, N), np.int8)
            expect[ok] = sa.expected(C, T, N, [it for it, k in zip(asked, ok) if k])
            same(q[LEAD: LEAD + W * N].reshape(W, N), expect, f"replay of tick {t}")
            assert st.positions().tolist() == pos
        del g
        assert uni.info()[4:] == [0, 0]


# ---- 7. float groups ------------------------------------------------------------------------------
def test_rings_filled_from_float_frames(capped):
    """The rings filled through push_f32 with layout "tc" (frames as an amplifier delivers them),
    every session's floats quantising to its int8 chunks under its set's scale, then queried."""
    import torch

    C, T, N = 19, 480, 3
    scales = [0.5, 1.3, 3.0, 7.25, 100.0]
    sets, x = sb.sets(C, T, N), ss.chunks(C, T)
    v = np.arange(-127, 128)
    xf = np.zeros(x.shape, np.float32)
    for i, s in enumerate(ss.SETS):
        lut = ((v + 0.5 * np.sign(v)) * (scales[s] / 127.0)).astype(np.float32)
        xf[i] = lut[x[i].astype(np.int16) + 127]
    xd = torch.from_numpy(xf).cuda()
    j = sa.crossings(T)[0]
    q = lib.quantize_input_torch(xd[1:2, :, :64].contiguous(), scales[1]).cpu().numpy()[0, : 64 * C].reshape(64, C).T
    assert np.array_equal(q, x[1][:, :64])  # the construction
    with lib.Bank(sets, scales) as bank, lib.Streams(bank, ss.SETS, ss.HOP, ss.MAX_PUSH) as st:
        pos = Feed(st, xd, ss.schedule(T), "tc").to(j)
        items = sa.uniform_items(T, pos)
        expect = sa.expected(C, T, N, items)
        for gc in (1, 0):
            capped(gc)
            rows, nbad = query(st, items)
            assert nbad == 0
            same(rows, expect, f"cap {gc}")
        capped(0)


# ---- 8. the build variants ------------------------------------------------------------------------
@pytest.mark.parametrize("variant", list(sb.VARIANTS))
@pytest.mark.parametrize("C,T,N", sb.VARIANT_GEOMETRIES)
def test_variants(C, T, N, variant, capped):
    sets = sb.VARIANTS[variant](C, T, N)
    mp = 1000
    ns = [mp] * ((T - 20) // mp) + [(T - 20) % mp, 37, 1, 30, 16, 5, 37, 23, 2]
    x = ss.chunks(C, T)[:, :, : sum(ns)]
    layout, gc = ("tc", 1) if list(sb.VARIANTS).index(variant) % 2 else ("ct", 0)
    with lib.Bank(sets) as bank:
        assert bank.exact_division == (variant in sb.EXACT)
        with lib.Streams(bank, ss.SETS, ss.HOP, mp) as st:
            pos = Feed(st, x, ns, layout).to(len(ns) - 1)
            items = sa.uniform_items(T, pos, cap=st.cap)
            assert pos == sum(ns) and len(items) > 80
            expect = sa.rows_for(C, T, N, [(i, ss.SETS[i], o) for i, o in items], sets=sets, tag=variant)
            capped(gc)
            rows, nbad = query(st, items)
            assert nbad == 0
            same(rows, expect, f"{variant} {layout} cap {gc}")


# ---- 9. refusals and the Python entry -------------------------------------------------------------
def test_refusals_in_the_documented_order(banks, gpu):
    """Each documented code, in the documented order, with nothing enqueued: a guard-filled y and the
    counter are what they were, and so is the group."""
    import torch

    C, T, N = 8, 64, 2
    ns = ss.schedule(T)
    A = lib.load()
    at = A.net_streams_windows_at
    with lib.Streams(banks(C, T, N), ss.SETS, ss.HOP, ss.MAX_PUSH) as st, \
            lib.StreamsEach(banks(C, T, N), ss.SETS, ss.HOP, ss.MAX_PUSH) as each:
        pos = Feed(st, ss.chunks(C, T), ns).to(len(ns) // 2)
        info = st.info()
        ses = torch.zeros(8, dtype=torch.int32, device="cuda")
        ons = torch.full((8,), pos - T, dtype=torch.int64, device="cuda")
        y = torch.full((4096,), GUARD, dtype=torch.int8, device="cuda")
        nb = torch.zeros(4, dtype=torch.int32, device="cuda")
        h, sp, op, yp, bp = st.handle, ses.data_ptr(), ons.data_ptr(), y.data_ptr(), nb.data_ptr()
        assert at(None, sp, op, 5, yp, bp, None) == INV
        assert at(None, None, None, 0, None, None, None) == INV            # the group comes before W == 0
        assert at(h, None, None, 0, None, bp + 1, None) == lib.NET_OK      # W == 0: nothing is looked at
        for W in (2**31 - 65535, 2**31, 2**40, 2**64 - 1):
            assert at(h, sp, op, W, yp, bp, None) == INV
        assert at(h, None, None, 2**40, None, bp + 1, None) == INV
        assert at(h, None, op, 5, yp, bp, None) == INV
        assert at(h, sp, None, 5, yp, bp, None) == INV
        assert at(h, sp, op, 5, None, bp, None) == INV
        for off in (1, 2, 3):
            assert at(h, sp + off, op, 5, yp, bp, None) == INV
            assert at(h, sp, op + off, 5, yp, bp, None) == INV
            assert at(h, sp, op, 5, yp + off, bp, None) == INV
            assert at(h, sp, op, 5, yp, bp + off, None) == INV
        assert at(h, sp, op + 4, 5, yp, bp, None) == INV                   # onsets is int64
        assert at(each.handle, sp, op + 4, 5, yp, bp, None) == INV        # the same checks on an each-group
        # a capturing stream: the uniform group refuses, nothing is captured, the capture ends cleanly
        g, s = torch.cuda.CUDAGraph(), torch.cuda.Stream()
        t = torch.zeros(8, device="cuda")
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            with torch.cuda.graph(g, stream=s):
                t += 1
                assert at(h, sp + 1, op, 5, yp, bp, s.cuda_stream) == INV  # the arguments come first
                assert at(h, sp, op, 5, yp, bp, s.cuda_stream) == lib.NET_ERR_UNSUPPORTED
        g.replay()
        torch.cuda.synchronize()
        assert t.tolist() == [1.0] * 8
        del g
        assert bool((y == GUARD).all()) and nb.tolist() == [0, 0, 0, 0] and st.info() == info
        # net_streams_at_span: host only; an each-group has no host position
        lo = np.full(2, -7, np.int64)
        assert A.net_streams_at_span(h, lo.ctypes.data, lo.ctypes.data + 8) == lib.NET_OK
        assert tuple(lo) == sa.span(T, st.cap, pos) == st.at_span()
        assert A.net_streams_at_span(h, None, lo.ctypes.data) == INV and A.net_streams_at_span(h, lo.ctypes.data, None) == INV
        lo[:] = -7
        assert A.net_streams_at_span(each.handle, lo.ctypes.data, lo.ctypes.data + 8) == INV and tuple(lo) == (-7, -7)
        # an each-group that nothing was pushed into: every onset is invalid, the call itself is fine
        assert at(each.handle, sp, op, 5, yp, bp, None) == lib.NET_OK
        torch.cuda.synchronize()
        assert not y[: 5 * N].any() and bool((y[5 * N:] == GUARD).all()) and nb.tolist() == [5, 0, 0, 0]


def test_python_entry_takes_tensors_and_sequences(banks, gpu):
    import torch

    C, T, N = 8, 64, 2
    ns = ss.schedule(T)
    with lib.Streams(banks(C, T, N), ss.SETS, ss.HOP, ss.MAX_PUSH) as st:
        pos = Feed(st, ss.chunks(C, T), ns).to(sa.points(T)[1])
        items = sa.uniform_items(T, pos)
        expect = sa.expected(C, T, N, items)
        sessions, onsets = [i for i, _ in items], [o for _, o in items]
        y = st.windows_at(sessions, onsets)
        assert tuple(y.shape) == (len(items), N) and y.dtype == torch.int8 and y.is_cuda
        same(y.cpu().numpy(), expect, "sequences")
        sd, od = torch.tensor(sessions, dtype=torch.int32).cuda(), torch.tensor(onsets, dtype=torch.int64).cuda()
        out = torch.zeros((len(items), N), dtype=torch.int8, device="cuda")
        assert st.windows_at(sd, od, out=out, check=False) is out
        same(out.cpu().numpy(), expect, "device tensors")
        assert tuple(st.windows_at([], []).shape) == (0, N)
        for bad in ((sessions[:-1], onsets), (sd.to(torch.int64), od), (sd, od.to(torch.int32)), (sd[None], od[None])):
            with pytest.raises(ValueError):
                st.windows_at(*bad)
        with pytest.raises(ValueError):
            st.windows_at(sd, od, out=torch.zeros((len(items) + 1, N), dtype=torch.int8, device="cuda"))
