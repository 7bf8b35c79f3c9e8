"""Stream groups far from zero on the GPU: every stream kernel run at positions that cross 2^31 and
2^32, past 2^53 and up to INT64_MAX (each-groups: up to the limits their plans keep), after the hook
mibminet_test_streams_seek (lib.streams_seek) has placed a fresh group there.

The reference of a row is never another stream entry and never built from position 0: a session
seeked to P is the session whose samples before P were zero, its recording begins at global sample P,
and the window with global onset o >= P is the C oracle's on the materialised window at o - P
(tests/support_streams_seek.py, whose cases tests/test_streams_seek_cpu.py certifies: the residues of
every start, the crossings, no all-zero expected row, the prefilter's two conditions).  Every
comparison is byte for byte."""
import ctypes

import numpy as np
import pytest

import support_bank as sb
import support_decim as sd
import support_decim_each as sde
import support_prefilter as pf
import support_streams as ss
import support_streams_each as se
import support_streams_seek as sk
from mibminet import decimate, lib
from support import GUARD, capped, dev, same, same_each, same_rows  # noqa: F401 (capped: a fixture)
from support_bank import banks  # noqa: F401 (a fixture)

pytestmark = pytest.mark.gpu

SETS, S, HOP, MAX_PUSH = sk.SETS, sk.S, sk.HOP, sk.MAX_PUSH
I63, INV, OK = sk.I63, lib.NET_ERR_INVALID, lib.NET_OK
JUNK, LEAD = 0x33, 64
F32_SCALES = [0.5, 1.3, 3.0, 7.25, 100.0]  # tests/test_gpu_streams.py's: the floats below quantise to the chunks


def i64(v):
    return (ctypes.c_int64 * len(v))(*[int(e) for e in v])


def seek_rc(st, pos, origin=None):
    """The hook's return code (lib.streams_seek raises on a refusal)."""
    return lib.load().mibminet_test_streams_seek(st.handle if st is not None else None, None if pos is None else i64(pos),
                                                 None if origin is None else i64(origin))


@pytest.fixture(scope="module")
def scaled_banks(gpu):
    """The five-set banks with F32_SCALES, by geometry."""
    cache = {}

    def get(C, T, N):
        if (C, T, N) not in cache:
            cache[(C, T, N)] = lib.Bank(sb.sets(C, T, N), F32_SCALES)
        return cache[(C, T, N)]

    yield get
    for b in cache.values():
        b.close()


def as_floats(x):
    """support_streams' chunks [S][C][L] as float32 that each session's scale of F32_SCALES quantises
    back to them (the middle of each int8 value's interval)."""
    v = np.arange(-127, 128)
    xf = np.zeros(x.shape, np.float32)
    for i, s in enumerate(SETS):
        lut = ((v + 0.5 * np.sign(v)) * (F32_SCALES[s] / 127.0)).astype(np.float32)
        xf[i] = lut[x[i].astype(np.int16) + 127]
        assert np.array_equal(sd.two_pass(np.ascontiguousarray(xf[i].T), F32_SCALES[s]), x[i])
    return xf


class Feed:
    """The pushes of `plan` (support_streams.plan from the group's position) through Streams.push or
    push_f32, from xd [S][C][L] on the device, the session's samples from its seek position on.  After
    every push: the position, k, n_bad (bad[j]) and the rows (rows[:, first[j] : first[j] + k])."""

    def __init__(self, st, xd, plan, rows, bad, entry="ct"):
        self.st, self.xd, self.plan, self.rows, self.bad, self.entry = st, xd, plan, rows, bad, entry
        self.start, self.done, self.first = plan[0][0], 0, 0

    def to(self, j):
        """Pushes up to and including push j; returns the position."""
        st, N = self.st, self.st.bank.dims.N
        while self.done <= j:
            pos, n, k, _, _ = self.plan[self.done]
            assert st.info()[4] == pos
            x = self.xd[:, :, pos - self.start: pos - self.start + n]
            if self.entry == "ct":
                y, nbad = st.push(x.contiguous())
            elif self.entry == "tc":
                y, nbad = st.push(x.transpose(1, 2).contiguous(), layout="tc")
            else:
                y, nbad = st.push_f32(x.transpose(1, 2).contiguous(), layout="tc")
            assert st.info()[4] == pos + n and tuple(y.shape) == (S, k, N), (self.done, st.info(), tuple(y.shape))
            assert int(nbad.item()) == self.bad[self.done], (self.done, int(nbad.item()), self.bad[self.done])
            same_rows(y.cpu().numpy(), self.rows[:, self.first: self.first + k], f"push {self.done} at {pos}")
            self.first += k
            self.done += 1
        return st.info()[4]


# ---- a. uniform pushes across each base ----------------------------------------------------------------
A_CASES = [(b, sk.GEOMETRY, 0) for b in sk.BASES] + [("2^32", sk.GEOMETRY, 1), ("2^32", sk.WIDE, 0)]


@pytest.mark.parametrize("entry", ["ct", "tc", "f32_tm"])
@pytest.mark.parametrize("base,geometry,cap", A_CASES)
def test_uniform_pushes_across_each_base(base, geometry, cap, entry, banks, scaled_banks, capped):
    import torch

    c = sk.uniform_case(base, geometry)
    C, T, N = geometry
    rows, keep = sk.uniform_rows(base, geometry)
    x = ss.chunks(C, T)
    xd = torch.from_numpy(as_floats(x) if entry == "f32_tm" else np.array(x)).cuda()
    capped(cap)
    with lib.Streams((scaled_banks if entry == "f32_tm" else banks)(C, T, N), SETS, HOP, MAX_PUSH) as st:
        lib.streams_seek(st, [c.P] * S)
        assert st.info() == [S, HOP, MAX_PUSH, c.cap, c.P, 0] and [st.origin(i) for i in range(S)] == [(c.P, s) for s in SETS]
        f = Feed(st, xd, c.plan, rows, [S * b for b in c.below], entry)
        assert f.to(len(c.plan) - 1) == c.P + c.L and st.info()[5] == len(c.onsets)
        sd.check_rings(st, sb.sets(C, T, N), [x[i] for i in range(S)], base=c.P)
        if base == "top":
            assert st.info()[4] == I63 and st.at_span() == (I63 - c.cap, I63 - T)
            info = st.info()
            y = torch.full((S * N + 8,), GUARD, dtype=torch.int8, device="cuda")
            nb = torch.zeros((1,), dtype=torch.int32, device="cuda")
            if entry == "f32_tm":
                rc = lib.load().net_streams_push_f32_tm(st.handle, xd.data_ptr(), 1, y.data_ptr(), nb.data_ptr(), None)
            else:
                rc = lib.load().net_streams_push(st.handle, xd.data_ptr(), 1, 1, y.data_ptr(), nb.data_ptr(), None)
            torch.cuda.synchronize()
            assert rc == INV and st.info() == info and bool((y == GUARD).all()) and int(nb.item()) == 0
            assert st.at_span() == (I63 - c.cap, I63 - T)
            sd.check_rings(st, sb.sets(C, T, N), [x[i] for i in range(S)], base=c.P)


# ---- b. a restart past 2^32 ----------------------------------------------------------------------------------
def test_restart_past_two_to_the_32(banks, capped):
    """The origin of the restarted session is a 64-bit position whose low 32 bits are below those of
    every onset answered before the boundary: an origin kept or compared in 32 bits would answer the
    windows that start before it, or refuse those after it."""
    import torch

    r = sk.restart_case()
    c = r.case
    xd = torch.from_numpy(np.array(ss.chunks(c.C, c.T))).cuda()
    for cap in (1, 0):
        capped(cap)
        with lib.Streams(banks(c.C, c.T, c.N), SETS, HOP, MAX_PUSH) as st:
            lib.streams_seek(st, [c.P] * S)
            f = Feed(st, xd, c.plan, r.rows, r.bad)
            assert f.to(r.at - 1) == r.R > 2**32 > c.P
            assert [st.origin(i) for i in range(S)] == [(c.P, s) for s in SETS]
            st.restart(r.i0, r.new)
            sets_now = [r.new if i == r.i0 else s for i, s in enumerate(SETS)]
            assert [st.origin(i) for i in range(S)] == list(zip(r.origin, sets_now)) and st.info()[4] == r.R
            assert f.to(len(c.plan) - 1) == c.P + c.L and sum(r.bad[r.at:]) >= 10


# ---- c. raw pushes with FIR and prefilter --------------------------------------------------------------------
@pytest.mark.parametrize("base", list(sk.DECIM))
def test_raw_pushes_with_fir_and_prefilter(base, capped):
    """off, slot0 and d0 of every push come from a 64-bit raw position."""
    import torch

    c = sk.decim_case(base)
    sets = sb.sets(c.C, c.T, c.N)
    qd, rows, keep = sk.decim_rows(c, sd.two_pass)
    assert rows[:, keep].any(axis=-1).all()  # what the CPU certifies on the NumPy quantiser holds on this one
    x = sd.frames(c.C, c.T, c.q, c.K)
    D = decimate.raw_decimated
    for cap in (1, 0):
        capped(cap)
        with lib.Bank(sets, pf.SCALES) as bank, lib.Streams(bank, SETS, HOP, MAX_PUSH) as st:
            st.decimate(c.q, c.h)
            st.prefilter(c.sos)
            lib.streams_seek(st, [c.P] * S)
            assert st.raw_info() == [c.q, c.K, c.P, c.D0] and st.info()[4:] == [c.D0, 0]
            assert [st.origin(i) for i in range(S)] == [(c.D0, s) for s in SETS]
            first = 0
            for j, (P, n, d0, m, k, _) in enumerate(c.plan):
                assert st.raw_info()[2:] == [P, d0]
                y, nbad = st.push_raw(dev(torch, np.ascontiguousarray(x[:, P - c.P: P - c.P + n])))
                assert st.raw_info()[2:] == [P + n, D(c.q, P + n)] == [P + n, d0 + m] and st.info()[4] == d0 + m
                assert tuple(y.shape) == (S, k, c.N) and int(nbad.item()) == S * c.below[j], (j, tuple(y.shape))
                same_rows(y.cpu().numpy(), rows[:, first: first + k], f"push {j} at raw {P}, cap {cap}")
                first += k
            assert first == len(c.onsets) == st.info()[5] and st.raw_info()[2] == c.P + c.L > c.B > c.P
            sd.check_rings(st, sets, qd, base=c.D0)


# ---- d. an each-group, plain pushes --------------------------------------------------------------------------
class EachFeed:
    """The ticks of an each-group through the C entry, session i from its own cursor into x [S][C][L]
    (int8) and from position P[i].  Every tick: cnt_out, win0 and positions() are held to
    support_streams_each.plan_each, n_bad to the refusals so far, and the rows past a session's k to
    GUARD."""

    def __init__(self, torch, st, x, P):
        self.torch, self.st, self.x = torch, st, x
        self.T, self.N = st.bank.dims.T, st.bank.dims.N
        self.cur, self.pos, self.refused, self.done = [0] * S, [int(p) for p in P], 0, 0
        self.rows = [[] for _ in range(S)]
        self.nb = torch.zeros((3,), dtype=torch.int32, device="cuda")

    def tick(self, n_max, counts):
        torch, st, C = self.torch, self.st, self.x.shape[1]
        plans = [se.plan_each(self.T, HOP, st.cap, self.pos[i], counts[i], n_max) for i in range(S)]
        slot = np.full((S, C, n_max), JUNK, np.int8)
        for i, (ok, n, *_) in enumerate(plans):
            slot[i, :, :n] = self.x[i, :, self.cur[i]: self.cur[i] + n]
        kmax = se.each_rows(HOP, n_max)
        xs, cin = torch.from_numpy(slot).cuda(), torch.tensor(counts, dtype=torch.int32, device="cuda")
        y = torch.full((S, kmax, self.N), GUARD, dtype=torch.int8, device="cuda")
        cout = torch.full((S,), -7, dtype=torch.int32, device="cuda")
        win0 = torch.full((S,), -7, dtype=torch.int64, device="cuda")
        before = st.positions().tolist()
        torch.cuda.synchronize()
        rc = lib.load().net_streams_push_each(st.handle, xs.data_ptr(), 1, cin.data_ptr(), n_max, y.data_ptr(), cout.data_ptr(),
                                              win0.data_ptr(), self.nb.data_ptr() + 4, torch.cuda.current_stream().cuda_stream)
        assert rc == OK, (rc, self.done)
        torch.cuda.synchronize()
        yh, ch, wh = y.cpu().numpy(), cout.tolist(), win0.tolist()
        for i, (ok, n, _, k, _, W0) in enumerate(plans):
            assert ch[i] == (k if ok else -1) and wh[i] == W0, (self.done, i, ch, wh, k, W0)
            assert (yh[i, k:] == GUARD).all(), f"tick {self.done}, session {i}: rows past its {k} were written"
            self.rows[i].append(yh[i, :k])
            self.cur[i] += n
            self.pos[i] += n
            self.refused += not ok
        after = st.positions().tolist()
        assert before == [p - pl[1] for p, pl in zip(self.pos, plans)] and after == self.pos, (self.done, before, after)
        assert self.nb.tolist() == [0, self.refused, 0], (self.done, self.nb.tolist(), self.refused)
        self.done += 1

    def to(self, t, n_max, counts):
        while self.done <= t:
            self.tick(int(n_max[self.done]), [int(v) for v in counts[self.done]])
        return list(self.pos)

    def result(self):
        return [np.concatenate(p, axis=0) if p else np.zeros((0, self.N), np.int8) for p in self.rows]


def compared(got, ref, T):
    """The rows of the windows that start at or after each session's seek position, and how many are
    left out."""
    assert len(got) == len(ref) == S
    for i, (g, (r, keep)) in enumerate(zip(got, ref)):
        assert g.shape == r.shape and (~keep).sum() <= -(-(T - 1) // HOP), (i, g.shape, r.shape, int((~keep).sum()))
    same_each([g[k] for g, (_, k) in zip(got, ref)], [r[k] for r, k in ref])


def test_each_group_plain_pushes(banks, capped):
    """Sessions at 2^31 - a and 2^32 - b cross their boundary mid-schedule, one runs past 2^53, one runs
    into EACH_POS_LIMIT (accepted, then refused with cnt_out -1 and one count in n_bad each time, its
    position unchanged, a count of 0 accepted in between), one stays at 0 and gives today's rows."""
    import torch

    c = sk.each_case()
    x, ref = ss.chunks(c.C, c.T), sk.each_rows()
    for cap in (1, 0):
        capped(cap)
        with lib.StreamsEach(banks(c.C, c.T, c.N), SETS, HOP, MAX_PUSH) as st:
            lib.streams_seek(st, c.P)
            assert st.positions().tolist() == c.P and st.info() == [S, HOP, MAX_PUSH, c.cap, 0, -1]
            f = EachFeed(torch, st, x, c.P)
            pos = f.to(len(c.n_max) - 1, c.n_max, c.counts)
            assert pos == [p + int(n) for p, n in zip(c.P, c.fed)] and f.refused == int((~c.walk.ok).sum()) >= 3
            assert st.info()[4:] == [len(c.n_max), -1]
            compared(f.result(), ref, c.T)
            sd.check_rings(st, sb.sets(c.C, c.T, c.N), [x[i][:, : int(c.fed[i])] for i in range(S)], base=c.P)


# ---- e. an each-group, raw pushes ----------------------------------------------------------------------------
def test_each_group_raw_pushes(capped):
    """d's layout on the raw axis with EACH_RAW_LIMIT, under (2, 7) with a prefilter: cnt_out, win0,
    raw_positions() and positions() are held to support_decim_each.plan_each_raw at every tick
    (RawDriver)."""
    import torch

    c = sk.each_raw_case()
    sets = sb.sets(c.C, c.T, c.N)
    qd, ref = sk.each_raw_rows(c, sd.two_pass)
    assert all(r[k].any(axis=-1).all() for r, k in ref)
    for cap in (1, 0):
        capped(cap)
        with lib.Bank(sets, pf.SCALES) as bank, lib.StreamsEach(bank, SETS, HOP, MAX_PUSH) as st:
            st.decimate(c.q, c.h)
            st.prefilter(c.sos)
            lib.streams_seek(st, c.P)
            assert st.raw_positions().tolist() == c.P and st.positions().tolist() == c.D0
            d = sde.RawDriver(torch, st, c.x, c.q, c.K, start=c.P)
            refused = 0
            for t in range(len(c.n_max)):
                d.push(int(c.n_max[t]), [int(v) for v in c.counts[t]])
                refused += int((~c.walk.ok[t].astype(bool)).sum())
                assert d.nb.tolist() == [0, refused, 0], (t, d.nb.tolist(), refused)
            got, _ = d.result()
            assert d.P == [p + int(n) for p, n in zip(c.P, c.fed)] and refused >= 3
            compared(got, ref, c.T)
            sd.check_rings(st, sets, qd, base=c.D0)


# ---- f. windows at given onsets, far from zero ---------------------------------------------------------------
def query(st, items, features):
    """One call of net_streams_windows_at[_feat] on the (session, onset) items: ([W][N], the feature
    rows or None, n_bad), the logits between guard bytes that must stay."""
    import torch

    d = st.bank.dims
    W, N = len(items), d.N
    ses = torch.tensor([int(i) for i, _ in items], dtype=torch.int32).cuda()
    ons = torch.tensor([int(o) for _, o in items], dtype=torch.int64).cuda()
    ybuf = torch.full((LEAD + W * N + LEAD,), GUARD, dtype=torch.int8, device="cuda")
    feat = torch.full((W, d.F2, d.T64), GUARD, dtype=torch.int8, device="cuda") if features else None
    nb = torch.zeros((3,), dtype=torch.int32, device="cuda")
    lead = (st.handle, ses.data_ptr(), ons.data_ptr(), W, ybuf.data_ptr() + LEAD)
    tail = (nb.data_ptr() + 4, torch.cuda.current_stream().cuda_stream)
    if features:
        rc = lib.load().net_streams_windows_at_feat(*lead, feat.data_ptr(), *tail)
    else:
        rc = lib.load().net_streams_windows_at(*lead, *tail)
    assert rc == OK, rc
    torch.cuda.synchronize()
    y, nbl = ybuf.cpu().numpy(), nb.tolist()
    assert (y[:LEAD] == GUARD).all() and (y[LEAD + W * N:] == GUARD).all() and nbl[0] == 0 == nbl[2]
    return y[LEAD: LEAD + W * N].reshape(W, N), feat.cpu().numpy() if features else None, nbl[1]


def ask(st, good, bad, P, what):
    """The valid items `good` and the invalid items `bad`, interleaved (an invalid item first and last
    where there are any), through both entries: the oracle's rows, zero rows and one count each."""
    d = st.bank.dims
    items, is_bad = [], []
    for k, g in enumerate(good):
        if k < len(bad):
            items.append(bad[k])
            is_bad.append(True)
        items.append(g)
        is_bad.append(False)
    items += bad[len(good):] + bad[:1]
    is_bad = np.array(is_bad + [True] * (len(items) - len(is_bad)))
    for features in (False, True):
        ref = sk.at_reference(d.C, d.T, d.N, good, P, features)
        y, f, nbad = query(st, items, features)
        ey = np.zeros((len(items), d.N), np.int8)
        ey[~is_bad] = ref[0] if features else ref
        assert nbad == int(is_bad.sum()), (what, features, nbad, int(is_bad.sum()))
        same(y, ey, f"{what}, features {features}")
        if features:
            ef = np.zeros(f.shape, np.int8)
            ef[~is_bad] = ref[1]
            same(f, ef, f"{what}, the feature rows")


@pytest.mark.parametrize("base", sk.BASES)
def test_windows_at_on_the_uniform_groups(base, banks, capped):
    """The group of a with its default origin: at the early point onsets just below the seek position
    are in the ring and complete, and the origin alone refuses them; at the crossing the onsets asked
    lie on both sides of the base."""
    import torch

    c = sk.uniform_case(base)
    rows, _ = sk.uniform_rows(base)
    xd = torch.from_numpy(np.array(ss.chunks(c.C, c.T))).cuda()
    with lib.Streams(banks(c.C, c.T, c.N), SETS, HOP, MAX_PUSH) as st:
        lib.streams_seek(st, [c.P] * S)
        f = Feed(st, xd, c.plan, rows, [S * b for b in c.below])
        for n, j in enumerate(sk.at_points(c)):
            pos = f.to(j)
            assert st.at_span() == (max(pos - c.cap, 0), pos - c.T)
            bad = [(1, c.P - 1), (3, c.P - 2), (0, c.P - 1)] if n == 0 else [(2, pos - c.T + 1)]
            for cap in (1, 0):
                capped(cap)
                ask(st, sk.uniform_at_items(c, pos), bad, c.P, f"{base} at {pos}, cap {cap}")


@pytest.mark.parametrize("base", ["2^53", "top"])
def test_windows_at_where_only_the_distance_refuses(base, banks, capped):
    """A group seeked with every origin 0, so that the origin refuses nothing: the newest window's onset
    2^32 and 2^33 lower is non-negative and at or below the position, and only d > cap refuses it.  A d
    cut to 32 bits would read T there and answer."""
    import torch

    c = sk.uniform_case(base)
    rows, keep = sk.uniform_rows(base)
    xd = torch.from_numpy(np.array(ss.chunks(c.C, c.T))).cuda()
    with lib.Streams(banks(c.C, c.T, c.N), SETS, HOP, MAX_PUSH) as st:
        lib.streams_seek(st, [c.P] * S, [0] * S)
        assert [st.origin(i) for i in range(S)] == [(0, s) for s in SETS] and st.info()[4] == c.P
        first, pos = 0, c.P
        for j, (p, n, k, _, _) in enumerate(c.plan):  # no window is refused: those from before P are not compared
            y, nbad = st.push(xd[:, :, p - c.P: p - c.P + n].contiguous())
            assert int(nbad.item()) == 0 and tuple(y.shape) == (S, k, c.N)
            w = np.flatnonzero(keep[first: first + k])
            same_rows(y.cpu().numpy()[:, w], rows[:, first + w], f"push {j}")
            first += k
        pos = st.info()[4]
        bad = [(1, o) for o in sk.far_bad_onsets(c.T, c.cap, pos).values()]
        for cap in (1, 0):
            capped(cap)
            ask(st, sk.uniform_at_items(c, pos), bad, c.P, f"{base}, origin 0, cap {cap}")


def test_windows_at_on_the_each_group(banks, capped):
    """The each-group of d (floor 0): after the tick that takes each crossing session past its base,
    onsets on both sides of it; after the last tick the far invalid onsets of the sessions past 2^53 and
    at the limit."""
    import torch

    c = sk.each_case()
    ticks, _ = sk.each_at_ticks(c)
    with lib.StreamsEach(banks(c.C, c.T, c.N), SETS, HOP, MAX_PUSH) as st:
        lib.streams_seek(st, c.P)
        f = EachFeed(torch, st, ss.chunks(c.C, c.T), c.P)
        for t in sorted(set(ticks)):
            pos = f.to(t, c.n_max, c.counts)
            good = [(i, o) for i in range(S) for o in sk.at_onsets(c.T, c.cap, pos[i], c.P[i])]
            good = [good[k] for k in np.random.default_rng([c.T, t]).permutation(len(good))]
            assert len({i for i, _ in good}) >= 4
            bad = [(i, pos[i] - c.T + 1) for i in (0, 1)]
            if t == len(c.n_max) - 1:
                bad = [(i, o) for i in (2, sk.LIMIT_AT) for o in sk.far_bad_onsets(c.T, c.cap, pos[i]).values()]
            for cap in (1, 0):
                capped(cap)
                ask(st, good, bad, c.P, f"tick {t}, cap {cap}")


# ---- g. the hook's refusals ------------------------------------------------------------------------------------
def test_refusals_on_a_uniform_group(banks, gpu):
    import torch

    C, T, N = sk.GEOMETRY
    ns, x = ss.schedule(T), ss.chunks(C, T)
    xd = torch.from_numpy(np.array(x)).cuda()
    today = ss.expected(ss.table(C, T, N))
    P = 2**40 + 7
    with lib.Streams(banks(C, T, N), SETS, HOP, MAX_PUSH) as st:
        was = (st.info(), [st.origin(i) for i in range(S)])
        assert seek_rc(None, [P] * S) == INV and seek_rc(st, None) == INV and seek_rc(st, None, [0] * S) == INV
        for pos in ([-1] * S, [-2**63] * S, [P, P, P + 1, P, P], [P] * (S - 1) + [0], [0, P, P, P, P]):
            assert seek_rc(st, pos) == INV, pos
        for origin in ([0, 0, -1, 0, 0], [P + 1] + [0] * (S - 1), [0] * (S - 1) + [I63], [-2**63] * S):
            assert seek_rc(st, [P] * S, origin) == INV, origin
        with pytest.raises(lib.NetError):
            lib.streams_seek(st, [-1] * S)
        with pytest.raises(ValueError):
            lib.streams_seek(st, [P] * (S - 1))
        assert (st.info(), [st.origin(i) for i in range(S)]) == was
        f = Feed(st, xd, ss.plan(T, HOP, ns), today, [0] * len(ns))  # the rows of an unseeked run
        f.to(0)
        assert seek_rc(st, [st.info()[4]] * S) == INV and seek_rc(st, [P] * S) == INV  # after a push
        assert f.to(len(ns) - 1) == ss.total(T)
    with lib.Streams(banks(C, T, N), SETS, HOP, MAX_PUSH) as st:  # after a restart, at position 0 too
        st.restart(1, 3)
        was = (st.info(), [st.origin(i) for i in range(S)])
        assert seek_rc(st, [P] * S) == INV and seek_rc(st, [0] * S) == INV
        assert (st.info(), [st.origin(i) for i in range(S)]) == was
    with lib.Streams(banks(C, T, N), SETS, HOP, MAX_PUSH) as st:  # after a seek; origins at both ends are taken
        assert seek_rc(st, [P] * S, [0, P, 7, P - 1, 0]) == OK
        was = (st.info(), [st.origin(i) for i in range(S)])
        assert was == ([S, HOP, MAX_PUSH, st.cap, P, 0], list(zip([0, P, 7, P - 1, 0], SETS)))
        assert seek_rc(st, [P] * S) == INV and seek_rc(st, [0] * S) == INV
        assert (st.info(), [st.origin(i) for i in range(S)]) == was
    with lib.Bank(sb.sets(C, T, N), pf.SCALES) as bank, lib.Streams(bank, SETS, HOP, MAX_PUSH) as st:
        q, K = 3, 33  # with a decimator the entries are raw positions and an origin lies in 0 .. D(P)
        st.decimate(q, sd.taps(K, 11))
        D = decimate.raw_decimated(q, P)
        assert P % q and seek_rc(st, [P] * S, [D + 1] + [0] * (S - 1)) == INV and seek_rc(st, [P] * S, [P] * S) == INV
        assert st.raw_info() == [q, K, 0, 0] and st.info()[4] == 0
        assert seek_rc(st, [P] * S, [D] * S) == OK and st.raw_info() == [q, K, P, D]
        assert [st.origin(i) for i in range(S)] == [(D, s) for s in SETS]
        with pytest.raises(lib.NetError):  # the setters want a group at 0: the hook comes after them
            st.prefilter(pf.sections(pf.M, sk.SOS_SEED))


def test_refusals_on_an_each_group(banks, gpu):
    import torch

    C, T, N = sk.GEOMETRY
    n_max, counts = se.schedule(T)
    x = ss.chunks(C, T)
    P = [2**40 + 5, 3, 0, 2**35 + 1, se.POS_LIMIT]
    with lib.StreamsEach(banks(C, T, N), SETS, HOP, MAX_PUSH) as st:
        was = (st.info(), st.positions().tolist(), [st.origin(i) for i in range(S)])
        assert was[1] == [0] * S
        assert seek_rc(st, None) == INV and seek_rc(st, P, [0] * S) == INV  # an each-group takes no origin
        for i, v in ((0, -1), (4, se.POS_LIMIT + 1), (2, I63), (1, -2**63)):
            assert seek_rc(st, [v if k == i else p for k, p in enumerate(P)]) == INV, (i, v)
        assert (st.info(), st.positions().tolist(), [st.origin(i) for i in range(S)]) == was
        f = EachFeed(torch, st, x, [0] * S)  # the rows of an unseeked run
        f.to(0, n_max, counts)
        assert seek_rc(st, P) == INV  # after a push
        pos = f.to(len(n_max) - 1, n_max, counts)
        assert pos == se.walk(T).fed.tolist()
        same_each(f.result(), se.expected(ss.table(C, T, N), se.walk(T).fed, T))
    with lib.StreamsEach(banks(C, T, N), SETS, HOP, MAX_PUSH) as st:  # after a restart
        st.restart(0, 2)
        assert seek_rc(st, P) == INV and st.positions().tolist() == [0] * S
    with lib.StreamsEach(banks(C, T, N), SETS, HOP, MAX_PUSH) as st:  # the limit itself is taken; a second seek is not
        assert seek_rc(st, P) == OK and st.positions().tolist() == P and st.info()[4:] == [0, -1]
        assert seek_rc(st, P) == INV and seek_rc(st, [0] * S) == INV and st.positions().tolist() == P
    with lib.Bank(sb.sets(C, T, N), pf.SCALES) as bank, lib.StreamsEach(bank, SETS, HOP, MAX_PUSH) as st:
        q, K = sk.EACH_QK  # with a decimator the limit is the raw one
        st.decimate(q, sd.taps(K, 11))
        R = [2**40 + 5, 3, 0, 2**35 + 1, sde.RAW_LIMIT]
        assert seek_rc(st, R[:4] + [sde.RAW_LIMIT + 1]) == INV and seek_rc(st, R[:4] + [se.POS_LIMIT]) == INV
        assert st.raw_positions().tolist() == [0] * S == st.positions().tolist()
        assert seek_rc(st, R) == OK and st.raw_positions().tolist() == R
        assert st.positions().tolist() == [decimate.raw_decimated(q, p) for p in R]
        with pytest.raises(lib.NetError):
            st.prefilter(pf.sections(pf.M, sk.SOS_SEED))
