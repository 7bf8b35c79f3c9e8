"""Live streams on the GPU (net_streams_push[_f32], forward_stream.hpp): five sessions under sets
(0, 1, 1, 3, 0) of a bank of five, their chunks pushed by a fixed schedule into the sessions' layer-1
rings, and the windows of the global grid returned as they end.

The reference of every row is the C oracle of the session's set on the materialised window of the
session's concatenated chunks (support_streams.table, computed once per geometry), never another GPU
entry, and every comparison is byte-exact.  tests/test_streams_cpu.py certifies the inputs: no
expected row is all zeros (zeros mark an unanswered window), a session's rows under a neighbour's
set or under the set it is restarted to differ on at least 75 % of its windows, and the windows at
o and o + 1 differ for at least half of the onsets, so a ring read one sample off shows.  The
schedule puts the first new sample at every residue mod 4, crosses the ring's seam while writing,
has pushes that complete no window and wraps the ring twice."""
import numpy as np
import pytest

import observability
import support_bank as sb
import support_streams as ss
import support_windows_bank as swb
from mibminet import lib
from mibminet.params import ParamSet
from support import CAPS, GUARD, capped, want  # noqa: F401 (capped: a fixture)
from support_bank import banks  # noqa: F401 (a fixture)

pytestmark = pytest.mark.gpu


class Driver:
    """Pushes the chunks of x ([S][C][L]: a NumPy int8 array, or a float32 device tensor) into the
    group `st` through the C entry.  Each chunk is staged contiguously at a byte offset that cycles
    through 0 .. 3 (float32: 0 and 4); each push's rows go to their own 4-byte aligned region of one
    logits buffer prefilled with GUARD, and the counter sits between two others.  rows() gives
    [S][windows so far][N] and checks that nothing outside the regions was written."""

    def __init__(self, torch, st, x, layout="ct", stream=None):
        self.torch, self.st, self.layout, self.stream = torch, st, layout, stream
        self.f32 = not isinstance(x, np.ndarray)
        xd = x if self.f32 else torch.from_numpy(np.array(x)).cuda()
        self.S, self.C, self.L = (int(v) for v in xd.shape)
        self.xd = xd if layout == "ct" else xd.transpose(1, 2).contiguous()
        self.item = 4 if self.f32 else 1
        self.N = st.bank.dims.N
        W = ss.windows_count(st.bank.dims.T, self.L, st.hop)
        self.y = torch.full((self.S * self.N * W + 4 * 1024 + 64,), GUARD, dtype=torch.int8, device="cuda")
        self.stage = torch.zeros(8 + self.S * self.C * st.max_push * self.item + 64, dtype=torch.uint8, device="cuda")
        self.nb = torch.zeros((3,), dtype=torch.int32, device="cuda")
        self.regions, self.used, self.pushes = [], 0, 0

    def push(self, n, expect=lib.NET_OK):
        torch, st = self.torch, self.st
        pos = st.info()[4]
        k = st.windows(n)
        off = (self.pushes % 2) * 4 if self.f32 else self.pushes % 4
        nbytes = self.S * self.C * n * self.item
        dt = torch.float32 if self.f32 else torch.int8
        shape = (self.S, self.C, n) if self.layout == "ct" else (self.S, n, self.C)
        src = self.xd[:, :, pos: pos + n] if self.layout == "ct" else self.xd[:, pos: pos + n, :]
        s = torch.cuda.current_stream() if self.stream is None else self.stream
        with torch.cuda.stream(s):
            self.stage[off: off + nbytes].view(dt).view(*shape).copy_(src)
        start = (self.used + 3) // 4 * 4
        assert start + self.S * k * self.N <= self.y.numel() - 64
        A = lib.load()
        xp, yp, bp = self.stage.data_ptr() + off, self.y.data_ptr() + start, self.nb.data_ptr() + 4
        if self.f32:
            rc = A.net_streams_push_f32(st.handle, xp, n, yp, bp, s.cuda_stream)
        else:
            rc = A.net_streams_push(st.handle, xp, 1 if self.layout == "ct" else 0, n, yp, bp, s.cuda_stream)
        assert rc == expect, (rc, pos, n)
        if rc == lib.NET_OK:
            self.regions.append((start, k))
            self.used = start + self.S * k * self.N
            self.pushes += 1
            assert st.info()[4] == pos + n
        return k

    def run(self, ns):
        for n in ns:
            self.push(n)
        return self

    def rows(self):
        """([S][W][N] of the windows so far, the three counters)."""
        self.torch.cuda.synchronize()
        y = self.y.cpu().numpy()
        mask = np.ones(y.shape, bool)
        parts = []
        for start, k in self.regions:
            size = self.S * k * self.N
            mask[start: start + size] = False
            parts.append(y[start: start + size].reshape(self.S, k, self.N))
        assert (y[mask] == GUARD).all(), "bytes outside the pushes' rows were written"
        return np.concatenate(parts, axis=1), self.nb.cpu().tolist()


# ---- 1. every row of every push -------------------------------------------------------------------
@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("layout", ["ct", "tc"])
@pytest.mark.parametrize("C,T,N", ss.GEOMETRIES)
def test_every_row_of_every_push(C, T, N, layout, cap, banks, capped):
    import torch

    expect = ss.expected(ss.table(C, T, N))
    capped(cap)
    with lib.Streams(banks(C, T, N), ss.SETS, ss.HOP, ss.MAX_PUSH) as st:
        assert st.cap == ss.cap(T, ss.MAX_PUSH) and st.info() == [ss.S, ss.HOP, ss.MAX_PUSH, st.cap, 0, 0]
        d = Driver(torch, st, ss.chunks(C, T), layout).run(ss.schedule(T))
        rows, nb = d.rows()
        assert nb == [0, 0, 0]
        assert rows.shape == expect.shape and st.info()[4:] == [ss.total(T), expect.shape[1]]
        for i in range(ss.S):
            bad = np.flatnonzero((rows[i] != expect[i]).any(axis=1))
            assert bad.size == 0, f"session {i}: {bad.size} of {len(expect[i])} windows differ, first {bad[:5]}"
    assert banks(C, T, N).device_copies() == 1


# ---- 2. the ring itself ---------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["ct", "tc"])
@pytest.mark.parametrize("C,T,N", ss.GEOMETRIES)
def test_ring_holds_layer1_of_the_last_samples(C, T, N, layout, banks, capped):
    """After a push that ends at position p the ring of session i holds, at t mod cap and again at
    t mod cap + cap, the oracle's layer-1 output of sample t under the session's set for the last
    min(p, cap) samples, and zeros where nothing was written yet."""
    import torch

    x, sets, ns = ss.chunks(C, T), sb.sets(C, T, N), ss.schedule(T)
    y1 = [swb.layer1_of(sets[ss.SETS[i]], x[i]) for i in range(ss.S)]
    plan = ss.plan(T, ss.HOP, ns)
    capped(3)
    with lib.Streams(banks(C, T, N), ss.SETS, ss.HOP, ss.MAX_PUSH) as st:
        c = st.cap
        # after the first pushes (one sample each, then a full one), after every push that crosses the
        # seam and the one after it, every 29th push, and the last
        look = {0, 1, 2, 3, 4, 5, len(ns) - 1} | set(range(6, len(ns), 29))
        for j, (pos, n, *_) in enumerate(plan):
            if pos % c + n >= c:
                look |= {j, min(j + 1, len(ns) - 1)}
        d = Driver(torch, st, x, layout)
        for j, (pos, n, *_) in enumerate(plan):
            d.push(n)
            if j not in look:
                continue
            p = pos + n
            t = np.arange(max(0, p - c), p)
            for i in range(ss.S):
                ring = lib.streams_ring(st, i)
                assert ring.shape == (16, 2 * c)
                np.testing.assert_array_equal(ring[:, :c], ring[:, c:], err_msg=f"the two copies, push {j}, session {i}")
                np.testing.assert_array_equal(ring[:, t % c], y1[i][:, t], err_msg=f"push {j} to {p}, session {i}")
                if p < c:
                    assert not ring[:, p:c].any(), f"push {j}: positions never written"
        assert len(look) >= 8


# ---- 3. float input -------------------------------------------------------------------------------
_SCALES = [0.5, 1.3, 3.0, 7.25, 100.0]


@pytest.mark.parametrize("C,T,N", [(19, 480, 3), (64, 480, 2)])
def test_float_input_with_the_sets_scales(C, T, N, capped):
    """Every session's samples as floats that its set's scale quantises to the int8 chunks
    (support.dequant's construction), non-finite samples planted as support.float_recording plants
    them.  The reference is the oracle on the two-pass quantisation (net_quantize_input_f32) of each
    session with its set's scale."""
    import torch

    sets, x = sb.sets(C, T, N), ss.chunks(C, T)
    L = x.shape[2]
    v = np.arange(-127, 128)
    xf = np.zeros(x.shape, np.float32)
    for i, s in enumerate(ss.SETS):
        lut = ((v + 0.5 * np.sign(v)) * (_SCALES[s] / 127.0)).astype(np.float32)
        xf[i] = lut[x[i].astype(np.int16) + 127]
    xd = torch.from_numpy(xf).cuda()
    xd[:, 0, :7] = torch.tensor([float("nan"), float("inf"), -float("inf"), 3.0, -3.0, 0.0, -0.0], device="cuda")
    xd[:, C - 1, L - 3:] = torch.tensor([float("nan"), -float("inf"), float("inf")], device="cuda")
    mid = T + 101  # and inside the stream, where a chunk ends
    xd[1, C // 2, mid: mid + 3] = torch.tensor([float("inf"), float("nan"), -1e30], device="cuda")
    expect = []
    for i, s in enumerate(ss.SETS):
        q = lib.quantize_input_torch(xd[i: i + 1].contiguous(), _SCALES[s])  # [1][stride], the trial [L][C]
        q = np.ascontiguousarray(q.cpu().numpy()[0, : L * C].reshape(L, C).T)
        keep = np.ones((C, L), bool)
        keep[0, :7] = keep[C - 1, L - 3:] = False
        if i == 1:
            keep[C // 2, mid: mid + 3] = False
        assert np.array_equal(q[keep], x[i][keep])  # the construction, where nothing is planted
        expect.append(ss.rows_of(sets[s], q, T))
    expect = np.stack(expect)
    with lib.Bank(sets, _SCALES) as bank, lib.Bank(sets) as bare:
        for cap in (1, 0):
            capped(cap)
            with lib.Streams(bank, ss.SETS, ss.HOP, ss.MAX_PUSH) as st:
                rows, nb = Driver(torch, st, xd).run(ss.schedule(T)).rows()
                assert nb == [0, 0, 0]
                np.testing.assert_array_equal(rows, expect, err_msg=f"cap {cap}")
        with lib.Streams(bank, ss.SETS, ss.HOP, ss.MAX_PUSH) as st:  # the Python entry
            y, nbad = st.push_f32(xd[:, :, :5].contiguous())
            assert tuple(y.shape) == (ss.S, 0, N) and int(nbad.item()) == 0
        with lib.Streams(bare, ss.SETS, ss.HOP, ss.MAX_PUSH) as st:  # no scales
            with pytest.raises(ValueError):
                st.push_f32(xd[:, :, :5].contiguous())
            assert lib.load().net_streams_push_f32(st.handle, xd.data_ptr(), 5, None, None, None) == lib.NET_ERR_INVALID
            assert st.info()[4] == 0


# ---- 4. hops --------------------------------------------------------------------------------------
@pytest.mark.parametrize("hop", [1, 50, 70])
def test_hops(hop, banks, capped):
    """hop = 1 (every push returns n windows once T samples are in), hop > max_push (most pushes
    return none) and hop > T (samples no window reads)."""
    import torch

    C, T, N = 8, 64, 2
    ns = (37, 26, 1, 1, 1, 5, 37, 16, 2, 37, 37, 9, 33, 37, 4)
    x = ss.chunks(C, T)[:, :, : sum(ns)]
    sets = sb.sets(C, T, N)
    expect = np.stack([ss.rows_of(sets[ss.SETS[i]], x[i], T, hop) for i in range(ss.S)])
    ks = [k for _, _, k, _, _ in ss.plan(T, hop, ns)]
    assert sum(ks) == expect.shape[1] and (hop != 1 or ks[2:] == list(ns[2:])) and (hop == 1 or ks.count(0) > len(ks) // 2)
    for cap in (1, 0):
        capped(cap)
        with lib.Streams(banks(C, T, N), ss.SETS, hop, ss.MAX_PUSH) as st:
            d = Driver(torch, st, x, "tc" if cap else "ct")
            assert [d.push(n) for n in ns] == ks
            rows, nb = d.rows()
            assert nb == [0, 0, 0]
            np.testing.assert_array_equal(rows, expect, err_msg=f"hop {hop}, cap {cap}")


# ---- 5. restart -----------------------------------------------------------------------------------
@pytest.mark.parametrize("C,T,N", ss.GEOMETRIES)
def test_restart(C, T, N, banks, capped):
    """Session 2 restarts under set 4 at a position that is no multiple of the hop: its windows that
    start before the origin come back as zeros and are counted, the later ones are the oracle's
    under set 4, and the other sessions are what they were."""
    import torch

    i0, new = ss.RESTART
    ns, tab = ss.schedule(T), ss.table(C, T, N)
    plan = ss.plan(T, ss.HOP, ns)
    # the first push boundary past the middle of the answered onsets that is no multiple of the hop
    at = next(j for j, (pos, *_) in enumerate(plan) if pos > (ss.total(T) - T) // 2 and pos % ss.HOP)
    origin = plan[at][0]
    expect = ss.expected(tab).copy()
    onsets = np.arange(expect.shape[1]) * ss.HOP
    done = sum(k for _, _, k, _, _ in plan[:at])  # windows returned before the restart
    late = np.arange(expect.shape[1]) >= done
    zero = late & ~ss.answered(onsets, origin)
    expect[i0][late] = tab[(i0, new)][late]
    expect[i0][zero] = 0
    assert zero.sum() >= (min(origin, T) - 3) // ss.HOP and (late & ~zero).sum() > 20
    for cap in (1, 0):
        capped(cap)
        with lib.Streams(banks(C, T, N), ss.SETS, ss.HOP, ss.MAX_PUSH) as st:
            d = Driver(torch, st, ss.chunks(C, T)).run(ns[:at])
            assert st.origin(i0) == (0, ss.SETS[i0])
            st.restart(i0, new)
            assert st.origin(i0) == (origin, new) and st.info()[4] == origin
            assert [st.origin(i) for i in range(ss.S) if i != i0] == [(0, s) for i, s in enumerate(ss.SETS) if i != i0]
            rows, nb = d.run(ns[at:]).rows()
            assert nb == [0, int(zero.sum()), 0], cap
            for i in range(ss.S):
                np.testing.assert_array_equal(rows[i], expect[i], err_msg=f"session {i}, cap {cap}")
            L = lib.load()
            for i, s in ((ss.S, 0), (2**40, 0), (0, -1), (0, 5), (0, 2**31 - 1)):
                assert L.net_streams_restart(st.handle, i, s, None) == lib.NET_ERR_INVALID
            assert st.origin(0) == (0, 0)


# ---- 6. every ring byte is seen -------------------------------------------------------------------
@pytest.mark.parametrize("case", observability.CASES, ids=repr)
def test_every_ring_byte_reaches_a_logit(case, gpu):
    """The certified trials of tests/observability.py laid end to end as one session, hop = T: a wrong
    byte anywhere in a window's y1 rows changes a logit of some trial.  max_push is coprime to 16, so
    successive trials sit at different places of the ring and the pushes' 16-sample blocks at every
    phase of it."""
    import torch

    name, ps, x = case
    B, C, T = x.shape
    mp = 4099 if T > 200 else 331
    rec = np.ascontiguousarray(x.transpose(1, 0, 2).reshape(1, C, B * T))
    expect = want(ps, x)
    with lib.Bank([ps]) as bank, lib.Streams(bank, [0], T, mp) as st:
        assert bank.exact_division == case.exact and np.gcd(mp, 16) == 1
        ns = [mp] * (B * T // mp) + ([B * T % mp] if B * T % mp else [])
        rows, nb = Driver(torch, st, rec).run(ns).rows()
        assert nb == [0, 0, 0] and rows.shape == (1, B, ps.dims.N)
        bad = np.flatnonzero((rows[0] != expect).any(axis=1))
        assert bad.size == 0, f"{name}: {bad.size} of {B} trials differ, first {bad[:5]}"
        # the trials did sit at many places in the ring, and the pushes started at every residue mod 16
        assert len({(b * T) % st.cap for b in range(B)}) >= min(B, 8)
        assert len(ns) < 16 or {(j * mp) % st.cap % 16 for j in range(len(ns))} == set(range(16))
    case.drop()


# ---- 7. the build variants ------------------------------------------------------------------------
@pytest.mark.parametrize("variant", list(sb.VARIANTS))
@pytest.mark.parametrize("C,T,N", sb.VARIANT_GEOMETRIES)
def test_variants(C, T, N, variant, capped):
    import torch

    sets = sb.VARIANTS[variant](C, T, N)
    mp = 1000
    ns = [mp] * ((T - 20) // mp) + [(T - 20) % mp, 37, 1, 30, 16, 5, 37, 23, 2]
    x = ss.chunks(C, T)[:, :, : sum(ns)]
    expect = np.stack([ss.rows_of(sets[ss.SETS[i]], x[i], T) for i in range(ss.S)])
    assert expect.shape[1] > 40
    with lib.Bank(sets) as bank:
        assert bank.exact_division == (variant in sb.EXACT)
        for layout, cap in (("ct", 1), ("ct", 0), ("tc", 1)):
            capped(cap)
            with lib.Streams(bank, ss.SETS, ss.HOP, mp) as st:
                rows, nb = Driver(torch, st, x, layout).run(ns).rows()
                assert nb == [0, 0, 0]
                np.testing.assert_array_equal(rows, expect, err_msg=f"{variant} {layout} cap {cap}")


# ---- 8. isolation and order -----------------------------------------------------------------------
def test_two_groups_on_one_bank_and_a_loaded_set(banks, gpu):
    """Two groups on one bank, other sets and other samples, pushed alternately on a stream of their
    own with one synchronisation at the end: each gives its own rows.  The bank has one device copy,
    and the loaded set is what it was."""
    import torch

    C, T, N = 19, 480, 3
    other = ParamSet.synthetic(seed=7, C=8, T=64, N=2)
    lib.params_load(other)
    trials = sb.epochs(8, 64)[:5]
    loaded = lib.forward_ct_torch(torch.from_numpy(np.array(trials)).cuda()).cpu().numpy()
    before = (lib.device_images(), lib.image_digest(), lib.params_info())
    bank, tab, ns, x = banks(C, T, N), ss.table(C, T, N), ss.schedule(T), ss.chunks(C, T)
    sets_b = (1, 0, 3)  # sessions 0, 1, 2 under the sets their neighbours have in the first group
    expect_b = np.stack([tab[(i, s)] for i, s in enumerate(sets_b)])
    s = torch.cuda.Stream()
    with lib.Streams(bank, ss.SETS, ss.HOP, ss.MAX_PUSH) as a, lib.Streams(bank, sets_b, ss.HOP, ss.MAX_PUSH) as b:
        da, db = Driver(torch, a, x, "ct", stream=s), Driver(torch, b, x[:3], "tc", stream=s)
        torch.cuda.synchronize()  # the drivers' buffers were filled on the default stream
        for n in ns:
            da.push(n)
            db.push(n)
        rows_a, nb_a = da.rows()
        rows_b, nb_b = db.rows()
        assert nb_a == [0, 0, 0] == nb_b
        np.testing.assert_array_equal(rows_a, ss.expected(tab))
        np.testing.assert_array_equal(rows_b, expect_b)
        assert bank.device_copies() == 1
    assert (lib.device_images(), lib.image_digest(), lib.params_info()) == before
    again = lib.forward_ct_torch(torch.from_numpy(np.array(trials)).cuda()).cpu().numpy()
    np.testing.assert_array_equal(again, loaded)
    np.testing.assert_array_equal(loaded, want(other, trials))
    lib.params_unload()


# ---- 9. refusals ----------------------------------------------------------------------------------
def test_refused_pushes_leave_the_group_as_it_was(banks, gpu):
    import torch

    C, T, N = 8, 64, 2
    ns = ss.schedule(T)
    expect = ss.expected(ss.table(C, T, N))
    A = lib.load()
    with lib.Streams(banks(C, T, N), ss.SETS, ss.HOP, ss.MAX_PUSH) as st:
        d = Driver(torch, st, ss.chunks(C, T))
        half = len(ns) // 2
        d.run(ns[:half])
        assert st.windows(5) > 0
        info = st.info()
        xs = torch.zeros(4096, dtype=torch.int8, device="cuda")
        y = torch.full((4096,), GUARD, dtype=torch.int8, device="cuda")
        nb = torch.zeros(4, dtype=torch.int32, device="cuda")
        x, yp, bp, h = xs.data_ptr(), y.data_ptr(), nb.data_ptr(), st.handle
        INV = lib.NET_ERR_INVALID
        assert A.net_streams_push(None, x, 1, 5, yp, bp, None) == INV
        assert A.net_streams_push(h, None, 9, 0, None, bp + 1, None) == lib.NET_OK  # n == 0: nothing is looked at
        assert A.net_streams_push(h, x, 1, ss.MAX_PUSH + 1, yp, bp, None) == INV
        for layout in (2, -1, 7):
            assert A.net_streams_push(h, x, layout, 5, yp, bp, None) == INV
        assert A.net_streams_push(h, None, 1, 5, yp, bp, None) == INV
        assert A.net_streams_push_f32(h, x + 2, 5, yp, bp, None) == INV  # misaligned float x
        assert A.net_streams_push_f32(h, x, 5, yp, bp, None) == INV  # a bank without scales
        assert A.net_streams_push(h, x, 1, 5, None, bp, None) == INV  # k > 0
        for off in (1, 2, 3):
            assert A.net_streams_push(h, x, 1, 5, yp + off, bp, None) == INV
            assert A.net_streams_push(h, x, 1, 5, yp, bp + off, None) == INV
        # a capturing stream: refused, nothing is captured, and the capture ends cleanly
        g, s = torch.cuda.CUDAGraph(), torch.cuda.Stream()
        t = torch.zeros(8, device="cuda")
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            with torch.cuda.graph(g, stream=s):
                t += 1
                assert A.net_streams_push(h, x, 1, 5, yp, bp, s.cuda_stream) == lib.NET_ERR_UNSUPPORTED
                assert A.net_streams_restart(h, 0, 1, s.cuda_stream) == lib.NET_ERR_UNSUPPORTED
        g.replay()
        torch.cuda.synchronize()
        assert t.tolist() == [1.0] * 8
        del g
        assert st.info() == info and st.origin(0) == (0, ss.SETS[0])
        assert bool((y == GUARD).all()) and nb.tolist() == [0, 0, 0, 0]
        # the next valid pushes still give the right rows
        rows, nbad = d.run(ns[half:]).rows()
        assert nbad == [0, 0, 0]
        np.testing.assert_array_equal(rows, expect)
        # the Python entry refuses what is no tensor of the group's shape
        for bad in (None, np.zeros((ss.S, C, 4), np.int8), torch.zeros((ss.S, C, 4), dtype=torch.int8),
                    torch.zeros((ss.S + 1, C, 4), dtype=torch.int8, device="cuda"),
                    torch.zeros((ss.S, C, 4), dtype=torch.float32, device="cuda")):
            with pytest.raises(ValueError):
                st.push(bad)
        with pytest.raises(ValueError):
            st.push(torch.zeros((ss.S, C, 4), dtype=torch.int8, device="cuda"), layout="tc")
        with pytest.raises(lib.NetError):
            st.push(torch.zeros((ss.S, C, ss.MAX_PUSH + 1), dtype=torch.int8, device="cuda"))
        assert st.info()[4] == ss.total(T)


def test_python_push_returns_rows_and_counter(banks, gpu):
    """Streams.push on the tensors alone: its own logits tensor [S][k][N] and a device counter."""
    import torch

    C, T, N = 8, 64, 2
    x = torch.from_numpy(np.array(ss.chunks(C, T))).cuda()
    expect = ss.expected(ss.table(C, T, N))
    with lib.Streams(banks(C, T, N), ss.SETS, ss.HOP, ss.MAX_PUSH) as st:
        got, pos = [], 0
        for j, n in enumerate(ss.schedule(T)[:20]):
            if j % 2:
                y, nbad = st.push(x[:, :, pos: pos + n].contiguous())
            else:
                y, nbad = st.push(x[:, :, pos: pos + n].transpose(1, 2).contiguous(), layout="tc")
            assert tuple(y.shape) == (ss.S, st.info()[5] - sum(g.shape[1] for g in got), N) and int(nbad.item()) == 0
            got.append(y.cpu().numpy())
            pos += n
        rows = np.concatenate(got, axis=1)
        np.testing.assert_array_equal(rows, expect[:, : rows.shape[1]])
        assert rows.shape[1] > 50
