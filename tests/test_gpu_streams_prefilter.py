"""The IIR prefilter of a stream group on the GPU: net_streams_set_prefilter, net_streams_prefilter_info
and the hook mibminet_test_sos_filter, on uniform groups and each-groups.

The reference of a row is never another stream entry: decimate.sos_filter on the CPU over the
session's whole recording from zero state, then decimate.fir_decimate, the two-pass quantiser with
the set's scale and the C oracle on the materialised sliding windows (tests/support_prefilter.py,
whose references tests/test_prefilter_cpu.py certifies: no intermediate near the subnormals, at least
64 distinct int8 values per session).  The hook's floats are compared as uint32 bit patterns,
everything else as bytes."""
import ctypes

import numpy as np
import pytest

import support_bank as sb
import support_decim as sd
import support_decim_each as sde
import support_prefilter as pf
import support_streams as ss
from mibminet import decimate, lib
from mibminet.params import ParamSet
from support import GUARD, capped, dev, same_each, same_rows, want, windows_at  # noqa: F401 (capped: a fixture)

pytestmark = pytest.mark.gpu

SETS, S, HOP, MAX_PUSH, SCALES, M = pf.SETS, pf.S, pf.HOP, pf.MAX_PUSH, pf.SCALES, pf.M
GEOMETRIES = sb.GEOMETRIES[:2]  # (8, 64, 2) and (19, 480, 3)
QK = [(2, 7), (3, 33)]
NAN, INF = float("nan"), float("inf")
OK, INV, UNS = lib.NET_OK, lib.NET_ERR_INVALID, lib.NET_ERR_UNSUPPORTED


def bits(t):
    return np.ascontiguousarray(t.cpu().numpy() if hasattr(t, "cpu") else t).view(np.uint32)


def run_raw(torch, st, x, ns, before=None):
    """Pushes the raw frames x [S][L][C] by the list ns; before(index) runs ahead of each push.  Returns
    the rows [S][W][N] and the n_bad of every push, and checks the positions after each."""
    out, bad, P = [], [], 0
    q = st.raw_info()[0]
    for i, n in enumerate(ns):
        if before is not None:
            before(i)
        y, nbad = st.push_raw(dev(torch, np.ascontiguousarray(x[:, P: P + n])))
        P += n
        assert st.raw_info()[2:] == [P, decimate.raw_decimated(q, P)]
        out.append(y)
        bad.append(nbad)
    assert P == x.shape[1]
    return torch.cat(out, dim=1).cpu().numpy(), [int(b.item()) for b in bad]


def info_of(S_, C, m, q):
    """net_streams_prefilter_info of a group of S_ sessions of C electrodes, restated."""
    return [m, q * MAX_PUSH, (S_ * 8 * m * C + 255) // 256 * 256 + S_ * 4 * q * MAX_PUSH * C]


# ---- 1. the hook: the filtered floats and the state themselves, bit for bit -------------------------------
def test_hook_gives_sos_filter_bit_for_bit(gpu):
    import torch

    cases = 0
    for m, R, n, x, sos, state in pf.hook_cases():
        y, z = decimate.sos_filter(x, sos, state)
        gy, gz = lib.sos_filter_torch(dev(torch, x), sos, dev(torch, state))
        assert gy.shape == (n, R) and gz.shape == (m, 2, R)
        np.testing.assert_array_equal(bits(gy), bits(y), err_msg=f"M {m} R {R} n {n}")
        np.testing.assert_array_equal(bits(gz), bits(z), err_msg=f"the state, M {m} R {R} n {n}")
        if n > 1:  # the same frames in two calls, the state carried on the device
            cut = n // 3 + 1
            y1, z1 = lib.sos_filter_torch(dev(torch, x[:cut]), sos, dev(torch, state))
            y2, z2 = lib.sos_filter_torch(dev(torch, x[cut:]), sos, z1)
            np.testing.assert_array_equal(bits(torch.cat([y1, y2])), bits(y), err_msg=f"split, M {m} R {R} n {n}")
            np.testing.assert_array_equal(bits(z2), bits(z), err_msg=f"split, the state, M {m} R {R} n {n}")
        cases += 1
    assert cases == 27
    x, sos, state = next((c[3], c[4], c[5]) for c in pf.hook_cases() if c[:3] == (3, 22, 5))
    y0, z0 = lib.sos_filter_torch(dev(torch, x[:0]), sos, dev(torch, state))  # no frame: the state is handed on
    assert y0.shape == (0, 22) and np.array_equal(bits(z0), bits(state))


# ---- 2. a uniform group over the schedule -----------------------------------------------------------------
@pytest.mark.parametrize("C,T,N,q,K,cap", [g + qk + (0,) for g in GEOMETRIES for qk in QK] + [GEOMETRIES[1] + QK[1] + (1,)])
def test_raw_pushes_over_the_schedule(C, T, N, q, K, cap, capped):
    import torch

    sets, h, sos, qd, rows = pf.reference(C, T, N, q, K)
    x, ns = sd.frames(C, T, q, K), sd.schedule(T, q, K)
    pl = sd.plan(T, q, ns)
    assert any(n == 1 and m == 0 for _, n, _, m, _, _ in pl) and any(n == q * MAX_PUSH for _, n, _, _, _, _ in pl)
    assert any(n < q for _, n, *_ in pl) and any(all(n < K - 1 for _, n, _, _, _, _ in pl[i: i + 3]) for i in range(len(pl) - 2))
    capped(cap)
    with lib.Bank(sets, SCALES) as bank, lib.Streams(bank, SETS, HOP, MAX_PUSH) as st:
        st.decimate(q, h)
        assert st.prefilter_info() == [0, 0, 0]
        given = st.prefilter(sos)
        assert given.dtype == np.float32 and np.array_equal(given, sos) and st.prefilter_info() == info_of(S, C, M, q)
        got, bad = run_raw(torch, st, x, ns)
        assert not any(bad) and got.shape[1] == sum(k for *_, k, _ in pl) == st.info()[5]
        for i in range(S):
            same_rows(got[i], rows[i][: got.shape[1]], f"session {i}")
        assert st.info()[4] >= 2 * st.cap + 16
        sd.check_rings(st, sets, qd)


# ---- 3. the identity section ------------------------------------------------------------------------------
def test_identity_section_gives_the_group_without_a_prefilter(gpu):
    """sos = [[1, 0, 0, 0, 0]] (and scipy's six-column form of it, with a0 = 2): the rows and rings of
    the same group without a prefilter."""
    import torch

    (C, T, N), (q, K) = GEOMETRIES[0], QK[0]
    sets, h = sb.sets(C, T, N), sd.taps(K, 11)
    x, ns = sd.frames(C, T, q, K), sd.schedule(T, q, K)
    with lib.Bank(sets, sd.SCALES) as bank, lib.Streams(bank, SETS, HOP, MAX_PUSH) as st, \
            lib.Streams(bank, SETS, HOP, MAX_PUSH) as six, lib.Streams(bank, SETS, HOP, MAX_PUSH) as sib:
        for g in (st, six, sib):
            g.decimate(q, h)
        assert np.array_equal(st.prefilter(pf.IDENTITY), pf.IDENTITY)
        assert np.array_equal(six.prefilter([[2, 0, 0, 2, 0, 0]]), pf.IDENTITY)
        assert st.prefilter_info() == info_of(S, C, 1, q) and sib.prefilter_info() == [0, 0, 0]
        got, bad = run_raw(torch, st, x, ns)
        got6, _ = run_raw(torch, six, x, ns)
        plain, _ = run_raw(torch, sib, x, ns)
        assert not any(bad) and np.array_equal(got, plain) and np.array_equal(got6, plain) and got.shape[1] > 20
        for i in range(S):
            np.testing.assert_array_equal(lib.streams_ring(st, i), lib.streams_ring(sib, i))
            np.testing.assert_array_equal(lib.streams_ring(six, i), lib.streams_ring(sib, i))


# ---- 4. an each-group: ragged counts, refused counts, a captured graph ------------------------------------
def test_each_group_with_ragged_and_refused_counts(gpu):
    """Counts of 0 and single frames, and in six ticks a count of -1, n_raw_max + 1 or INT32_MIN: cnt_out
    is -1 (RawDriver), n_bad rises by one each, and the session's later rows, so its states and its
    history, go on as if the tick had not happened."""
    import torch

    c = pf.each_case()
    sets = sb.sets(c.C, c.T, c.N)
    ref = [pf.session_reference(sets[s], SCALES[s], c.x[i][: int(c.fed[i])], c.sos, c.h, c.q, c.T) for i, s in enumerate(SETS)]
    with lib.Bank(sets, SCALES) as bank, lib.StreamsEach(bank, SETS, HOP, MAX_PUSH) as st:
        st.decimate(c.q, c.h)
        st.prefilter(c.sos)
        assert st.prefilter_info() == info_of(S, c.C, M, c.q)
        d = sde.RawDriver(torch, st, c.x, c.q, c.K)
        for t in range(len(c.n_max)):
            d.push(c.n_max[t], [int(v) for v in c.counts[t]])  # holds cnt_out, win0 and both positions to the plan
        got, nb = d.result()
        assert nb == [0, len(c.bad), 0] and d.P == c.fed.tolist()
        same_each(got, [r[1] for r in ref])
        sd.check_rings(st, sets, [r[0] for r in ref])


def test_each_group_replayed_from_a_captured_graph(gpu):
    """One eager raw push, then the same enqueue captured on one stream and replayed for the rest of
    the ragged schedule with the frames and the counts rewritten in place: the coefficients travel in
    the captured kernel's arguments, the trip counts come from the plan's records."""
    import torch

    c = pf.each_case()
    sets, w = sb.sets(c.C, c.T, c.N), sde.walk(c.T, c.q, c.K)
    rows = [pf.session_reference(sets[s], SCALES[s], c.x[i][: int(c.fed_good[i])], c.sos, c.h, c.q, c.T)[1]
            for i, s in enumerate(SETS)]
    counts, n_max = c.good, c.n_max
    top = c.q * MAX_PUSH
    kmax = sde.each_raw_rows(HOP, c.q, top)
    A = lib.load()
    with lib.Bank(sets, SCALES) as bank, lib.StreamsEach(bank, SETS, HOP, MAX_PUSH) as st:
        st.decimate(c.q, c.h)
        st.prefilter(c.sos)
        xs = torch.zeros((S, top, c.C), dtype=torch.float32, device="cuda")
        cin = torch.zeros((S,), dtype=torch.int32, device="cuda")
        y = torch.full((S, kmax, c.N), GUARD, dtype=torch.int8, device="cuda")
        cout = torch.zeros((S,), dtype=torch.int32, device="cuda")
        win0 = torch.zeros((S,), dtype=torch.int64, device="cuda")
        nb = torch.zeros((3,), dtype=torch.int32, device="cuda")
        s = torch.cuda.Stream()
        args = (st.handle, xs.data_ptr(), cin.data_ptr(), top, y.data_ptr(), cout.data_ptr(), win0.data_ptr(), nb.data_ptr() + 4)
        cur, got = [0] * S, [[] for _ in range(S)]

        def load(t):
            slot = np.full((S, top, c.C), np.nan, np.float32)
            for i in range(S):
                slot[i, : counts[t, i]] = c.x[i, cur[i]: cur[i] + counts[t, i]]
            xs.copy_(torch.from_numpy(slot))
            cin.copy_(torch.from_numpy(np.array(counts[t])))
            y.fill_(GUARD)

        def collect(t):
            torch.cuda.synchronize()
            yh, ch = y.cpu().numpy(), cout.tolist()
            assert ch == w.k[t].tolist() and win0.tolist() == w.W0[t].tolist(), t
            for i in range(S):
                got[i].append(yh[i, : ch[i]])
                assert (yh[i, ch[i]:] == GUARD).all(), (t, i)
                cur[i] += int(counts[t, i])

        load(0)
        torch.cuda.synchronize()
        assert A.net_streams_push_each_raw_f32_tm(*args, s.cuda_stream) == OK  # eager
        collect(0)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(s):
            with torch.cuda.graph(g, stream=s):
                assert A.net_streams_push_each_raw_f32_tm(*args, s.cuda_stream) == OK
        torch.cuda.synchronize()
        assert st.raw_positions().tolist() == w.P[1].tolist()  # the capture ran nothing
        for t in range(1, len(n_max)):
            load(t)
            g.replay()
            collect(t)
        del g
        assert nb.tolist() == [0, 0, 0] and st.raw_positions().tolist() == w.fed.tolist() == cur
        assert st.positions().tolist() == [decimate.raw_decimated(c.q, int(p)) for p in w.fed]
        same_each([np.concatenate(p) for p in got], rows)


# ---- 5. a restart -----------------------------------------------------------------------------------------
def test_restart_zeroes_the_states(gpu):
    """Session RESTART[0] restarts under set RESTART[1] ahead of a push at a raw position off the grid:
    its later rows are those of a session whose earlier frames were all zero (zero history, zero
    states), the windows that start before its origin are zero rows counted in n_bad, the other
    sessions are untouched."""
    import torch

    c = pf.restart_case()
    sets, h, sos, qd, rows = pf.reference(c.C, c.T, c.N, c.q, c.K)
    x, origin = sd.frames(c.C, c.T, c.q, c.K), c.pl[c.at][2]
    zeroed, scale, _, _ = c.sessions[0]
    rows_r = pf.session_reference(sets[c.s_r], scale, zeroed, sos, h, c.q, c.T)[1]
    with lib.Bank(sets, SCALES) as bank, lib.Streams(bank, SETS, HOP, MAX_PUSH) as st:
        st.decimate(c.q, h)
        st.prefilter(sos)
        got, bad = run_raw(torch, st, x, c.ns, before=lambda i: st.restart(c.i_r, c.s_r) if i == c.at else None)
        assert st.origin(c.i_r) == (origin, c.s_r)
        W = got.shape[1]
        for i in range(S):
            if i != c.i_r:
                same_rows(got[i], rows[i][:W], f"session {i}")
        expect, w, want_bad = np.array(rows[c.i_r][:W]), 0, []
        for j, (_, _, _, _, k, onsets) in enumerate(c.pl):
            n_bad = 0
            for o in onsets:
                if j >= c.at:
                    expect[w] = rows_r[w] if o >= origin else 0
                    n_bad += o < origin
                w += 1
            want_bad.append(n_bad)
        assert w == W and sum(want_bad) > 0 and bad == want_bad
        same_rows(got[c.i_r], expect, "the restarted session")
        sd.check_rings(st, sets, qd, skip=(c.i_r,))


# ---- 6. a widened montage ---------------------------------------------------------------------------------
def test_widened_montage_with_non_finite_unselected_electrodes(gpu):
    """19 x 480 sets widened to 64 rows: the unselected electrodes carry NaN and the infinities in every
    chunk, so in their states from then on; the rows are the oracle's under the ORIGINAL sets on the
    selected electrodes."""
    import torch

    c = pf.montage_case()
    orig = tuple(ParamSet.synthetic(seed=331 + i, C=19, T=c.T, N=c.N) for i in range(3))
    expect = [pf.session_reference(ps, pf.MONTAGE_SCALES[i], c.sessions[i][0], c.sos, c.h, c.q, c.T)[1]
              for i, ps in enumerate(orig)]
    wide = [ps.widened(c.R, c.maps[i]) for i, ps in enumerate(orig)]
    with lib.Bank(wide, pf.MONTAGE_SCALES) as bank, lib.Streams(bank, (0, 1, 2), HOP, MAX_PUSH) as st:
        st.decimate(c.q, c.h)
        st.prefilter(c.sos)
        got, bad = run_raw(torch, st, c.x, c.ns)
        assert not any(bad)
        for i in range(3):
            same_rows(got[i], expect[i][: got.shape[1]], f"session {i}")


# ---- 7. refusals ------------------------------------------------------------------------------------------
def test_refusals_leave_the_group_unchanged(gpu):
    import torch

    (C, T, N), (q, K) = GEOMETRIES[0], QK[0]
    sets, h, _, rows = sd.reference(C, T, N, q, K)
    x, ns = sd.frames(C, T, q, K), sd.schedule(T, q, K)
    sos = np.array(pf.sections(M, pf.SEED))
    A = lib.load()
    setter = A.net_streams_set_prefilter

    def ptr(a):
        return a.ctypes.data_as(ctypes.c_void_p)

    def with_at(j, v):
        out = sos.copy()
        out.reshape(-1)[j] = v
        return out

    with lib.Bank(sets, sd.SCALES) as bank:
        with lib.Streams(bank, SETS, HOP, MAX_PUSH) as st, lib.StreamsEach(bank, SETS, HOP, MAX_PUSH) as ea, \
                lib.Streams(bank, SETS, HOP, MAX_PUSH) as nodec, lib.Streams(bank, SETS, HOP, MAX_PUSH) as twice:
            assert setter(None, ptr(sos), M, None) == INV
            assert setter(nodec.handle, ptr(sos), M, None) == INV  # before a decimator
            for g in (st, ea, twice):
                g.decimate(q, h)
            for g in (st, ea):
                for m in (0, 9, 2**40):
                    assert setter(g.handle, ptr(np.resize(sos, (9, 5))), m, None) == INV, m
                assert setter(g.handle, None, M, None) == INV
                for j, v in ((0, NAN), (7, INF), (14, -INF), (4, NAN)):
                    assert setter(g.handle, ptr(with_at(j, v)), M, None) == INV, (j, v)
            # a capturing stream, after every other check
            gr, s = torch.cuda.CUDAGraph(), torch.cuda.Stream()
            t = torch.zeros(8, device="cuda")
            torch.cuda.synchronize()
            with torch.cuda.stream(s):
                with torch.cuda.graph(gr, stream=s):
                    t += 1
                    for g in (st, ea):
                        assert setter(g.handle, ptr(sos), 0, s.cuda_stream) == INV
                        assert setter(g.handle, ptr(sos), M, s.cuda_stream) == UNS
            del gr
            torch.cuda.synchronize()
            # set twice
            twice.prefilter(sos)
            assert setter(twice.handle, ptr(sos), M, None) == INV and setter(twice.handle, ptr(pf.IDENTITY), 1, None) == INV
            assert twice.prefilter_info() == info_of(S, C, M, q)
            # after every refusal: no prefilter, and the rows of the decimator alone
            for g in (st, ea, nodec):
                assert g.prefilter_info() == [0, 0, 0]
            got, bad = run_raw(torch, st, x, ns)
            assert not any(bad)
            for i in range(S):
                same_rows(got[i], rows[i][: got.shape[1]], f"session {i}")
            # set after a push, on either kind of group
            full = torch.full((S,), 4, dtype=torch.int32, device="cuda")
            ea.push_raw(dev(torch, np.ascontiguousarray(x[:, :4])), full)
            for g in (st, ea):
                assert setter(g.handle, ptr(sos), M, None) == INV and g.prefilter_info() == [0, 0, 0]
            info = (ctypes.c_int64 * 3)()
            assert A.net_streams_prefilter_info(None, info) == INV and A.net_streams_prefilter_info(st.handle, None) == INV
            for bad_sos in (sos[:, :4], sos[0], np.zeros((2, 7), np.float32)):
                with pytest.raises(ValueError):
                    twice.prefilter(bad_sos)


# ---- 8. windows at given onsets after a prefiltered push --------------------------------------------------
def test_windows_at_after_a_prefiltered_push(gpu):
    import torch

    (C, T, N), (q, K) = GEOMETRIES[0], QK[0]
    sets, h, sos, qd, _ = pf.reference(C, T, N, q, K)
    x, ns = sd.frames(C, T, q, K), sd.schedule(T, q, K)
    with lib.Bank(sets, SCALES) as bank, lib.Streams(bank, SETS, HOP, MAX_PUSH) as st:
        st.decimate(q, h)
        st.prefilter(sos)
        run_raw(torch, st, x, ns)
        lo, hi = st.at_span()
        assert (lo, hi) == (st.info()[4] - st.cap, st.info()[4] - T) and lo > 0
        cues = [q * lo, q * lo + 1, q * (lo + 7) - 1, q * hi - 3, q * hi]  # raw frames: on and off the grid
        onsets = [decimate.raw_decimated(q, a) for a in cues]
        assert all(lo <= o <= hi for o in onsets)
        sessions = [0, 1, 2, 3, 4]
        got = st.windows_at(sessions, onsets).cpu().numpy()
        for w, (i, o) in enumerate(zip(sessions, onsets)):
            np.testing.assert_array_equal(got[w], want(sets[SETS[i]], windows_at(qd[i], [o], T))[0], err_msg=f"item {w}")
