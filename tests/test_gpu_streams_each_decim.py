"""Raw frames at each session's own pace on the GPU: net_streams_set_decimator_each,
net_streams_push_each_raw_f32_tm and net_streams_raw_positions.

The five sessions of support_decim under sets (0, 1, 1, 3, 0), each fed a prefix of its own raw frames
by the ragged count schedule of support_decim_each (certified in tests/test_decim_each_cpu.py and
again here).  The reference of a row is never another stream entry: decimate.fir_decimate on the CPU
over the session's concatenated chunks, then the two-pass quantiser with the set's scale, then the C
oracle on the materialised sliding windows.  Every comparison is byte-exact; cnt_out, win0 and both
kinds of position are held to the restatement of the plan after every push (RawDriver)."""
import ctypes

import numpy as np
import pytest

import support_bank as sb
import support_decim as sd
import support_decim_each as sde
import support_streams as ss
from mibminet import decimate, lib
from mibminet.params import ParamSet
from support import GUARD, capped, same_each, want, windows_at  # noqa: F401 (capped: a fixture)

pytestmark = pytest.mark.gpu

SETS, S, HOP, MAX_PUSH, SCALES = sd.SETS, sd.S, sd.HOP, sd.MAX_PUSH, sd.SCALES
GEOMETRIES = sb.GEOMETRIES[:2]  # (8, 64, 2) and (19, 480, 3)
QK = [(2, 7), (3, 33)]
NAN, INF = float("nan"), float("inf")
OK, INV, UNS = lib.NET_OK, lib.NET_ERR_INVALID, lib.NET_ERR_UNSUPPORTED
INT32_MIN = -2**31


def D(q, P):
    return decimate.raw_decimated(q, P)


# ---- 1. the ragged schedule -------------------------------------------------------------------------------
@pytest.mark.parametrize("C,T,N,q,K,cap", [g + qk + (0,) for g in GEOMETRIES for qk in QK]
                         + [GEOMETRIES[0] + (16, 128, 0), GEOMETRIES[1] + QK[1] + (1,)])
def test_ragged_schedule(C, T, N, q, K, cap, capped):
    import torch

    sets, h, qd, rows = sde.reference(C, T, N, q, K)
    w = sde.certify(T, q, K)
    n_max, counts = sde.schedule(T, q, K)
    capped(cap)
    with lib.Bank(sets, SCALES) as bank, lib.StreamsEach(bank, SETS, HOP, MAX_PUSH) as st:
        assert st.raw_info() == [0, 0, 0, 0]
        st.decimate(q, h)
        assert st.raw_info() == [q, K, -1, -1] and st.raw_positions().tolist() == [0] * S
        d = sde.RawDriver(torch, st, sde.frames(C, T, q, K), q, K).run(n_max, counts)
        got, nb = d.result()
        assert nb == [0, 0, 0] and d.P == w.fed.tolist() and st.info()[4:] == [len(n_max), -1]
        same_each(got, rows)
        assert min(D(q, p) for p in d.P) >= 2 * st.cap + 16
        sd.check_rings(st, sets, qd)


# ---- 2. refused counts ------------------------------------------------------------------------------------
def test_refused_counts_move_nothing(gpu):
    """In chosen ticks one session's count is -1, n_raw_max + 1 or INT32_MIN: cnt_out is -1 (RawDriver),
    n_bad rises by one, the session's ring and both its positions stay, and its later rows, so its
    history, go on as if the tick had not happened."""
    import torch

    (C, T, N), (q, K) = GEOMETRIES[0], QK[0]
    sets, h = sb.sets(C, T, N), sd.taps(K, 11)
    n_max, counts = sde.schedule(T, q, K)
    counts = np.array(counts, np.int64)
    ticks = len(n_max)
    bad = {(3, 1): -1, (7, 3): n_max[7] + 1, (ticks // 3, 0): INT32_MIN, (ticks // 2, 4): -1, (ticks // 2 + 1, 4): n_max[ticks // 2 + 1] + 1,
           (ticks - 2, 2): INT32_MIN}
    fed = counts.sum(axis=0)
    for (t, s), v in bad.items():
        fed[s] -= counts[t, s]
        counts[t, s] = v
    x = sde.frames(C, T, q, K)
    ref = [sd.session_reference(sets[s], SCALES[s], x[i][: int(fed[i])], h, q, T) for i, s in enumerate(SETS)]
    with lib.Bank(sets, SCALES) as bank, lib.StreamsEach(bank, SETS, HOP, MAX_PUSH) as st:
        st.decimate(q, h)
        d = sde.RawDriver(torch, st, x, q, K)
        for t in range(ticks):
            who = [s for s in range(S) if (t, s) in bad]
            before = [lib.streams_ring(st, s).tobytes() for s in who]
            d.push(n_max[t], [int(c) for c in counts[t]])  # holds both positions to the restatement
            assert [lib.streams_ring(st, s).tobytes() for s in who] == before, t
        got, nb = d.result()
        assert nb == [0, len(bad), 0] and d.P == fed.tolist()
        same_each(got, [r[1] for r in ref])
        sd.check_rings(st, sets, [r[0] for r in ref])


# ---- 3. identity and stride -------------------------------------------------------------------------------
@pytest.mark.parametrize("q", [1, 3])
def test_identity_and_stride(q, gpu):
    """h = [1]: q = 1 gives the bytes of push_f32(layout="tc") on a sibling each-group with the same
    slots and counts, rows, cnt_out and rings; q = 3 is each session's x[::3] on its own axis."""
    import torch

    C, T, N = GEOMETRIES[0]
    sets = sb.sets(C, T, N)
    n_max, counts = sde.schedule(T, q, 1)
    fed = sde.walk(T, q, 1).fed
    x = sd.inputs(np.random.default_rng([C, T, q, 43]), (S, int(fed.max()), C)) * np.float32(0.5)
    one = np.ones(1, np.float32)
    qd = [sd.two_pass(x[i][: int(fed[i])][::q], SCALES[s]) for i, s in enumerate(SETS)]
    with lib.Bank(sets, SCALES) as bank, lib.StreamsEach(bank, SETS, HOP, MAX_PUSH) as st, \
            lib.StreamsEach(bank, SETS, HOP, MAX_PUSH) as sib:
        st.decimate(q, one)
        d = sde.RawDriver(torch, st, x, q, 1)
        got = [[] for _ in range(S)]
        for t, m in enumerate(n_max):
            row = [int(c) for c in counts[t]]
            xs, cin = d.slots(m, row), torch.tensor(row, dtype=torch.int32, device="cuda")
            y, cout, nbad = st.push_raw(xs, cin)  # the Python entry
            assert tuple(y.shape) == (S, sde.each_raw_rows(HOP, q, m), N) and int(nbad.item()) == 0
            if q == 1:
                y2, cout2, _ = sib.push_f32(xs, cin, layout="tc")
                assert cout.tolist() == cout2.tolist()
                for i, k in enumerate(cout.tolist()):
                    assert torch.equal(y[i, :k], y2[i, :k]), (t, i)
            for i, k in enumerate(cout.tolist()):
                got[i].append(y[i, :k].cpu().numpy())
                d.cur[i] += row[i]
        assert st.raw_positions().tolist() == fed.tolist() and st.positions().tolist() == [D(q, int(p)) for p in fed]
        same_each([np.concatenate(g) for g in got], [ss.rows_of(sets[s], qd[i], T) for i, s in enumerate(SETS)])
        sd.check_rings(st, sets, qd)
        if q == 1:
            assert sib.positions().tolist() == fed.tolist()
            for i in range(S):
                np.testing.assert_array_equal(lib.streams_ring(st, i), lib.streams_ring(sib, i))


# ---- 4. equal counts equal the uniform group --------------------------------------------------------------
@pytest.mark.parametrize("q,K", QK)
def test_equal_counts_give_the_uniform_raw_push(q, K, gpu):
    """Every count n = n_raw_max over support_decim.schedule: the rows and rings of Streams.push_raw on
    the same frames, from position 0."""
    import torch

    C, T, N = GEOMETRIES[0]
    sets, h, _, _ = sd.reference(C, T, N, q, K)
    x, ns = sd.frames(C, T, q, K), sd.schedule(T, q, K)
    with lib.Bank(sets, SCALES) as bank, lib.StreamsEach(bank, SETS, HOP, MAX_PUSH) as st, \
            lib.Streams(bank, SETS, HOP, MAX_PUSH) as uni:
        st.decimate(q, h)
        uni.decimate(q, h)
        P = 0
        for n in ns:
            xs = torch.from_numpy(np.ascontiguousarray(x[:, P: P + n])).cuda()
            y, cout, nbad = st.push_raw(xs, torch.full((S,), n, dtype=torch.int32, device="cuda"))
            yu, _ = uni.push_raw(xs)
            k = int(yu.shape[1])
            assert cout.tolist() == [k] * S and int(nbad.item()) == 0 and torch.equal(y[:, :k], yu), P
            P += n
        assert st.raw_positions().tolist() == [P] * S == [uni.raw_info()[2]] * S
        for i in range(S):
            np.testing.assert_array_equal(lib.streams_ring(st, i), lib.streams_ring(uni, i))


# ---- 5. a widened montage ---------------------------------------------------------------------------------
def test_widened_montage_with_non_finite_unselected_electrodes(gpu):
    """19 x 480 sets widened to 64 rows (R > 32): the unselected electrodes carry NaN and the infinities,
    in the chunks and so in the histories; the rows are the oracle's under the ORIGINAL sets."""
    import torch

    T, N, R, q, K = 480, 3, 64, 2, 7
    orig = tuple(ParamSet.synthetic(seed=331 + i, C=19, T=T, N=N) for i in range(3))
    maps = [[int(c) for c in np.random.default_rng([R, 50 + i]).permutation(R)[:19]] for i in range(3)]
    h = sd.taps(K, 12)
    n_max, counts = sde.schedule(T, q, K)
    counts = counts[:, :3]
    fed = counts.sum(axis=0)
    rng = np.random.default_rng([R, T, 19])
    x = sd.inputs(rng, (3, int(fed.max()), R))
    expect = []
    for i, ps in enumerate(orig):
        keep = x[i][:, maps[i]].copy()
        junk = rng.random(x[i].shape)
        x[i][junk < 0.1] = NAN
        x[i][(junk >= 0.1) & (junk < 0.2)] = -INF
        x[i][(junk >= 0.2) & (junk < 0.3)] = INF
        x[i][:, maps[i]] = keep
        expect.append(sd.session_reference(ps, SCALES[i], keep[: int(fed[i])], h, q, T)[1])
    wide = [ps.widened(R, maps[i]) for i, ps in enumerate(orig)]
    with lib.Bank(wide, SCALES[:3]) as bank, lib.StreamsEach(bank, (0, 1, 2), HOP, MAX_PUSH) as st:
        st.decimate(q, h)
        got, nb = sde.RawDriver(torch, st, x, q, K).run(n_max, counts).result()
        assert nb == [0, 0, 0]
        same_each(got, expect)


# ---- 6. a restart -----------------------------------------------------------------------------------------
def test_restart_makes_a_fresh_session(gpu):
    """Session RESTART[0] restarts under set RESTART[1] at a raw position off the grid and off slot 0:
    its later rows are those of a fresh session under the new set fed the frames after the restart,
    both its positions start at 0 again, and the other sessions are unaffected."""
    import torch

    (C, T, N), (q, K) = GEOMETRIES[0], QK[1]
    sets, h, qd, rows = sde.reference(C, T, N, q, K)
    n_max, counts = sde.schedule(T, q, K)
    w, x = sde.walk(T, q, K), sde.frames(C, T, q, K)
    i_r, s_r = ss.RESTART
    at = next(t for t in range(len(n_max)) if w.P[t, i_r] % q and w.P[t, i_r] % (K - 1) and D(q, int(w.P[t, i_r])) > T + 20)
    P_r, fed = int(w.P[at, i_r]), int(w.fed[i_r])
    qd_r, rows_r = sd.session_reference(sets[s_r], SCALES[s_r], x[i_r][P_r:fed], h, q, T)
    before = rows[i_r][: ss.windows_count(T, D(q, P_r), HOP)]
    assert len(before) > 0 and len(rows_r) > 5
    with lib.Bank(sets, SCALES) as bank, lib.StreamsEach(bank, SETS, HOP, MAX_PUSH) as st:
        st.decimate(q, h)
        d = sde.RawDriver(torch, st, x, q, K).run(n_max[:at], counts[:at])
        st.restart(i_r, s_r)
        d.restarted(i_r)
        want_P = [0 if i == i_r else int(v) for i, v in enumerate(w.P[at])]
        assert st.raw_positions().tolist() == want_P and st.positions().tolist() == [D(q, p) for p in want_P]
        assert st.origin(i_r) == (-1, s_r) and st.raw_info() == [q, K, -1, -1]
        got, nb = d.run(n_max[at:], counts[at:]).result()
        assert nb == [0, 0, 0] and d.P[i_r] == fed - P_r
        same_each(got, [np.concatenate([before, rows_r]) if i == i_r else rows[i] for i in range(S)])
        set_of, qd2 = list(SETS), list(qd)
        set_of[i_r], qd2[i_r] = s_r, qd_r
        sd.check_rings(st, sets, qd2, set_of=set_of)
        # a capturing stream is refused, and nothing moves
        g, s = torch.cuda.CUDAGraph(), torch.cuda.Stream()
        t = torch.zeros(8, device="cuda")
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            with torch.cuda.graph(g, stream=s):
                t += 1
                assert lib.load().net_streams_restart(st.handle, 0, 1, s.cuda_stream) == UNS
        del g
        torch.cuda.synchronize()
        assert st.raw_positions().tolist() == d.P and st.origin(0) == (-1, SETS[0])


# ---- 7. windows at cues given in raw frames ---------------------------------------------------------------
def test_windows_at_after_a_raw_push(gpu):
    import torch

    (C, T, N), (q, K) = GEOMETRIES[0], QK[0]
    sets, h, qd, _ = sde.reference(C, T, N, q, K)
    n_max, counts = sde.schedule(T, q, K)
    with lib.Bank(sets, SCALES) as bank, lib.StreamsEach(bank, SETS, HOP, MAX_PUSH) as st:
        st.decimate(q, h)
        d = sde.RawDriver(torch, st, sde.frames(C, T, q, K), q, K).run(n_max, counts)
        pos = st.positions().tolist()
        assert len(set(pos)) > 1
        # raw frames on and off the grid, the oldest and the newest window of a session among them
        cues = [(0, q * (pos[0] - T)), (1, q * (pos[1] - T) - 1), (2, q * (pos[2] - st.cap) + 1), (3, q * (pos[3] - st.cap + 9) - 1),
                (4, q * (pos[4] - T - 5)), (1, q * (pos[1] - st.cap))]
        sessions, onsets = [i for i, _ in cues], [D(q, a) for _, a in cues]
        assert all(pos[i] - st.cap <= o <= pos[i] - T for i, o in zip(sessions, onsets))
        assert all(a <= d.P[i] for i, a in cues) and any(a % q for _, a in cues)
        got = st.windows_at(sessions, onsets).cpu().numpy()
        for j, (i, o) in enumerate(zip(sessions, onsets)):
            np.testing.assert_array_equal(got[j], want(sets[SETS[i]], windows_at(qd[i], [o], T))[0], err_msg=f"item {j}")


# ---- 8. a captured graph ----------------------------------------------------------------------------------
def test_raw_push_replayed_from_a_captured_graph(gpu):
    """One eager raw push, then the push captured on one stream and replayed for the rest of the ragged
    schedule with x and the counts rewritten in place: the rows are the reference's, which the eager
    run gives (test 1), and the positions the totals."""
    import torch

    (C, T, N), (q, K) = GEOMETRIES[0], QK[1]
    sets, h, _, rows = sde.reference(C, T, N, q, K)
    n_max, counts = sde.schedule(T, q, K)
    w, x = sde.walk(T, q, K), sde.frames(C, T, q, K)
    M = q * MAX_PUSH
    kmax = sde.each_raw_rows(HOP, q, M)
    A = lib.load()
    with lib.Bank(sets, SCALES) as bank, lib.StreamsEach(bank, SETS, HOP, MAX_PUSH) as st:
        st.decimate(q, h)
        xs = torch.zeros((S, M, C), dtype=torch.float32, device="cuda")
        cin = torch.zeros((S,), dtype=torch.int32, device="cuda")
        y = torch.full((S, kmax, N), GUARD, dtype=torch.int8, device="cuda")
        cout = torch.zeros((S,), dtype=torch.int32, device="cuda")
        win0 = torch.zeros((S,), dtype=torch.int64, device="cuda")
        nb = torch.zeros((3,), dtype=torch.int32, device="cuda")
        s = torch.cuda.Stream()
        args = (st.handle, xs.data_ptr(), cin.data_ptr(), M, y.data_ptr(), cout.data_ptr(), win0.data_ptr(), nb.data_ptr() + 4)
        cur, got = [0] * S, [[] for _ in range(S)]

        def load(t):
            slot = np.full((S, M, C), np.nan, np.float32)
            for i in range(S):
                slot[i, : counts[t, i]] = x[i, cur[i]: cur[i] + counts[t, i]]
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
        assert st.positions().tolist() == [D(q, int(p)) for p in w.fed] and st.info()[4] == 2  # enqueues, not replays
        same_each([np.concatenate(p) for p in got], rows)


# ---- 9. refusals ------------------------------------------------------------------------------------------
def test_refusals_leave_the_groups_unchanged(gpu):
    import torch

    (C, T, N), (q, K) = GEOMETRIES[0], QK[0]
    sets, h = sb.sets(C, T, N), sd.taps(K, 11)
    A = lib.load()
    M = q * MAX_PUSH
    x = torch.from_numpy(sd.inputs(np.random.default_rng(6), (S, M + 1, C))).cuda()
    y = torch.full((S, MAX_PUSH, N), GUARD, dtype=torch.int8, device="cuda")
    cin = torch.full((8,), 5, dtype=torch.int32, device="cuda")
    cout = torch.full((8,), -7, dtype=torch.int32, device="cuda")
    w0 = torch.full((8,), -7, dtype=torch.int64, device="cuda")
    nb = torch.zeros((4,), dtype=torch.int32, device="cuda")
    xp, ci, yp, co, wp, bp = x.data_ptr(), cin.data_ptr(), y.data_ptr(), cout.data_ptr(), w0.data_ptr(), nb.data_ptr()
    setter, push, rawpos = A.net_streams_set_decimator_each, A.net_streams_push_each_raw_f32_tm, A.net_streams_raw_positions

    def taps_ptr(a):
        return a.ctypes.data_as(ctypes.c_void_p)

    def state(*groups):
        torch.cuda.synchronize()
        return [(g.raw_info(), g.info(), g.positions().tolist() if isinstance(g, lib.StreamsEach) else None,
                 g.raw_positions().tolist() if isinstance(g, lib.StreamsEach) and g.raw_info()[0] else None,
                 [lib.streams_ring(g, i).tobytes() for i in range(S)]) for g in groups]

    with lib.Bank(sets, SCALES) as bank, lib.Bank(sets) as bare:
        with lib.StreamsEach(bank, SETS, HOP, MAX_PUSH) as st, lib.StreamsEach(bank, SETS, HOP, MAX_PUSH) as plain, \
                lib.Streams(bank, SETS, HOP, MAX_PUSH) as uni, lib.StreamsEach(bare, SETS, HOP, MAX_PUSH) as nos:
            # the setter: the kind of group, then the limits, the taps, the bank
            nan = h.copy()
            nan[3] = NAN
            before = state(st, nos, uni)
            assert setter(None, q, taps_ptr(h), K, None) == INV
            assert setter(uni.handle, q, taps_ptr(h), K, None) == INV
            assert setter(uni.handle, 0, None, 0, None) == INV
            for qq, taps, KK in ((0, h, K), (17, h, K), (q, h, 0), (q, np.resize(h, 129), 129), (q, nan, K)):
                assert setter(st.handle, qq, taps_ptr(taps), KK, None) == INV, (qq, KK)
            assert setter(st.handle, q, None, K, None) == INV
            assert setter(nos.handle, q, taps_ptr(h), K, None) == INV
            assert A.net_streams_set_decimator(st.handle, q, taps_ptr(h), K, None) == UNS  # as before
            assert state(st, nos, uni) == before
            # an each-group without a decimator: no raw push, no raw positions; a decimator after a push
            assert push(plain.handle, xp, ci, 5, yp, co, wp, bp, None) == INV
            assert rawpos(plain.handle, wp, None) == INV
            plain.push_f32(x[:, :5].contiguous(), cin[:S].contiguous(), layout="tc")
            before = state(plain)
            assert setter(plain.handle, q, taps_ptr(h), K, None) == INV
            assert state(plain) == before
            # a capturing stream, after every other check
            g, s = torch.cuda.CUDAGraph(), torch.cuda.Stream()
            t = torch.zeros(8, device="cuda")
            torch.cuda.synchronize()
            with torch.cuda.stream(s):
                with torch.cuda.graph(g, stream=s):
                    t += 1
                    assert setter(st.handle, 0, taps_ptr(h), K, s.cuda_stream) == INV
                    assert setter(st.handle, q, taps_ptr(h), K, s.cuda_stream) == UNS
            del g
            assert st.raw_info() == [0, 0, 0, 0]
            st.decimate(q, h)
            uni.decimate(q, h)
            full = torch.full((S,), M, dtype=torch.int32, device="cuda")
            for _ in range(2):
                st.push_raw(x[:, :M].contiguous(), full)
            assert st.positions().tolist() == [2 * MAX_PUSH] * S
            before = state(st, uni)
            assert setter(st.handle, q, taps_ptr(h), K, None) == INV  # a second decimator
            # the plain entries on a decimating each-group, each kind of group against the other's entries
            assert A.net_streams_push_each_f32_tm(st.handle, xp, ci, 5, yp, co, wp, bp, None) == INV
            assert A.net_streams_push_each_f32(st.handle, xp, ci, 5, yp, co, wp, bp, None) == INV
            assert A.net_streams_push_each(st.handle, xp, 0, ci, 5, yp, co, wp, bp, None) == INV
            assert A.net_streams_push_raw_f32_tm(st.handle, xp, 5, yp, bp, None) == INV
            assert push(uni.handle, xp, ci, 5, yp, co, wp, bp, None) == INV
            assert rawpos(uni.handle, wp, None) == INV
            assert push(None, xp, ci, 5, yp, co, wp, bp, None) == INV
            # the raw push's own checks, in order: n_raw_max, the pointers, the alignments
            for n in (0, M + 1, 2**40):
                assert push(st.handle, xp, ci, n, yp, co, wp, bp, None) == INV
            assert push(st.handle, None, ci, 5, yp, co, wp, bp, None) == INV
            assert push(st.handle, xp, None, 5, yp, co, wp, bp, None) == INV
            assert push(st.handle, xp, ci, 5, None, co, wp, bp, None) == INV
            assert push(st.handle, xp, ci, 5, yp, None, wp, bp, None) == INV
            for off in (1, 2, 3):
                assert push(st.handle, xp + off, ci, 5, yp, co, wp, bp, None) == INV
                assert push(st.handle, xp, ci + off, 5, yp, co, wp, bp, None) == INV
                assert push(st.handle, xp, ci, 5, yp + off, co, wp, bp, None) == INV
                assert push(st.handle, xp, ci, 5, yp, co + off, wp, bp, None) == INV
                assert push(st.handle, xp, ci, 5, yp, co, wp + off, bp, None) == INV
                assert push(st.handle, xp, ci, 5, yp, co, wp, bp + off, None) == INV
            assert push(st.handle, xp, ci, 5, yp, co, wp + 4, bp, None) == INV  # win0 is int64
            assert rawpos(None, wp, None) == INV and rawpos(st.handle, None, None) == INV
            assert rawpos(st.handle, wp + 4, None) == INV
            info = (ctypes.c_int64 * 4)()
            assert A.net_streams_raw_info(None, info) == INV and A.net_streams_raw_info(st.handle, None) == INV
            assert state(st, uni) == before
            torch.cuda.synchronize()
            assert bool((y == GUARD).all()) and nb.tolist() == [0] * 4
            assert cout.tolist() == [-7] * 8 and w0.tolist() == [-7] * 8
            assert lib.each_raw_rows(HOP, q, M) == sde.each_raw_rows(HOP, q, M) and lib.each_raw_rows(HOP, 17, M) == 0
            # the Python entry refuses what is no tensor of the group's shape
            for bad in (None, x[:, :4].contiguous().cpu(), x[:4, :4].contiguous(), x[:, :4, :4].contiguous()):
                with pytest.raises(ValueError):
                    st.push_raw(bad, full)
            with pytest.raises(ValueError):
                st.push_raw(x[:, :4].contiguous(), full.cpu())
            assert state(st, uni) == before
