"""Raw frames at q times the network's rate on the GPU: net_streams_set_decimator,
net_streams_push_raw_f32_tm and the hook mibminet_test_fir_decimate.

The reference of a row is never another stream entry: decimate.fir_decimate on the CPU, then the
two-pass quantiser with the set's scale, then the C oracle on the materialised sliding windows
(tests/support_decim.py).  The hook's floats are compared as uint32 bit patterns, everything else as
bytes.  Inputs and taps are such that no non-zero intermediate can be subnormal (support_decim)."""
import numpy as np
import pytest

import support_bank as sb
import support_decim as sd
import support_streams as ss
from mibminet import decimate, lib
from mibminet.params import ParamSet
from support import capped, dev, same_rows, want, windows_at  # noqa: F401 (capped: a fixture)

pytestmark = pytest.mark.gpu

SETS, S, HOP, MAX_PUSH, SCALES = sd.SETS, sd.S, sd.HOP, sd.MAX_PUSH, sd.SCALES
GEOMETRIES = sb.GEOMETRIES[:2]  # (8, 64, 2) and (19, 480, 3)
QK = [(2, 7), (3, 33)]
NAN, INF = float("nan"), float("inf")
OK, INV, UNS = lib.NET_OK, lib.NET_ERR_INVALID, lib.NET_ERR_UNSUPPORTED


def run_raw(torch, st, x, ns, before=None):
    """Pushes the raw frames x [S][L][C] by the list ns; before(index) runs ahead of each push.  Returns
    the rows [S][W][N], the n_bad of every push, and checks the positions after each."""
    out, bad, P = [], [], 0
    q = st.raw_info()[0]
    for i, n in enumerate(ns):
        if before is not None:
            before(i)
        y, nbad = st.push_raw(dev(torch, np.ascontiguousarray(x[:, P: P + n])))
        P += n
        assert st.raw_info()[2:] == [P, decimate.raw_decimated(q, P)] and st.info()[4] == decimate.raw_decimated(q, P)
        out.append(y)
        bad.append(nbad)
    assert P == x.shape[1]
    return torch.cat(out, dim=1).cpu().numpy(), [int(b.item()) for b in bad]


# ---- 3. the hook: the decimated floats themselves, bit for bit ------------------------------------------
@pytest.mark.parametrize("q,K", [(1, 1), (2, 2), (2, 7), (3, 33), (5, 4), (16, 128)])
def test_hook_gives_fir_decimate_bit_for_bit(q, K, gpu):
    import torch

    h = sd.taps(K, 5)
    hd = torch.from_numpy(h).cuda()
    cases = 0
    for R in (8, 22, 64):
        rng = np.random.default_rng([q, K, R])
        for n in (1, q - 1, q, 47):
            for P in (1000 * q + 1, 7 * q, 3):  # off the grid (q > 1), on it, and fewer frames than K - 1 so far
                if n == 0:
                    continue
                x = sd.inputs(rng, (n, R))
                state = sd.inputs(rng, (K - 1, R))  # oldest first: frame P - (K - 1) + i at row i
                state[: max(K - 1 - P, 0)] = 0.0    # frames before the first are zeros
                slots = np.zeros_like(state)
                if K > 1:
                    slots[(P - (K - 1) + np.arange(K - 1)) % (K - 1)] = state
                expect, _ = decimate.fir_decimate(x, h, q, state, P)
                got = lib.fir_decimate_torch(dev(torch, x), dev(torch, slots) if K > 1 else None, hd, q, P)
                assert got.shape == expect.shape == (lib.raw_samples(q, P, n), R)
                np.testing.assert_array_equal(got.cpu().numpy().view(np.uint32), expect.view(np.uint32),
                                              err_msg=f"R {R} n {n} P {P}")
                cases += expect.shape[0] > 0
    assert cases >= 18


# ---- 4. raw pushes over the schedule ----------------------------------------------------------------------
@pytest.mark.parametrize("C,T,N,q,K,cap", [g + qk + (0,) for g in GEOMETRIES for qk in QK] + [GEOMETRIES[1] + QK[1] + (1,)])
def test_raw_pushes_over_the_schedule(C, T, N, q, K, cap, capped):
    import torch

    sets, h, qd, rows = sd.reference(C, T, N, q, K)
    x, ns = sd.frames(C, T, q, K), sd.schedule(T, q, K)
    pl = sd.plan(T, q, ns)
    assert any(n == 1 and m == 0 for _, n, _, m, _, _ in pl) and any(n == q * MAX_PUSH for _, n, _, _, _, _ in pl)
    assert any(all(n < K - 1 for _, n, _, _, _, _ in pl[i: i + 3]) for i in range(len(pl) - 2))
    capped(cap)
    with lib.Bank(sets, SCALES) as bank, lib.Streams(bank, SETS, HOP, MAX_PUSH) as st:
        assert st.raw_info() == [0, 0, 0, 0]
        st.decimate(q, h)
        assert st.raw_info() == [q, K, 0, 0]
        got, bad = run_raw(torch, st, x, ns)
        assert not any(bad) and got.shape[1] == sum(k for *_, k, _ in pl) == st.info()[5]
        for i in range(S):
            same_rows(got[i], rows[i][: got.shape[1]], f"session {i}")
        assert st.info()[4] >= 2 * st.cap + 16
        sd.check_rings(st, sets, qd)


# ---- 5. identity and stride -------------------------------------------------------------------------------
@pytest.mark.parametrize("q", [1, 3])
def test_identity_and_stride(q, gpu):
    """h = [1]: q = 1 gives the bytes of push_f32 on the same frames, rows and rings; q = 3 is x[::3]."""
    import torch

    C, T, N = GEOMETRIES[0]
    sets = sb.sets(C, T, N)
    ns = sd.schedule(T, q, 1)
    x = sd.inputs(np.random.default_rng([C, T, q, 41]), (S, sum(ns), C))
    x *= np.float32(0.5)  # unfiltered, the inputs reach 2^10 only: fewer of them clip at the smaller scales
    one = np.ones(1, np.float32)
    qd = [sd.two_pass(x[i][::q], SCALES[s]) for i, s in enumerate(SETS)]
    with lib.Bank(sets, SCALES) as bank, lib.Streams(bank, SETS, HOP, MAX_PUSH) as st:
        st.decimate(q, one)
        got, bad = run_raw(torch, st, x, ns)
        assert not any(bad)
        for i, s in enumerate(SETS):
            same_rows(got[i], ss.rows_of(sets[s], qd[i], T), f"session {i}")
        sd.check_rings(st, sets, qd)
        if q == 1:
            with lib.Streams(bank, SETS, HOP, MAX_PUSH) as sib:
                out, P = [], 0
                for n in ns:
                    out.append(sib.push_f32(dev(torch, np.ascontiguousarray(x[:, P: P + n])), layout="tc")[0])
                    P += n
                assert np.array_equal(torch.cat(out, dim=1).cpu().numpy(), got)
                for i in range(S):
                    np.testing.assert_array_equal(lib.streams_ring(st, i), lib.streams_ring(sib, i))


# ---- 6. a widened montage ---------------------------------------------------------------------------------
def test_widened_montage_with_non_finite_unselected_electrodes(gpu):
    """19 x 480 sets widened to 64 rows: the unselected electrodes carry NaN and the infinities, in the
    chunks and so in the histories; the rows are the oracle's under the ORIGINAL sets on the selected
    columns."""
    import torch

    T, N, R, q, K = 480, 3, 64, 2, 7
    orig = tuple(ParamSet.synthetic(seed=331 + i, C=19, T=T, N=N) for i in range(3))
    maps = [[int(c) for c in np.random.default_rng([R, 50 + i]).permutation(R)[:19]] for i in range(3)]
    h, ns = sd.taps(K, 12), sd.schedule(T, q, K)
    rng = np.random.default_rng([R, T, 9])
    x = sd.inputs(rng, (3, sum(ns), R))
    expect = []
    for i, ps in enumerate(orig):
        keep = x[i][:, maps[i]].copy()
        junk = rng.random(x[i].shape)
        x[i][junk < 0.1] = NAN
        x[i][(junk >= 0.1) & (junk < 0.2)] = -INF
        x[i][(junk >= 0.2) & (junk < 0.3)] = INF
        x[i][:, maps[i]] = keep
        expect.append(sd.session_reference(ps, SCALES[i], keep, h, q, T)[1])
    wide = [ps.widened(R, maps[i]) for i, ps in enumerate(orig)]
    with lib.Bank(wide, SCALES[:3]) as bank, lib.Streams(bank, (0, 1, 2), HOP, MAX_PUSH) as st:
        st.decimate(q, h)
        got, bad = run_raw(torch, st, x, ns)
        assert not any(bad)
        for i in range(3):
            same_rows(got[i], expect[i][: got.shape[1]], f"session {i}")


# ---- 7. a restart mid-schedule ----------------------------------------------------------------------------
def test_restart_zeroes_the_history(gpu):
    """Session RESTART[0] restarts under set RESTART[1] ahead of a push at a raw position off the grid:
    its later rows are those of a session whose earlier frames were all zero, the windows that start
    before its origin are zero rows counted in n_bad, the other sessions are untouched."""
    import torch

    (C, T, N), (q, K) = GEOMETRIES[0], QK[1]
    sets, h, qd, rows = sd.reference(C, T, N, q, K)
    x, ns = sd.frames(C, T, q, K), sd.schedule(T, q, K)
    pl = sd.plan(T, q, ns)
    i_r, s_r = ss.RESTART
    at = next(i for i, (P, _, d0, *_) in enumerate(pl) if d0 > T + 20 and P % q)
    P_r, origin = pl[at][0], pl[at][2]
    zeroed = np.array(x[i_r])
    zeroed[:P_r] = 0.0
    rows_r = sd.session_reference(sets[s_r], SCALES[s_r], zeroed, h, q, T)[1]
    with lib.Bank(sets, SCALES) as bank, lib.Streams(bank, SETS, HOP, MAX_PUSH) as st:
        st.decimate(q, h)
        got, bad = run_raw(torch, st, x, ns, before=lambda i: st.restart(i_r, s_r) if i == at else None)
        assert st.origin(i_r) == (origin, s_r)
        W = got.shape[1]
        for i in range(S):
            if i != i_r:
                same_rows(got[i], rows[i][:W], f"session {i}")
        expect, w, want_bad = np.array(rows[i_r][:W]), 0, []
        for j, (_, _, _, _, k, onsets) in enumerate(pl):
            n_bad = 0
            for o in onsets:
                if j >= at:
                    expect[w] = rows_r[w] if o >= origin else 0
                    n_bad += o < origin
                w += 1
            want_bad.append(n_bad)
        assert w == W and sum(want_bad) > 0 and bad == want_bad
        same_rows(got[i_r], expect, "the restarted session")
        sd.check_rings(st, sets, qd, skip=(i_r,))


# ---- 8. windows at cues given in raw frames ---------------------------------------------------------------
def test_windows_at_after_a_raw_push(gpu):
    import torch

    (C, T, N), (q, K) = GEOMETRIES[0], QK[0]
    sets, h, qd, _ = sd.reference(C, T, N, q, K)
    x, ns = sd.frames(C, T, q, K), sd.schedule(T, q, K)
    with lib.Bank(sets, SCALES) as bank, lib.Streams(bank, SETS, HOP, MAX_PUSH) as st:
        st.decimate(q, h)
        run_raw(torch, st, x, ns)
        lo, hi = st.at_span()
        P = st.raw_info()[2]
        assert (lo, hi) == (st.info()[4] - st.cap, st.info()[4] - T) and lo > 0
        cues = [q * lo, q * lo + 1, q * (lo + 7) - 1, q * hi - 3, q * hi]  # raw frames: on and off the grid
        onsets = [decimate.raw_decimated(q, a) for a in cues]
        assert all(lo <= o <= hi for o in onsets) and P >= cues[-1]
        sessions = [0, 1, 2, 3, 4]
        got = st.windows_at(sessions, onsets).cpu().numpy()
        for w, (i, o) in enumerate(zip(sessions, onsets)):
            np.testing.assert_array_equal(got[w], want(sets[SETS[i]], windows_at(qd[i], [o], T))[0], err_msg=f"item {w}")


# ---- 9. refusals ------------------------------------------------------------------------------------------
def test_refusals_leave_the_group_unchanged(gpu):
    import ctypes

    import torch

    (C, T, N), (q, K) = GEOMETRIES[0], QK[0]
    sets, h = sb.sets(C, T, N), sd.taps(K, 11)
    A = lib.load()
    x = dev(torch, sd.inputs(np.random.default_rng(4), (S, q * MAX_PUSH + 1, C)))
    y = torch.full((S, MAX_PUSH, N), 0x5A, dtype=torch.int8, device="cuda")
    nb = torch.zeros((1,), dtype=torch.int32, device="cuda")
    xp, yp, bp = x.data_ptr(), y.data_ptr(), nb.data_ptr()

    def taps_ptr(a):
        return a.ctypes.data_as(ctypes.c_void_p)

    def state(*groups):
        torch.cuda.synchronize()
        return [(g.raw_info(), g.info(), [lib.streams_ring(g, i).tobytes() for i in range(S)]) for g in groups]

    with lib.Bank(sets, SCALES) as bank, lib.Bank(sets) as bare:
        with lib.Streams(bank, SETS, HOP, MAX_PUSH) as st, lib.Streams(bank, SETS, HOP, MAX_PUSH) as plain, \
                lib.StreamsEach(bank, SETS, HOP, MAX_PUSH) as ea, lib.Streams(bare, SETS, HOP, MAX_PUSH) as nos:
            # set_decimator: the limits, the taps, the kind of group, the bank
            nan = h.copy()
            nan[3] = NAN
            before = state(st, nos)
            for qq, taps, KK in ((0, h, K), (17, h, K), (q, h, 0), (q, np.resize(h, 129), 129), (q, nan, K)):
                assert A.net_streams_set_decimator(st.handle, qq, taps_ptr(taps), KK, None) == INV, (qq, KK)
            assert A.net_streams_set_decimator(st.handle, q, None, K, None) == INV
            assert A.net_streams_set_decimator(None, q, taps_ptr(h), K, None) == INV
            assert A.net_streams_set_decimator(nos.handle, q, taps_ptr(h), K, None) == INV
            assert A.net_streams_set_decimator(ea.handle, q, taps_ptr(h), K, None) == UNS
            assert state(st, nos) == before and ea.info()[:5] == [S, HOP, MAX_PUSH, st.cap, 0]
            # a raw push on a plain group, a second decimator, a decimator after a push
            assert A.net_streams_push_raw_f32_tm(plain.handle, xp, 5, yp, bp, None) == INV
            plain.push_f32(x[:, :5].contiguous(), layout="tc")
            before = state(plain)
            assert A.net_streams_set_decimator(plain.handle, q, taps_ptr(h), K, None) == INV
            assert A.net_streams_push_raw_f32_tm(plain.handle, xp, 5, yp, bp, None) == INV
            assert state(plain) == before
            st.decimate(q, h)
            for _ in range(2):  # past T decimated samples: the next push completes windows
                st.push_raw(x[:, : q * MAX_PUSH].contiguous())
            assert st.info()[4] == 2 * MAX_PUSH >= T and lib.raw_samples(q, st.raw_info()[2], q * MAX_PUSH) == MAX_PUSH
            before = state(st)
            assert A.net_streams_set_decimator(st.handle, q, taps_ptr(h), K, None) == INV
            # the plain entries on a decimating group
            assert A.net_streams_push_f32_tm(st.handle, xp, 5, yp, bp, None) == INV
            assert A.net_streams_push_f32(st.handle, xp, 5, yp, bp, None) == INV
            assert A.net_streams_push(st.handle, xp, 0, 5, yp, bp, None) == INV
            # the raw push's own checks: the size, x, y with k > 0, n_bad; n_raw == 0 is no error
            assert A.net_streams_push_raw_f32_tm(st.handle, xp, q * MAX_PUSH + 1, yp, bp, None) == INV
            assert A.net_streams_push_raw_f32_tm(st.handle, xp + 2, 2 * q * HOP, yp, bp, None) == INV
            assert A.net_streams_push_raw_f32_tm(st.handle, None, 2 * q * HOP, yp, bp, None) == INV
            assert st.windows(MAX_PUSH) > 0
            assert A.net_streams_push_raw_f32_tm(st.handle, xp, q * MAX_PUSH, None, bp, None) == INV
            assert A.net_streams_push_raw_f32_tm(st.handle, xp, q * MAX_PUSH, yp + 1, bp, None) == INV
            assert A.net_streams_push_raw_f32_tm(st.handle, xp, q * MAX_PUSH, yp, bp + 2, None) == INV
            assert A.net_streams_push_raw_f32_tm(None, xp, 5, yp, bp, None) == INV
            assert A.net_streams_push_raw_f32_tm(ea.handle, xp, 5, yp, bp, None) == INV
            assert A.net_streams_push_raw_f32_tm(st.handle, None, 0, None, None, None) == OK
            assert state(st) == before
            torch.cuda.synchronize()
            assert bool((y == 0x5A).all()) and nb.item() == 0
            info = (ctypes.c_int64 * 4)()
            assert A.net_streams_raw_info(None, info) == INV and A.net_streams_raw_info(st.handle, None) == INV
