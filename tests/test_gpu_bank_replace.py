"""net_bank_replace on the device: one set of a resident bank replaced in stream order while the
others, and the stream groups on the bank, go on.  At 8 x 64 x 2 (minimum T) and 19 x 480 x 3 (tail
tiles).

The reference of every row is the C oracle of the set that row must have been decoded by, on the
materialised item (support_bank.table, support.want, support_streams.rows_of), never another GPU entry;
every comparison is byte-exact.  tests/test_bank_replace_cpu.py certifies that the replacing sets change
every reference row under the slot, so a call that read the old set, or a slot half written, cannot
pass."""
import numpy as np
import pytest

import support_bank as sb
import support_features as sf
import support_streams as ss
import support_streams_each as se
from mibminet import lib
from mibminet.params import ParamSet
from support import SCALE, at_offset, dequant, same, want

pytestmark = pytest.mark.gpu
E, SLOT = sf.E, sf.SLOT
UNS = lib.NET_ERR_UNSUPPORTED
S, X = ParamSet.synthetic, ParamSet.synthetic_extreme


def _expected(C, T, N, so, new=None):
    """The rows of the first E epochs under set_of `so`, slot SLOT being `new` (None: as created)."""
    ref = sb.reference(sb.table(C, T, N)[:, :E], so).copy()
    if new is not None:
        ref[so == SLOT] = want(new, sb.epochs(C, T)[:E])[so == SLOT]
    return ref


# ---- 1. the ordering claim ----------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", ["alternating", "grouped"])
@pytest.mark.parametrize("C,T,N", sf.REPLACE_GEOMETRIES)
def test_calls_before_read_the_old_set_and_calls_after_the_new(C, T, N, pattern, gpu):
    """A call, the replacement of set 2, a second call, two replacements back to back and a third call,
    all on one stream with no synchronisation between them, the outputs read afterwards: the first
    call's rows under set 2 are the old set's, the second's the new set's, the third's the last
    replacement's; every other row is the same in all three."""
    import torch

    src, onsets, channels = sb.case(C, T)
    so = sb.patterns(E)[pattern]
    assert (so == SLOT).sum() >= 4
    new, head = sf.new_set(C, T, N), sf.head_set(C, T, N)
    xd = at_offset(torch, src, 3)
    on = torch.tensor(onsets[:E], dtype=torch.int64).cuda()
    sod = torch.tensor(so, dtype=torch.int32).cuda()
    with lib.Bank(sb.sets(C, T, N)) as bank:
        call = lambda: lib.forward_epochs_bank_torch(bank, xd, on, sod, channels=channels, check=False)
        call()  # the upload (one host sync); everything below is enqueued without one
        assert bank.device_copies() == 1
        torch.cuda.synchronize()
        y0 = call()
        bank.replace(SLOT, new)
        y1 = call()
        bank.replace(SLOT, sb.sets(C, T, N)[0])  # overwritten at once: its pinned source must not be reused early
        bank.replace(SLOT, head)
        y2 = call()
        torch.cuda.synchronize()
        same(y0.cpu().numpy(), _expected(C, T, N, so), "before")
        same(y1.cpu().numpy(), _expected(C, T, N, so, new), "after the replacement")
        same(y2.cpu().numpy(), _expected(C, T, N, so, head), "after two more: the second wins")
        with lib.Bank(sb.sets(C, T, N)[:2] + (head,)) as fresh:
            assert bank.image(SLOT) == fresh.image(2)
        # the features entry reads the same copy
        y, f = lib.forward_epochs_bank_torch(bank, xd, on, sod, channels=channels, check=False, features=True)
        same(y.cpu().numpy(), _expected(C, T, N, so, head), "features entry")
        ref_f = sb.reference(sf.table(C, T, N)[0], so)  # the head-only set shares layers 1-4
        assert np.array_equal(f.cpu().numpy(), ref_f)


def test_the_scale_is_replaced_with_the_set(gpu):
    import torch

    C, T, N = 19, 480, 3
    src, onsets, channels = sb.case(C, T)
    so = sb.patterns(E)["alternating"]
    new = sf.new_set(C, T, N)
    xf = torch.from_numpy(dequant(src) * np.float32(2.0)).cuda()  # quantises back to src under scale 2 SCALE
    with lib.Bank(sb.sets(C, T, N), [2 * SCALE] * 2 + [SCALE] + [2 * SCALE] * 2) as bank:
        y0 = lib.forward_epochs_bank_torch(bank, xf, onsets[:E], so, channels=channels, check=False)
        bank.replace(SLOT, new, 2 * SCALE)
        y1 = lib.forward_epochs_bank_torch(bank, xf, onsets[:E], so, channels=channels, check=False)
        torch.cuda.synchronize()
        ok = so != SLOT
        same(y0.cpu().numpy()[ok], _expected(C, T, N, so)[ok], "other sets, before")
        same(y1.cpu().numpy(), _expected(C, T, N, so, new), "the new set under its new scale")


# ---- 2. refusals once the copy exists -------------------------------------------------------------------
@pytest.mark.parametrize("C,T,N", sf.REPLACE_GEOMETRIES)
def test_refusals_change_nothing_on_the_device(C, T, N, gpu):
    import torch

    src, onsets, channels = sb.case(C, T)
    so = sb.patterns(E)["alternating"]
    xd = at_offset(torch, src, 1)
    good = sf.new_set(C, T, N)
    with lib.Bank(sb.sets(C, T, N), [1.0] * 5) as bank:
        call = lambda: lib.forward_epochs_bank_torch(bank, xd, onsets[:E], so, channels=channels).cpu().numpy()
        before, images, info = call(), [bank.image(s) for s in range(5)], bank.info()
        same(before, _expected(C, T, N, so), "before")
        blob = good.to_blob()
        for new, scale, code in ((blob[:-4], 1.0, lib.NET_ERR_BLOB), (S(seed=9, C=C, T=T, N=N + 1), 1.0, UNS),
                                 (S(seed=9, C=C, T=T, N=N, reorder_bn=False), 1.0, UNS),
                                 (X(seed=77, C=C, T=T, N=N, mids=3), 1.0, UNS), (good, 0.0, lib.NET_ERR_INVALID),
                                 (good, 2.0**61, lib.NET_ERR_RANGE)):
            with pytest.raises(lib.NetError) as e:
                bank.replace(SLOT, new, scale)
            assert e.value.code == code
        with pytest.raises(lib.NetError) as e:
            bank.replace(5, good, 1.0)
        assert e.value.code == lib.NET_ERR_INVALID
        # a capturing stream: host data is copied, so the call is refused and nothing is captured
        g, s = torch.cuda.CUDAGraph(), torch.cuda.Stream()
        t = torch.zeros(8, device="cuda")
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            with torch.cuda.graph(g, stream=s):
                t += 1
                with pytest.raises(lib.NetError) as e:
                    bank.replace(SLOT, good, 1.0, stream=s)
                assert e.value.code == UNS
        g.replay()
        torch.cuda.synchronize()
        assert t.tolist() == [1.0] * 8
        del g
        assert [bank.image(s) for s in range(5)] == images and bank.info() == info and bank.device_copies() == 1
        same(call(), before, "after the refusals")


# ---- 3. a live uniform group ----------------------------------------------------------------------------
@pytest.mark.parametrize("C,T,N", sf.REPLACE_GEOMETRIES)
def test_a_live_group_goes_on_under_a_replaced_set(C, T, N, gpu):
    """support_streams' schedule.  A third of the way in, set 3 (session 3's) is replaced by itself with
    another head, with no restart: every later row of session 3, windows that began before the
    replacement included, is the oracle's under the hybrid.  Two thirds in, it is replaced by an
    unrelated set and session 3 restarts: the windows that start before its origin are zero rows
    counted in n_bad, the others the oracle's under the new set.  The other sessions' rows are what
    they are without any replacement, throughout."""
    import torch

    ns, x = ss.schedule(T), ss.chunks(C, T)
    plan = ss.plan(T, ss.HOP, ns)
    sets = sb.sets(C, T, N)
    who, slot = 3, ss.SETS[3]
    assert ss.SETS.count(slot) == 1
    hybrid, new = sb.hybrid(sets[slot], sets[4], 5), sf.new_set(C, T, N)
    tab = ss.table(C, T, N)
    old_rows, hyb_rows, new_rows = tab[(who, slot)], ss.rows_of(hybrid, x[who], T), ss.rows_of(new, x[who], T)
    # (conditions on the references) the three sets are told apart by most rows, and none is zeros
    assert (hyb_rows != old_rows).any(axis=1).mean() >= 0.75 and (new_rows != hyb_rows).any(axis=1).mean() >= 0.75
    assert new_rows.any(axis=1).all() and hyb_rows.any(axis=1).all()
    j1, j2 = len(ns) // 3, 2 * len(ns) // 3
    origin = plan[j2][0]
    assert any(o < plan[j1][0] for p in plan[j1:] for o in p[4])  # windows that began before the first replacement
    assert any(o < origin for p in plan[j2:] for o in p[4]) and any(o >= origin for o in plan[-1][4])
    xd = torch.from_numpy(np.array(x)).cuda()
    with lib.Bank(sets) as bank, lib.Streams(bank, ss.SETS, ss.HOP, ss.MAX_PUSH) as st:
        out = []
        for j, (pos, n, k, W0, onsets) in enumerate(plan):
            if j == j1:
                bank.replace(slot, hybrid)
            if j == j2:
                bank.replace(slot, new)
                st.restart(who, slot)
            out.append(st.push(xd[:, :, pos: pos + n].contiguous()))
        torch.cuda.synchronize()
        assert st.origin(who) == (origin, slot)
        zeros = 0
        for j, ((y, nbad), (pos, n, k, W0, onsets)) in enumerate(zip(out, plan)):
            y = y.cpu().numpy()
            expect = np.stack([tab[(i, ss.SETS[i])][W0: W0 + k] for i in range(ss.S)]).reshape(ss.S, k, N)
            if j >= j1:
                expect[who] = hyb_rows[W0: W0 + k]
            late = 0
            if j >= j2:
                early = np.array([o < origin for o in onsets], bool)
                expect[who] = new_rows[W0: W0 + k]
                expect[who][early] = 0
                late = int(early.sum())
            zeros += late
            assert int(nbad.item()) == late, j
            for i in range(ss.S):
                same(y[i], expect[i], f"push {j}, session {i}")
        assert zeros > 0


# ---- 4. a captured push of an each-group ------------------------------------------------------------------
def test_a_captured_push_decodes_under_the_new_set_without_recapture(gpu):
    """net_streams_push_each captured once and replayed tick after tick; between two replays set 3 is
    replaced (another head, so the rings stay valid).  The graph reads the bank's copy when it
    replays: session 3's rows are the old set's before the replacement and the hybrid's after it."""
    import torch

    C, T, N = 19, 480, 3
    n_max, counts = se.schedule(T)
    w = se.walk(T)
    x, sets = ss.chunks(C, T), sb.sets(C, T, N)
    M, hop = ss.MAX_PUSH, ss.HOP
    kmax = se.each_rows(hop, M)
    who, slot = 3, ss.SETS[3]
    hybrid = sb.hybrid(sets[slot], sets[4], 5)
    tab = ss.table(C, T, N)
    rows = {i: tab[(i, ss.SETS[i])] for i in range(ss.S)}
    hyb_rows = ss.rows_of(hybrid, x[who], T)
    t0 = next(t for t in range(len(n_max)) if all(w.pos[t, i] >= T + 3 for i in range(4)))
    ticks = list(range(t0, min(t0 + 6, len(n_max))))
    assert len(ticks) >= 4
    A = lib.load()
    with lib.Bank(sets) as bank, lib.StreamsEach(bank, ss.SETS, hop, M) as st:
        xs = torch.zeros((ss.S, C, M), dtype=torch.int8, device="cuda")
        cin = torch.zeros((ss.S,), dtype=torch.int32, device="cuda")
        y = torch.zeros((ss.S, kmax, N), dtype=torch.int8, device="cuda")
        cout = torch.zeros((ss.S,), dtype=torch.int32, device="cuda")
        s = torch.cuda.Stream()
        push = (st.handle, xs.data_ptr(), 1, cin.data_ptr(), M, y.data_ptr(), cout.data_ptr(), None, None)
        cur = [0] * ss.S

        def load(t):
            slot_x = np.full((ss.S, C, M), 0x33, np.int8)
            for i in range(ss.S):
                slot_x[i, :, : counts[t][i]] = x[i, :, cur[i]: cur[i] + counts[t][i]]
                cur[i] += int(counts[t][i])
            xs.copy_(torch.from_numpy(slot_x))
            cin.copy_(torch.from_numpy(np.array(counts[t], np.int32)))

        for t in range(t0):
            load(t)
            torch.cuda.synchronize()
            assert A.net_streams_push_each(*push, s.cuda_stream) == lib.NET_OK
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(s):
            with torch.cuda.graph(g, stream=s):
                assert A.net_streams_push_each(*push, s.cuda_stream) == lib.NET_OK
        torch.cuda.synchronize()
        seen = {False: 0, True: 0}
        for n, t in enumerate(ticks):
            replaced = n >= len(ticks) // 2
            if n == len(ticks) // 2:
                bank.replace(slot, hybrid, stream=s)  # ordered on the stream the graph replays on
            load(t)
            torch.cuda.synchronize()
            with torch.cuda.stream(s):
                g.replay()
            torch.cuda.synchronize()
            got, k = y.cpu().numpy(), cout.cpu().tolist()
            assert k == w.k[t].tolist()
            for i in range(ss.S):
                src = hyb_rows if (replaced and i == who) else rows[i]
                W0 = int(w.W0[t, i])
                same(got[i, : k[i]], src[W0: W0 + k[i]], f"tick {t}, session {i}")
                if i == who and k[i] and (hyb_rows[W0: W0 + k[i]] != rows[i][W0: W0 + k[i]]).any():
                    seen[replaced] += 1
        assert seen[True] > 0  # a tick after the replacement told the two sets apart
        del g
