"""The layer-4 activations beside the logits (net_model_compute_epochs_bank_feat[_f32],
net_streams_windows_at_feat; forward_gen.hpp: finish_prev_feat, store_feat).

The reference of a feature row is the C oracle's layer chain on the materialised item with the pad
columns dropped (support_features.features, which also holds the chain to the oracle's model), the
reference of a logit row the oracle's model; never another GPU entry, every comparison byte-exact.
Every call writes its features into a buffer prefilled with 0x55 between guard bytes that must
survive.  tests/test_bank_replace_cpu.py certifies that no reference feature row is all zeros, which is
what an invalid item gets."""
import numpy as np
import pytest

import support_bank as sb
import support_features as sf
import support_streams as ss
import support_streams_at as sa
import support_streams_each as se
from mibminet import lib
from support import GUARD, SCALE, at_offset, capped, dequant, same, windows_at  # noqa: F401 (capped: a fixture)

pytestmark = pytest.mark.gpu
FILL, LEAD = 0x55, 64
INV = lib.NET_ERR_INVALID
E = sf.E
# T64 = 1 (one 16-byte row per item), 7 (odd: byte stores), 17, 64 (every layer-4 part, 16-byte stores)
GEOMETRIES = [(8, 64, 2), (19, 480, 3), (22, 1125, 4), (4, 4096, 16)]


class Out:
    """y [n][N] and feat [n][16][T64] on the device, each between LEAD guard bytes, feat prefilled
    with FILL; the counter between two others."""

    def __init__(self, n, N, T64):
        import torch

        self.n, self.N, self.fb = n, N, 16 * T64
        self.y = torch.full((2 * LEAD + n * N,), GUARD, dtype=torch.int8, device="cuda")
        self.f = torch.full((2 * LEAD + n * self.fb,), GUARD, dtype=torch.int8, device="cuda")
        self.f[LEAD: LEAD + n * self.fb] = FILL
        self.nb = torch.zeros((3,), dtype=torch.int32, device="cuda")
        assert self.f.data_ptr() % 16 == 0
        self.yp, self.fp, self.nbp = self.y.data_ptr() + LEAD, self.f.data_ptr() + LEAD, self.nb.data_ptr() + 4

    def read(self):
        """([n][N], [n][16][T64], the count) after checking that nothing outside them was written."""
        import torch

        torch.cuda.synchronize()
        y, f, nb = self.y.cpu().numpy(), self.f.cpu().numpy(), self.nb.cpu().tolist()
        for buf, size in ((y, self.n * self.N), (f, self.n * self.fb)):
            assert (buf[:LEAD] == GUARD).all() and (buf[LEAD + size:] == GUARD).all(), "bytes outside the rows were written"
        assert nb[0] == 0 == nb[2]
        return (y[LEAD: LEAD + self.n * self.N].reshape(self.n, self.N),
                f[LEAD: LEAD + self.n * self.fb].reshape(self.n, 16, self.fb // 16), nb[1])


def epochs_feat(bank, src, row_stride, channels, onsets, set_of, f32=False, expect=lib.NET_OK):
    """One call of the C entry on the device source `src`; returns Out.read()."""
    import ctypes

    import torch

    d = bank.dims
    n = len(onsets)
    on = torch.tensor([int(o) for o in onsets], dtype=torch.int64).cuda()
    so = torch.tensor([int(s) for s in set_of], dtype=torch.int32).cuda()
    ch = (ctypes.c_int32 * d.C)(*channels)
    out = Out(n, d.N, d.T64)
    fn = lib.load().net_model_compute_epochs_bank_feat_f32 if f32 else lib.load().net_model_compute_epochs_bank_feat
    rc = fn(bank.handle, src.data_ptr(), src.numel(), row_stride, ch, on.data_ptr(), so.data_ptr(), n, out.yp, out.fp, out.nbp,
            0, torch.cuda.current_stream().cuda_stream)
    assert rc == expect, rc
    return out.read()


# ---- 1. the epochs-bank entries ---------------------------------------------------------------------
@pytest.mark.parametrize("C,T,N", GEOMETRIES)
def test_epochs_bank_features_and_logits(C, T, N, capped):
    """E = 23 epochs under one workgroup and under three (later passes, and set switches inside a
    range), the sets alternating, grouped and with one set unused."""
    import torch

    src, onsets, channels = sb.case(C, T)
    feat, logits = sf.table(C, T, N)
    xd = at_offset(torch, src, 3)
    with lib.Bank(sb.sets(C, T, N)) as bank:
        assert bank.feature_bytes() == 16 * (T // 64)
        for name in ("alternating", "grouped", "one-unused"):
            so = sb.patterns(E)[name]
            for cap in (1, 3):
                capped(cap)
                y, f, nbad = epochs_feat(bank, xd, src.shape[1], channels, onsets[:E], so)
                assert nbad == 0
                same(y, sf.reference(logits, so), f"logits, {name}, cap {cap}")
                same(f, sf.reference(feat, so), f"features, {name}, cap {cap}")
        capped(0)
        # the Python entry, and the plain entry beside it
        so = sb.patterns(E)["alternating"]
        y, f = lib.forward_epochs_bank_torch(bank, xd, onsets[:E], so, channels=channels, features=True)
        assert tuple(f.shape) == (E, 16, T // 64) and f.dtype == torch.int8
        same(f.cpu().numpy(), sf.reference(feat, so), "features=True")
        assert torch.equal(y, lib.forward_epochs_bank_torch(bank, xd, onsets[:E], so, channels=channels))


@pytest.mark.parametrize("variant", ["plain-bn", "all-exact"])
def test_variants(variant, capped):
    import torch

    C, T, N = 19, 480, 3
    src, onsets, channels = sb.case(C, T)
    feat, logits = sf.table(C, T, N, variant)
    so = sb.patterns(E)["alternating"]
    with lib.Bank(sb.VARIANTS[variant](C, T, N)) as bank:
        assert bank.exact_division == (variant in sb.EXACT)
        capped(3)
        y, f, nbad = epochs_feat(bank, at_offset(torch, src, 1), src.shape[1], channels, onsets[:E], so)
        assert nbad == 0
        same(y, sf.reference(logits, so), variant)
        same(f, sf.reference(feat, so), variant)


def test_float_entry(capped):
    import torch

    C, T, N = 19, 480, 3
    src, onsets, channels = sb.case(C, T)
    feat, logits = sf.table(C, T, N)
    so = sb.patterns(E)["grouped"]
    xf = torch.from_numpy(dequant(src)).cuda()
    with lib.Bank(sb.sets(C, T, N), [SCALE] * 5) as bank:
        capped(3)
        y, f, nbad = epochs_feat(bank, xf, src.shape[1], channels, onsets[:E], so, f32=True)
        assert nbad == 0
        same(y, sf.reference(logits, so), "float logits")
        same(f, sf.reference(feat, so), "float features")


@pytest.mark.parametrize("C,T,N", [(8, 64, 2), (19, 480, 3), (4, 4096, 16)])
def test_invalid_items_get_zero_rows(C, T, N, capped):
    """One bad onset and one bad set index: two zero feature rows beside two zero logit rows, each
    counted once, the neighbours exact, every other byte of the prefilled buffer overwritten."""
    import torch

    src, onsets, channels = sb.case(C, T)
    feat, logits = sf.table(C, T, N)
    so = sb.patterns(E)["alternating"].copy()
    on = list(onsets[:E])
    on[5], so[11] = sb.last_onset(C, T) + 1, 5
    on[E - 1], so[E - 1] = -1, -1  # both wrong: counted once
    bad = np.zeros(E, bool)
    bad[[5, 11, E - 1]] = True
    ref_y, ref_f = sf.reference(logits, np.where(bad, 0, so)).copy(), sf.reference(feat, np.where(bad, 0, so)).copy()
    ref_y[bad], ref_f[bad] = 0, 0
    with lib.Bank(sb.sets(C, T, N)) as bank:
        for cap in (1, 3, 0):
            capped(cap)
            y, f, nbad = epochs_feat(bank, at_offset(torch, src, 2), src.shape[1], channels, on, so)
            assert nbad == 3, cap
            same(y, ref_y, f"cap {cap}")
            same(f, ref_f, f"cap {cap}")
        capped(0)
        with pytest.raises(ValueError, match="3 of 23"):
            lib.forward_epochs_bank_torch(bank, at_offset(torch, src, 2), on, so, channels=channels, features=True)


def test_feat_must_be_there_and_aligned(gpu):
    import ctypes

    import torch

    C, T, N = 8, 64, 2
    src, onsets, channels = sb.case(C, T)
    xd = torch.from_numpy(src).cuda()
    with lib.Bank(sb.sets(C, T, N)) as bank, lib.StreamsEach(bank, ss.SETS, ss.HOP, ss.MAX_PUSH) as each:
        on = torch.tensor(onsets[:4], dtype=torch.int64).cuda()
        so = torch.zeros(4, dtype=torch.int32).cuda()
        ses = torch.zeros(4, dtype=torch.int32).cuda()
        out = Out(4, N, 1)
        ch = (ctypes.c_int32 * C)(*channels)
        ep, at = lib.load().net_model_compute_epochs_bank_feat, lib.load().net_streams_windows_at_feat
        for fp in (None, out.fp + 1, out.fp + 4, out.fp + 8):
            assert ep(bank.handle, xd.data_ptr(), xd.numel(), src.shape[1], ch, on.data_ptr(), so.data_ptr(), 4, out.yp, fp,
                      out.nbp, 0, None) == INV
            assert at(each.handle, ses.data_ptr(), on.data_ptr(), 4, out.yp, fp, out.nbp, None) == INV
        assert at(each.handle, None, None, 0, None, None, None, None) == lib.NET_OK
        y, f, nbad = out.read()
        assert (y == GUARD).all() and (f == FILL).all() and nbad == 0  # nothing was enqueued


# ---- 2. windows out of the live rings -----------------------------------------------------------------
def at_feat(st, items):
    """One call of net_streams_windows_at_feat on the (session, onset) items; returns Out.read()."""
    import torch

    d = st.bank.dims
    ses = torch.tensor([int(i) for i, _ in items], dtype=torch.int32).cuda()
    ons = torch.tensor([int(o) for _, o in items], dtype=torch.int64).cuda()
    out = Out(len(items), d.N, d.T64)
    rc = lib.load().net_streams_windows_at_feat(st.handle, ses.data_ptr(), ons.data_ptr(), len(items), out.yp, out.fp,
                                                out.nbp, torch.cuda.current_stream().cuda_stream)
    assert rc == lib.NET_OK, rc
    return out.read()


_ROWS = {}


def window_rows(C, T, N, items):
    """([n][N], [n][16][T64]): the oracle's logits and features of the windows x[i][:, o : o + T] of
    support_streams' chunks under each session's set, each window computed once."""
    sets, x = sb.sets(C, T, N), ss.chunks(C, T)
    todo = sorted({it for it in items if (C, T, it) not in _ROWS})
    for i in sorted({i for i, _ in todo}):
        on = [o for k, o in todo if k == i]
        f, y = sf.features(sets[ss.SETS[i]], windows_at(np.ascontiguousarray(x[i]), on, T))
        for o, fr, yr in zip(on, f, y):
            _ROWS[(C, T, (i, o))] = (yr, fr)
    return np.stack([_ROWS[(C, T, it)][0] for it in items]), np.stack([_ROWS[(C, T, it)][1] for it in items])


@pytest.mark.parametrize("C,T,N", [(8, 64, 2), (19, 480, 3)])
def test_windows_at_features_on_a_uniform_group(C, T, N, capped):
    """At every query point of support_streams_at (before the ring is full, after the pushes that
    crossed the seam, past two laps): every session's newest and oldest window and onsets at every
    residue mod 16, so windows that wrap the seam and windows that do not, with two invalid items
    (one past the newest, a session outside the group) in the list."""
    import torch

    ns, x = ss.schedule(T), torch.from_numpy(np.array(ss.chunks(C, T))).cuda()
    cap = ss.cap(T, ss.MAX_PUSH)
    with lib.Bank(sb.sets(C, T, N)) as bank, lib.Streams(bank, ss.SETS, ss.HOP, ss.MAX_PUSH) as st:
        done, wrapped = 0, 0
        for j in sa.points(T):
            while done <= j:
                pos = st.info()[4]
                st.push(x[:, :, pos: pos + ns[done]].contiguous())
                done += 1
            pos = st.info()[4]
            good = sa.uniform_items(T, pos)
            wrapped += sum(sa.wraps(o, T, cap) for _, o in good)
            items = good[:3] + [(1, pos - T + 1)] + good[3:] + [(ss.S, pos - T)]
            ok = np.ones(len(items), bool)
            ok[[3, len(items) - 1]] = False
            ref_y, ref_f = np.zeros((len(items), N), np.int8), np.zeros((len(items), 16, T // 64), np.int8)
            ref_y[ok], ref_f[ok] = window_rows(C, T, N, good)
            np.testing.assert_array_equal(ref_y[ok], sa.expected(C, T, N, good))
            for gc in (1, 3, 0):
                capped(gc)
                y, f, nbad = at_feat(st, items)
                assert nbad == 2, (j, gc)
                same(y, ref_y, f"logits, push {j}, cap {gc}")
                same(f, ref_f, f"features, push {j}, cap {gc}")
            capped(0)
        assert wrapped > 0
        good = sa.uniform_items(T, pos)
        y, f = st.windows_at([i for i, _ in good], [o for _, o in good], features=True)
        same(f.cpu().numpy(), window_rows(C, T, N, good)[1], "Streams.windows_at(features=True)")
        assert torch.equal(y, st.windows_at([i for i, _ in good], [o for _, o in good]))


@pytest.mark.parametrize("C,T,N", [(8, 64, 2), (19, 480, 3)])
def test_windows_at_features_on_an_each_group(C, T, N, capped):
    """The sessions at positions of their own (support_streams_each's schedule, all of it), the onsets
    in every session's own count; one item from before a session's ring and one negative onset."""
    import torch

    n_max, counts = se.schedule(T)
    w = se.walk(T)
    x = ss.chunks(C, T)
    with lib.Bank(sb.sets(C, T, N)) as bank, lib.StreamsEach(bank, ss.SETS, ss.HOP, ss.MAX_PUSH) as st:
        cur = [0] * ss.S
        for t in range(len(n_max)):
            slot = np.full((ss.S, C, n_max[t]), 0x33, np.int8)
            for i in range(ss.S):
                slot[i, :, : counts[t][i]] = x[i, :, cur[i]: cur[i] + counts[t][i]]
                cur[i] += int(counts[t][i])
            st.push(torch.from_numpy(slot).cuda(), torch.from_numpy(np.array(counts[t], np.int32)).cuda())
        assert st.positions().tolist() == cur == w.fed.tolist()
        good = sa.shuffled([(i, o) for i in range(ss.S) for o in sa.onsets_at(T, cur[i])], [T, 7])
        assert len({i for i, _ in good}) == ss.S
        items = [(0, cur[0] - st.cap - 1)] + good + [(3, -1)]
        ref_y, ref_f = np.zeros((len(items), N), np.int8), np.zeros((len(items), 16, T // 64), np.int8)
        ref_y[1:-1], ref_f[1:-1] = window_rows(C, T, N, good)
        for gc in (1, 3, 0):
            capped(gc)
            y, f, nbad = at_feat(st, items)
            assert nbad == 2, gc
            same(y, ref_y, f"logits, cap {gc}")
            same(f, ref_f, f"features, cap {gc}")
        capped(0)
        y, f = st.windows_at([i for i, _ in good], [o for _, o in good], features=True)
        same(f.cpu().numpy(), ref_f[1:-1], "StreamsEach.windows_at(features=True)")
