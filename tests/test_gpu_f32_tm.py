"""Float32 sample-major frames on the GPU (the _f32_tm entries, gen::l1_fetch<F32TM>) and, with them,
sets widened over the whole cap (net_blob_widen).

The geometries cover each class of the K-slot mapping (image_layout.hpp, l1_chunk) with small T:
C = 1 (every slot but one reads a neighbour), 8 (one chunk), 19 (the g >> 1 pairs), 33 (the first of
three chunks), 38, 49 and 64.  Four sessions under sets (0, 1, 1, 2) of a bank of three with the
scales 0.5, 3 and 7.25; their samples are floats that the set's scale quantises back to a known int8
array (support.dequant's construction), as tests/test_gpu_streams.py builds its float case.  Where
only a wrong K-slot or a wrong tail would see them, non-finite values are planted: channel C - 1 of
the last sample of every push's chunk and channel 0 of the first of the next (in [S][n][C] that is
also the last float of one session's chunk and the first of the next session's), the first and last
samples of the whole array, and the unused tail of an each-group's slot.  Arrays lie 4 bytes off a
16-byte boundary and no length is a multiple of 16.

The reference of every byte is the C oracle on the two-pass quantisation (net_quantize_input_f32)
of the same samples, never the code under test; that the sibling _f32 entry gives the same bytes on
the transposed array is a second assertion.  Every comparison is byte equality."""
import functools

import numpy as np
import pytest

import support_streams as ss
import support_windows_bank as swb
from mibminet import lib
from mibminet.params import ParamSet
from support import capped, dev, same_rows, sliding_windows, want, windows_at  # noqa: F401 (capped: a fixture)

pytestmark = pytest.mark.gpu

GEOMETRIES = [(1, 64, 1), (8, 64, 2), (19, 480, 3), (33, 64, 2), (38, 480, 2), (49, 64, 2), (64, 480, 2)]
SETS = (0, 1, 1, 2)
NS = len(SETS)
SCALES = (0.5, 3.0, 7.25)
HOP, MAX_PUSH = ss.HOP, ss.MAX_PUSH
NAN, INF = float("nan"), float("inf")
S_, X_ = ParamSet.synthetic, ParamSet.synthetic_extreme


# ---- inputs and references, once per geometry -----------------------------------------------------
def floats_of(q, scale):
    """float32 samples that the input quantiser with `scale` maps back to the int8 array q (the
    middle of each value's interval, as support.dequant)."""
    v = np.arange(-127, 128)
    lut = ((v + 0.5 * np.sign(v)) * (scale / 127.0)).astype(np.float32)
    return lut[np.asarray(q, np.int16) + 127]


def plant(x_tc, ends):
    """Non-finite floats in [L][C] frames: channel C - 1 of sample e - 1 and channel 0 of sample e for
    every e of `ends`, and the first and last frames' outer channels."""
    L, C = x_tc.shape
    kinds = (NAN, INF, -INF)
    for i, e in enumerate(ends):
        if 0 < e < L:
            x_tc[e - 1, C - 1] = kinds[i % 3]
            x_tc[e, 0] = kinds[(i + 1) % 3]
    x_tc[0, 0], x_tc[0, C - 1], x_tc[L - 1, 0], x_tc[L - 1, C - 1] = NAN, -INF, INF, NAN


def two_pass(x_ct, scale):
    """The two-pass quantisation (net_quantize_input_f32) of float32 [C][L] (NumPy) -> int8 [C][L]."""
    import torch

    C, L = x_ct.shape
    q = lib.quantize_input_torch(torch.from_numpy(np.array(x_ct, order="C")[None]).cuda(), scale)
    return np.ascontiguousarray(q.cpu().numpy()[0, : L * C].reshape(L, C).T)


def make_sets(C, T, N, variant=None):
    if variant == "exact":
        return tuple(X_(seed=221 + i, C=C, T=T, N=N, mids=3) for i in range(3))
    kw = dict(reorder_bn=False) if variant == "plain-bn" else {}
    return tuple(S_(seed=211 + i, C=C, T=T, N=N, **kw) for i in range(3))


@functools.lru_cache(maxsize=None)
def frames(C, T):
    """[NS][L][C] float32, L = the schedule's total: every session's frames, non-finite values planted
    at every push boundary.  Read-only."""
    L = ss.total(T)
    q = np.random.default_rng([C, T, 5]).integers(-127, 128, size=(NS, C, L), dtype=np.int8)
    x = np.stack([floats_of(q[i], SCALES[s]).T for i, s in enumerate(SETS)])
    ends = np.cumsum(ss.schedule(T)).tolist()
    for i in range(NS):
        plant(x[i], ends)
    x = np.ascontiguousarray(x)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def reference(C, T, N, variant=None):
    """(sets, q [NS][C][L] int8: the two-pass quantisation of frames(C, T) under each session's scale,
    rows: [NS] arrays [W][N], the oracle's logits of every sliding window of every session)."""
    sets = make_sets(C, T, N, variant)
    x = frames(C, T)
    q = np.stack([two_pass(x[i].T, SCALES[s]) for i, s in enumerate(SETS)])
    rows = [ss.rows_of(sets[s], q[i], T) for i, s in enumerate(SETS)]
    return sets, q, rows


# ---- 1. windows and windows-at: y and every workspace byte --------------------------------------------
@pytest.mark.parametrize("C,T,N", GEOMETRIES)
def test_windows_and_windows_at(C, T, N, gpu):
    import torch

    sets, q, _ = reference(C, T, N)
    L = T + 53  # 5 mod 16
    x_tc, qs, ps = frames(C, T)[0, :L], q[0, :, :L], sets[0]
    y1 = np.zeros((16, lib.windows_row_stride(L)), np.int8)
    y1[:, :L] = swb.layer1_of(ps, qs)
    xd = dev(torch, x_tc)
    assert xd.data_ptr() % 16 == 4 and L % 16
    xct = dev(torch, np.ascontiguousarray(x_tc.T))
    lib.params_load(ps)
    try:
        y, ws = lib.forward_windows_f32_torch(xd, HOP, SCALES[0], layout="tc", return_y1=True)
        same_rows(y.cpu().numpy(), want(ps, sliding_windows(qs, T, HOP)), "windows")
        np.testing.assert_array_equal(ws.cpu().numpy(), y1)
        ys, wss = lib.forward_windows_f32_torch(xct, HOP, SCALES[0], return_y1=True)
        assert torch.equal(y, ys) and torch.equal(ws, wss)
        # any order, a duplicate, the last valid onset
        onsets = [L - T, 0, 7, 7, 1, L - T - 2]
        y, ws = lib.forward_windows_at_torch(xd, onsets, layout="tc", scale=SCALES[0], return_y1=True)
        same_rows(y.cpu().numpy(), want(ps, windows_at(qs, onsets, T)), "windows at")
        np.testing.assert_array_equal(ws.cpu().numpy(), y1)
        ys, wss = lib.forward_windows_at_torch(xct, onsets, scale=SCALES[0], return_y1=True)
        assert torch.equal(y, ys) and torch.equal(ws, wss)
        # the int8 time-major entry on the two-pass quantisation
        yq, wsq = lib.forward_windows_at_torch(torch.from_numpy(np.ascontiguousarray(qs.T)).cuda(), onsets, layout="tc",
                                               return_y1=True)
        assert torch.equal(y, yq) and torch.equal(ws, wsq)
    finally:
        lib.params_unload()


# ---- 2. windows through a bank: per-block scales, a gap block ---------------------------------------------
@pytest.mark.parametrize("C,T,N", GEOMETRIES)
def test_windows_bank_with_a_gap_block(C, T, N, gpu):
    """Recording A (session 0, set 0) with its pad, one gap block (-1) of non-finite junk, recording B
    (session 3, set 2): each block's samples are quantised with its set's scale."""
    import torch

    sets, _, _ = reference(C, T, N)
    fr = frames(C, T)
    la, lb = T + 21, T + 6
    sa = (la + 15) // 16 * 16
    sb_ = sa + 16
    L = sb_ + lb
    x = np.random.default_rng([C, T, 6]).standard_normal((L, C)).astype(np.float32) * 4.0  # the pads: junk
    x[:la], x[sb_:] = fr[0, :la], fr[3, :lb]
    x[sa:sb_] = np.resize(np.array([NAN, INF, -INF, 1e30], np.float32), (16, C))
    blk = np.full((L + 15) // 16, 2, np.int32)
    blk[: sa // 16], blk[sa // 16] = 0, -1
    on = {0: list(range(0, la - T + 1, HOP)), 2: [sb_ + o for o in range(0, lb - T + 1, HOP)]}
    onsets = on[0] + on[2]
    ws_want = np.zeros((16, lib.windows_row_stride(L)), np.int8)
    expect = {}
    for s in (0, 2):
        qs = two_pass(x.T, SCALES[s])
        y1 = swb.layer1_of(sets[s], qs)
        for b in np.flatnonzero(blk == s):
            ws_want[:, 16 * b: min(16 * b + 16, L)] = y1[:, 16 * b: min(16 * b + 16, L)]
        expect[s] = want(sets[s], windows_at(qs, on[s], T))
    assert L % 16 and len(on[0]) == 8 and len(on[2]) == 3
    with lib.Bank(sets, SCALES) as bank:
        blk_d = torch.from_numpy(blk).cuda()
        y, ws = lib.forward_windows_bank_torch(bank, dev(torch, x), blk_d, onsets, layout="tc", return_y1=True)
        same_rows(y.cpu().numpy(), np.concatenate([expect[0], expect[2]]), "bank windows")
        np.testing.assert_array_equal(ws.cpu().numpy(), ws_want)
        ys, wss = lib.forward_windows_bank_torch(bank, dev(torch, np.ascontiguousarray(x.T)), blk_d, onsets,
                                                 return_y1=True)
        assert torch.equal(y, ys) and torch.equal(ws, wss)


# ---- 3. uniform streams over the schedule, the grid capped and not ---------------------------------------
def run_uniform(torch, st, x, layout):
    """Pushes frames x [NS][L][C] by the schedule, every chunk 4 bytes off a 16-byte boundary; returns
    [NS][W][N]."""
    T = st.bank.dims.T
    out, pos = [], 0
    for n in ss.schedule(T):
        chunk = np.ascontiguousarray(x[:, pos: pos + n] if layout == "tc" else x[:, pos: pos + n].transpose(0, 2, 1))
        y, nbad = st.push_f32(dev(torch, chunk), layout=layout)
        out.append(y)
        pos += n
    assert int(nbad.item()) == 0 and st.info()[4] == pos == x.shape[1]
    return torch.cat(out, dim=1).cpu().numpy()


def check_rings(st, sets, q, ref=None):
    """Every ring holds, twice, the oracle's layer 1 of the last cap samples; `ref`: the sibling's group."""
    c, L = st.cap, q.shape[2]
    t = np.arange(max(0, L - c), L)
    for i, s in enumerate(SETS):
        ring = lib.streams_ring(st, i)
        np.testing.assert_array_equal(ring[:, :c], ring[:, c:], err_msg=f"the two copies, session {i}")
        np.testing.assert_array_equal(ring[:, t % c], swb.layer1_of(sets[s], q[i][:, t]), err_msg=f"session {i}")
        if ref is not None:
            np.testing.assert_array_equal(ring, lib.streams_ring(ref, i), err_msg=f"the sibling's ring, session {i}")


@pytest.mark.parametrize("cap", [1, 3, 0])
@pytest.mark.parametrize("C,T,N", GEOMETRIES)
def test_uniform_streams_over_the_schedule(C, T, N, cap, capped):
    import torch

    sets, q, rows = reference(C, T, N)
    x = frames(C, T)
    capped(cap)
    with lib.Bank(sets, SCALES) as bank, lib.Streams(bank, SETS, HOP, MAX_PUSH) as st:
        got = run_uniform(torch, st, x, "tc")
        for i in range(NS):
            same_rows(got[i], rows[i], f"session {i}")
        if cap == 0:  # the sibling on the transposed chunks: the same rows, the same rings
            with lib.Streams(bank, SETS, HOP, MAX_PUSH) as sib:
                assert np.array_equal(run_uniform(torch, sib, x, "ct"), got)
                check_rings(st, sets, q, sib)
        else:
            check_rings(st, sets, q)


# ---- 4. each-groups: ragged counts, the slot's tail --------------------------------------------------------
def ragged(T, seed):
    """[ticks][NS] counts in 0 .. MAX_PUSH with 0 and MAX_PUSH in every tick's row or the next, until
    every session was fed T + 40 samples or more."""
    rng = np.random.default_rng([T, seed])
    out, fed = [], np.zeros(NS, np.int64)
    while fed.min() < T + 40:
        c = rng.integers(1, MAX_PUSH + 1, size=NS)
        c[len(out) % NS] = MAX_PUSH
        c[(len(out) + 1) % NS] = 0 if len(out) % 3 == 0 else c[(len(out) + 1) % NS]
        out.append(c)
        fed += c
    return np.array(out)


def slots(x, cur, counts, layout):
    """[NS][MAX_PUSH][C] (or its "ct" transpose): session i's next counts[i] frames, the rest of the slot
    non-finite."""
    NSx, _, C = x.shape
    slot = np.resize(np.array([NAN, -INF, INF], np.float32), (NSx, MAX_PUSH, C)).copy()
    for i, n in enumerate(counts):
        slot[i, :n] = x[i, cur[i]: cur[i] + n]
    return np.ascontiguousarray(slot if layout == "tc" else slot.transpose(0, 2, 1))


def run_each(torch, st, x, counts, layout):
    """Feeds the ticks of `counts`; returns ([NS] lists of row arrays, the samples fed per session)."""
    cur, got = [0] * NS, [[] for _ in range(NS)]
    for row in counts.tolist():
        cnt = torch.tensor(row, dtype=torch.int32, device="cuda")
        y, cout, nbad = st.push_f32(dev(torch, slots(x, cur, row, layout)), cnt, layout=layout)
        yh, ch = y.cpu().numpy(), cout.cpu().tolist()
        assert int(nbad.item()) == 0
        for i in range(NS):
            got[i].append(yh[i, : ch[i]])
            cur[i] += row[i]
    return [np.concatenate(g) for g in got], cur


@pytest.mark.parametrize("C,T,N", GEOMETRIES)
def test_each_streams_with_ragged_counts(C, T, N, capped):
    import torch

    sets, q, rows = reference(C, T, N)
    x = frames(C, T)
    counts = ragged(T, 1)
    assert (counts == 0).any() and (counts == MAX_PUSH).any() and counts.sum(0).max() <= x.shape[1]
    capped(3)
    with lib.Bank(sets, SCALES) as bank, lib.StreamsEach(bank, SETS, HOP, MAX_PUSH) as st, \
            lib.StreamsEach(bank, SETS, HOP, MAX_PUSH) as sib:
        got, fed = run_each(torch, st, x, counts, "tc")
        assert st.positions().tolist() == fed
        for i in range(NS):
            W = ss.windows_count(T, fed[i], HOP)
            assert W > 0
            same_rows(got[i], rows[i][:W], f"session {i}")
        capped(0)
        sgot, _ = run_each(torch, sib, x, counts, "ct")
        for i in range(NS):
            assert np.array_equal(got[i], sgot[i])
            np.testing.assert_array_equal(lib.streams_ring(st, i), lib.streams_ring(sib, i))


def test_each_push_replayed_from_a_captured_graph(gpu):
    """Eager pushes until every session holds T samples, then one push captured on a side stream (which
    runs nothing) and replayed once on fresh frames: the rows are the oracle's."""
    import torch

    C, T, N = 19, 480, 3
    sets, q, rows = reference(C, T, N)
    x = frames(C, T)
    with lib.Bank(sets, SCALES) as bank, lib.StreamsEach(bank, SETS, HOP, MAX_PUSH) as st:
        n0 = T + 5
        cur = [0] * NS
        for a in range(0, n0, MAX_PUSH):
            row = [min(MAX_PUSH, n0 - a)] * NS
            st.push_f32(dev(torch, slots(x, cur, row, "tc")), torch.tensor(row, dtype=torch.int32, device="cuda"),
                        layout="tc")
            cur = [c + n for c, n in zip(cur, row)]
        row = [MAX_PUSH, 0, 17, 1]
        kmax = st.rows(MAX_PUSH)
        xs = dev(torch, np.zeros((NS, MAX_PUSH, C), np.float32))
        cin = torch.zeros((NS,), dtype=torch.int32, device="cuda")
        y = torch.full((NS, kmax, N), 0x5A, dtype=torch.int8, device="cuda")
        cout = torch.zeros((NS,), dtype=torch.int32, device="cuda")
        nb = torch.zeros((1,), dtype=torch.int32, device="cuda")
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(s):
            with torch.cuda.graph(g, stream=s):
                assert lib.load().net_streams_push_each_f32_tm(st.handle, xs.data_ptr(), cin.data_ptr(), MAX_PUSH,
                                                               y.data_ptr(), cout.data_ptr(), None, nb.data_ptr(),
                                                               s.cuda_stream) == lib.NET_OK
        torch.cuda.synchronize()
        assert st.positions().tolist() == cur  # the capture ran nothing
        xs.copy_(torch.from_numpy(slots(x, cur, row, "tc")))
        cin.copy_(torch.tensor(row, dtype=torch.int32))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        yh, ch = y.cpu().numpy(), cout.cpu().tolist()
        del g
        assert nb.item() == 0 and st.positions().tolist() == [c + n for c, n in zip(cur, row)]
        for i in range(NS):
            w0, w1 = ss.windows_count(T, cur[i], HOP), ss.windows_count(T, cur[i] + row[i], HOP)
            assert ch[i] == w1 - w0
            same_rows(yh[i, : ch[i]], rows[i][w0:w1], f"session {i}")
            assert (yh[i, ch[i]:] == 0x5A).all()
        assert ch[0] > 0 and ch[1] == 0


# ---- 5. the build variants ---------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["exact", "plain-bn"])
def test_variants(variant, capped):
    import torch

    C, T, N = 19, 480, 3
    sets, q, rows = reference(C, T, N, variant)
    x = frames(C, T)
    with lib.Bank(sets, SCALES) as bank, lib.Streams(bank, SETS, HOP, MAX_PUSH) as st:
        assert bank.exact_division == (variant == "exact")
        got = run_uniform(torch, st, x, "tc")
        for i in range(NS):
            same_rows(got[i], rows[i], f"{variant}, session {i}")
        check_rings(st, sets, q)
    L = T + 53
    lib.params_load(sets[2])
    try:
        assert lib.params_info()["exact_division"] == (variant == "exact")
        y, ws = lib.forward_windows_f32_torch(dev(torch, x[3, :L]), HOP, SCALES[2], layout="tc", return_y1=True)
        same_rows(y.cpu().numpy(), rows[3][: ss.windows_count(T, L, HOP)], variant)
        np.testing.assert_array_equal(ws.cpu().numpy()[:, :L], swb.layer1_of(sets[2], q[3][:, :L]))
        assert not ws.cpu().numpy()[:, L:].any()
    finally:
        lib.params_unload()


# ---- 6. refusals -------------------------------------------------------------------------------------------
def test_refusals_leave_everything_as_it_was(gpu):
    """A misaligned float x, a bank without scales, and each kind of group at the other's entry:
    NET_ERR_INVALID before anything is enqueued; the group's position, counters and rings stay."""
    import torch

    C, T, N = 8, 64, 2
    sets, q, _ = reference(C, T, N)
    x = frames(C, T)
    A, INV = lib.load(), lib.NET_ERR_INVALID
    L = T + 53
    xd = dev(torch, x[0, :L])
    ws = torch.zeros((16, lib.windows_row_stride(L)), dtype=torch.int8, device="cuda")
    y = torch.full((64, N), 0x5A, dtype=torch.int8, device="cuda")
    on = torch.zeros((4,), dtype=torch.int64, device="cuda")
    blk = torch.zeros(((L + 15) // 16,), dtype=torch.int32, device="cuda")
    cnt = torch.full((NS,), 5, dtype=torch.int32, device="cuda")
    cout = torch.full((NS,), -7, dtype=torch.int32, device="cuda")
    nb = torch.zeros((1,), dtype=torch.int32, device="cuda")
    xp, yp, wp, op, bp = xd.data_ptr(), y.data_ptr(), ws.data_ptr(), on.data_ptr(), nb.data_ptr()
    lib.params_load(sets[0])
    try:
        with lib.Bank(sets, SCALES) as bank, lib.Bank(sets) as bare:
            for p, b in ((xp + 2, bank), (xp + 1, bank), (xp, bare)):  # misaligned; no scales
                if b is bank:
                    assert A.net_model_compute_windows_f32_tm(p, L, HOP, 3.0, yp, wp, ws.numel(), 0, None) == INV
                    assert A.net_model_compute_windows_at_f32_tm(p, L, op, 4, 3.0, yp, bp, wp, ws.numel(), 0, None) == INV
                assert A.net_model_compute_windows_bank_f32_tm(b.handle, p, L, blk.data_ptr(), op, 4, yp, bp, wp,
                                                               ws.numel(), 0, None) == INV
                with lib.Streams(b, SETS, HOP, MAX_PUSH) as st, lib.StreamsEach(b, SETS, HOP, MAX_PUSH) as ea:
                    if b is bank:  # something in the rings first
                        st.push_f32(dev(torch, np.ascontiguousarray(x[:, :5])), layout="tc")
                        ea.push_f32(dev(torch, slots(x, [0] * NS, [5] * NS, "tc")), cnt, layout="tc")
                    torch.cuda.synchronize()
                    before = ([lib.streams_ring(g, i) for g in (st, ea) for i in range(NS)], st.info(), ea.info(),
                              ea.positions().tolist())
                    assert A.net_streams_push_f32_tm(st.handle, p, 5, yp, bp, None) == INV
                    assert A.net_streams_push_each_f32_tm(ea.handle, p, cnt.data_ptr(), MAX_PUSH, yp, cout.data_ptr(), None,
                                                          bp, None) == INV
                    # each kind of group refuses the other's entry, whatever else is right
                    assert A.net_streams_push_f32_tm(ea.handle, xp, 5, yp, bp, None) == INV
                    assert A.net_streams_push_each_f32_tm(st.handle, xp, cnt.data_ptr(), MAX_PUSH, yp, cout.data_ptr(), None,
                                                          bp, None) == INV
                    if b is bare:
                        for layout in ("tc", "ct"):
                            with pytest.raises(ValueError):
                                st.push_f32(xd[None, :5].expand(NS, 5, C).contiguous(), layout=layout)
                    torch.cuda.synchronize()
                    after = ([lib.streams_ring(g, i) for g in (st, ea) for i in range(NS)], st.info(), ea.info(),
                             ea.positions().tolist())
                    assert before[1:] == after[1:] and all(np.array_equal(a, c) for a, c in zip(before[0], after[0]))
            # the scale's domain and a NULL bank, as the siblings
            assert A.net_model_compute_windows_f32_tm(xp, L, HOP, 0.0, yp, wp, ws.numel(), 0, None) == INV
            assert A.net_model_compute_windows_f32_tm(xp, L, HOP, 2.0 ** 61, yp, wp, ws.numel(), 0, None) == lib.NET_ERR_RANGE
            assert A.net_model_compute_windows_bank_f32_tm(None, xp, L, blk.data_ptr(), op, 4, yp, bp, wp, ws.numel(), 0,
                                                           None) == INV
            assert A.net_streams_push_f32_tm(None, xp, 5, yp, bp, None) == INV
        torch.cuda.synchronize()
        assert bool((y == 0x5A).all()) and not ws.any() and nb.item() == 0 and cout.tolist() == [-7] * NS
        for bad in (xd[:, :4], xd.to(torch.float64), xd.cpu()):  # the Python entries: shape, type, place
            with pytest.raises(ValueError):
                lib.forward_windows_f32_torch(bad, HOP, 3.0, layout="tc")
        with pytest.raises(ValueError):
            lib.forward_windows_f32_torch(xd, HOP, 3.0, layout="xx")
    finally:
        lib.params_unload()


# ---- 7. the two halves together: widened sets on frames of the whole cap ----------------------------------
def test_widened_sets_on_frames_of_the_whole_cap(capped):
    """Three sets of 19, 19 and 38 channels widened to R = 64 with distinct maps share one bank and one
    stream group; the frames are float [S][n][64], the unselected electrodes random and non-finite.
    Each session's rows are the oracle's under its ORIGINAL set on the two-pass quantisation of its
    gathered channels."""
    import torch

    T, N, R = 480, 3, 64
    orig = (S_(seed=231, C=19, T=T, N=N), S_(seed=232, C=19, T=T, N=N), S_(seed=233, C=38, T=T, N=N))
    maps = [[int(c) for c in np.random.default_rng([R, 40 + i]).permutation(R)[: ps.dims.C]] for i, ps in enumerate(orig)]
    assert maps[0] != maps[1]
    L = ss.total(T)
    rng = np.random.default_rng([R, T, 8])
    x = (rng.standard_normal((3, L, R)) * 2.0).astype(np.float32)
    x[rng.random(x.shape) < 0.05] = NAN
    x[rng.random(x.shape) < 0.05] = -INF
    expect = []
    for i, ps in enumerate(orig):
        qi = rng.integers(-127, 128, size=(ps.dims.C, L), dtype=np.int8)
        x[i][:, maps[i]] = floats_of(qi, SCALES[i]).T
        keep = x[i][:, maps[i]].copy()
        plant(x[i], np.cumsum(ss.schedule(T)).tolist())  # columns 0 and 63 at every push boundary ...
        x[i][1:-1, maps[i]] = keep[1:-1]  # ... which a selected electrode sees in the first and last frame only
        expect.append(ss.rows_of(ps, two_pass(np.ascontiguousarray(x[i][:, maps[i]].T), SCALES[i]), T))
    wide = [orig[0].widened(R, maps[0]), lib.blob_widen(orig[1].to_blob(), R, maps[1]), orig[2].widened(R, maps[2])]
    with lib.Bank(wide, SCALES) as bank, lib.Streams(bank, (0, 1, 2), HOP, MAX_PUSH) as st:
        assert bank.info()[:4] == [3, R, T, N]
        out, pos = [], 0
        for n in ss.schedule(T):
            y, nbad = st.push_f32(dev(torch, np.ascontiguousarray(x[:, pos: pos + n])), layout="tc")
            out.append(y)
            pos += n
        got = torch.cat(out, dim=1).cpu().numpy()
        assert int(nbad.item()) == 0
        for i in range(3):
            same_rows(got[i], expect[i], f"session {i}")
