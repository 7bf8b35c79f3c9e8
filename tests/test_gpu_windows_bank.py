"""Windows through a bank on the GPU (net_model_compute_windows_bank[_f32], forward_bank.hpp): seven
recordings laid along time at multiples of 16 samples, each under its own set of a bank of five, and
their sliding windows in one call.

The reference of every row is the C oracle of the window's set on the materialised window
(support_windows_bank.table, computed once per geometry), never another GPU entry, and every
comparison is byte-exact.  tests/test_windows_bank_cpu.py certifies the inputs: no row is all zeros,
the five sets' rows differ pairwise on every window, and swapping any one layer's parameters between
the sets of neighbouring recordings changes at least 75 % of a set's windows, so a window or a sample
that ran any layer on a neighbour's state shows.  Under lib.grid_cap(1) one workgroup walks every
switch of the window list and, in layer 1, one workgroup's four waves walk every change of blk_set.
"""
import numpy as np
import pytest

import support_bank as sb
import support_windows_bank as swb
from mibminet import lib
from mibminet.params import ParamSet
from oracle import golden_np as G
from support import _BAD, CAPS, at_offset, capped, want, windows_at  # noqa: F401 (capped: a fixture)
from support_bank import banks  # noqa: F401 (a fixture)

pytestmark = pytest.mark.gpu


_WS = {}


def _workspace(C, T, N):
    """support_windows_bank.workspace of the geometry's case, computed once."""
    if (C, T, N) not in _WS:
        x, _, _, blk_set, _, _, _ = swb.case(C, T)
        _WS[(C, T, N)] = swb.workspace(sb.sets(C, T, N), x, blk_set)
        _WS[(C, T, N)].setflags(write=False)
    return _WS[(C, T, N)]


def _call(bank, x, layout, L, blk_set, onsets, f32=False):
    """The C entry on a prefilled logits buffer, a counter between two guards and a workspace with a
    guard behind it: (rows [W][N], the three counters, ws [16][row_stride]).  Nothing past the W N
    logits or the workspace may be written."""
    import torch

    W, N = len(onsets), bank.dims.N
    rs = lib.windows_row_stride(L)
    y = torch.full((W * N + 64,), 0x5A, dtype=torch.int8, device="cuda")
    ws = torch.full((16 * rs + 64,), 0x5A, dtype=torch.int8, device="cuda")
    nb = torch.zeros((3,), dtype=torch.int32, device="cuda")
    ond = torch.tensor([int(o) for o in onsets], dtype=torch.int64, device="cuda")
    bsd = torch.tensor([int(s) for s in blk_set], dtype=torch.int32, device="cuda")
    assert len(blk_set) == (L + 15) // 16
    A = lib.load()
    tail = (L, bsd.data_ptr(), ond.data_ptr(), W, y.data_ptr(), nb.data_ptr() + 4, ws.data_ptr(), 16 * rs, 0, None)
    if f32:
        rc = A.net_model_compute_windows_bank_f32(bank.handle, x.data_ptr(), *tail)
    else:
        rc = A.net_model_compute_windows_bank(bank.handle, x.data_ptr(), 1 if layout == "ct" else 0, *tail)
    assert rc == lib.NET_OK, rc
    torch.cuda.synchronize()
    assert bool((y[W * N:] == 0x5A).all()) and bool((ws[16 * rs:] == 0x5A).all())
    return y[: W * N].view(W, N).cpu().numpy(), nb.cpu().tolist(), ws[: 16 * rs].view(16, rs).cpu().numpy()


def _placed(torch, x, layout, offset):
    return at_offset(torch, x if layout == "ct" else np.ascontiguousarray(x.T), offset)


# ---- every window of every recording ----------------------------------------------------------------
@pytest.mark.parametrize("layout", ["ct", "tc"])
@pytest.mark.parametrize("C,T,N", swb.GEOMETRIES)
def test_all_windows(C, T, N, layout, banks, capped):
    import torch

    bank, tab = banks(C, T, N), swb.table(C, T, N)
    x, starts, L, blk_set, onsets, first, set_of = swb.case(C, T)
    expect, y1 = swb.reference(tab, set_of), _workspace(C, T, N)
    for offset in range(4):
        xd = _placed(torch, x, layout, offset)
        for cap in CAPS:
            capped(cap)
            rows, nb, ws = _call(bank, xd, layout, L, blk_set, onsets)
            assert nb == [0, 0, 0], (offset, cap)
            np.testing.assert_array_equal(rows, expect, err_msg=f"offset {offset}, cap {cap}")
            # layer 1 of every sample under its block's set, the pad samples between the recordings
            # included (their blocks belong to the recording before them), zeros from L on
            np.testing.assert_array_equal(ws[:, :L], y1[:, :L], err_msg=f"workspace, offset {offset}, cap {cap}")
            assert not ws[:, L:].any()
    assert bank.device_copies() == 1
    # the recordings do have pads, and a pad block takes the set of the recording before it
    ends = [int(starts[r]) + T + swb.DELTAS[r] for r in range(6)]
    padded = [r for r in range(6) if ends[r] % 16]
    assert len(padded) >= 4 and all(ends[r] < starts[r + 1] and blk_set[ends[r] >> 4] == swb.SETS[r] for r in padded)


# ---- gap blocks -------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,T,N", swb.GEOMETRIES)
def test_gap_blocks_are_zero_and_touch_nothing_else(C, T, N, banks, capped):
    """blk_set entries outside the bank: those 16-byte columns of the workspace are zero, every other
    block is what it was, and the windows that touch no such block are answered as before."""
    import torch

    bank, tab = banks(C, T, N), swb.table(C, T, N)
    x, starts, L, blk_set, onsets, first, set_of = swb.case(C, T)
    nblk = len(blk_set)
    bs = np.array(blk_set)
    # the first block, two in a row inside recording 3, the block before a boundary, the partial last one
    gaps = {0: -1, int(starts[3] >> 4) + 2: bank.n_sets, int(starts[3] >> 4) + 3: 2**31 - 1,
            int(starts[5] >> 4) - 1: -(2**31), nblk - 1: -1}
    for b, v in gaps.items():
        bs[b] = v
    y1 = np.array(_workspace(C, T, N))
    for b in gaps:
        y1[:, 16 * b: 16 * b + 16] = 0
    clear = [i for i, o in enumerate(onsets) if not any(int(o) >> 4 <= b <= (int(o) + T - 1) >> 4 for b in gaps)]
    assert 0 < len(clear) < len(onsets)
    capped(1)
    rows, nb, ws = _call(bank, at_offset(torch, x, 1), "ct", L, bs, onsets[clear])
    assert nb == [0, 0, 0]
    np.testing.assert_array_equal(ws, y1)
    np.testing.assert_array_equal(rows, swb.reference(tab, set_of)[clear])


# ---- invalid windows around switches and range ends -------------------------------------------------
# the base list: windows of the case by index, and at 6 a window that crosses from recording 1 into
# recording 2 (both set 1).  Sets 0 0 0 0 0 | 1 1 | 3 x 7 | 4 x 4 | 0 0 0 | 2 2 2: switches at 5, 7, 14,
# 18 and 21; with three workgroups the ranges are [0, 8), [8, 16) and [16, 24).
_BASE = [0, 1, 2, 3, 4, 6, "cross11", 7, 8, 9, 10, 11, 12, 13, 20, 21, 22, 23, 24, 25, 26, 30, 31, 32]
# 0: first of a range, before any set is there; 4: directly before a switch; 7: directly after one
# and last of a range; 8: first of a range (with 7, two in a row across a range end: the switch to
# set 3 moves to 9); 15: last of a range; 16, 17: two in a row from a range's start; 23: last of all.  "bad": an onset of support._BAD; "cross": starts in
# one recording and ends in a neighbour of another set; "gap": starts in a gap block; "gap-end": ends
# in one
_BAD_AT = {0: "bad", 4: "cross01", 7: "gap", 8: "bad", 15: "gap-end", 16: "cross34", 17: "bad", 23: "bad"}


@pytest.mark.parametrize("C,T,N", swb.GEOMETRIES)
def test_invalid_windows(C, T, N, banks, capped):
    import torch

    bank, tab = banks(C, T, N), swb.table(C, T, N)
    x, starts, L, blk_set, onsets, first, set_of = swb.case(C, T)
    sets = sb.sets(C, T, N)
    shift = swb.GEOMETRIES.index((C, T, N))
    cross11 = int(starts[2]) - T // 2  # ends in recording 2, before the gap block below
    g = (int(starts[2]) + T - 20) >> 4  # a block of recording 2 (set 1, no window of its own) made a gap
    assert 16 * g > cross11 + T - 1 and 16 * g + 15 < int(starts[3]) and blk_set[g] == 1
    bs = np.array(blk_set)
    bs[g] = -1
    special = {"cross11": cross11, "cross01": int(starts[1]) - T // 2, "cross34": int(starts[4]) - 7, "gap": 16 * g + 1,
               "gap-end": 16 * g + 5 - (T - 1)}
    assert bs[special["cross01"] >> 4] == 0 and bs[(special["cross01"] + T - 1) >> 4] == 1
    assert bs[special["cross34"] >> 4] == 3 and bs[(special["cross34"] + T - 1) >> 4] == 4
    assert bs[special["gap-end"] >> 4] == 1 and (special["gap-end"] + T - 1) >> 4 == g
    assert all(0 <= v <= L - T for v in special.values())
    on, so, expect = [], [], np.zeros((len(_BASE), N), np.int8)
    for i, b in enumerate(_BASE):
        if b == "cross11":
            on.append(cross11)
            so.append(1)
            expect[i] = want(sets[1], windows_at(x, [cross11], T))[0]
        else:
            on.append(int(onsets[b]))
            so.append(int(set_of[b]))
            expect[i] = tab[set_of[b], b]
    assert [i for i in range(1, 24) if so[i] != so[i - 1]] == [5, 7, 14, 18, 21] and expect.any(axis=1).all()
    for j, (i, what) in enumerate(sorted(_BAD_AT.items())):
        if what == "bad":
            v = _BAD[(j + shift) % len(_BAD)] if i != 23 else None
            on[i] = L - T + 1 if v is None else v
        else:
            on[i] = special[what]
    ok = [i for i in range(len(_BASE)) if i not in _BAD_AT]
    xd = at_offset(torch, x, 3)
    for cap in CAPS:
        capped(cap)
        rows, nb, _ = _call(bank, xd, "ct", L, bs, on)
        assert nb == [0, len(_BAD_AT), 0], cap
        assert not rows[sorted(_BAD_AT)].any(), cap
        np.testing.assert_array_equal(rows[ok], expect[ok], err_msg=f"cap {cap}")
    # the Python entry counts them and says what they are
    bsd = torch.from_numpy(bs).cuda()
    with pytest.raises(ValueError, match="8 of 24 onsets lie outside the recording or the bank"):
        lib.forward_windows_bank_torch(bank, xd, bsd, on)
    got = lib.forward_windows_bank_torch(bank, xd, bsd, on, check=False).cpu().numpy()
    np.testing.assert_array_equal(got[ok], expect[ok])


# ---- the build variants -----------------------------------------------------------------------------
@pytest.mark.parametrize("variant", list(sb.VARIANTS))
@pytest.mark.parametrize("C,T,N", sb.VARIANT_GEOMETRIES)
def test_variants(C, T, N, variant, capped):
    import torch

    sets = sb.VARIANTS[variant](C, T, N)
    x, starts, L, blk_set, onsets, first, set_of = swb.case(C, T)
    wins = windows_at(x, onsets, T)
    expect = np.zeros((len(onsets), N), np.int8)
    for s in set(swb.SETS):
        at = np.flatnonzero(set_of == s)
        expect[at] = want(sets[s], wins[at])
    xd = at_offset(torch, x, 2)
    with lib.Bank(sets) as bank:
        assert bank.exact_division == (variant in sb.EXACT)
        for layout, cap in (("ct", 1), ("ct", 0), ("tc", 1)):
            capped(cap)
            rows, nb, _ = _call(bank, xd if layout == "ct" else _placed(torch, x, "tc", 2), layout, L, blk_set, onsets)
            assert nb == [0, 0, 0]
            np.testing.assert_array_equal(rows, expect, err_msg=f"{variant} {layout} cap {cap}")


# ---- float32 input, one scale per set ---------------------------------------------------------------
_SCALES = [0.5, 1.3, 3.0, 7.25, 100.0]


def _dequant(q, scale):
    """support.dequant's construction for `scale`: the middle of each int8 value's interval."""
    v = np.arange(-127, 128)
    lut = ((v + 0.5 * np.sign(v)) * (scale / 127.0)).astype(np.float32)
    assert np.array_equal(G.quantize_to_int(lut, scale), v)
    return lut[np.asarray(q, np.int16) + 127]


@pytest.mark.parametrize("C,T,N", [(19, 480, 3), (22, 1125, 4), (64, 480, 2)])
def test_float32_with_five_scales(C, T, N, capped):
    """Every sample holds the float that its block's scale quantises to the int8 sample, with
    non-finite samples planted as support.float_recording plants them.  The reference is
    golden_np.quantize_to_int of each recording's samples with its set's scale, then the oracle.
    quantize_to_int is undefined on NaN (it casts one to an integer), so the four NaN samples take
    what the two-pass quantiser (net_quantize_input_f32, pinned over every bit pattern by
    tests/test_gpu_f32.py) gives them."""
    import torch

    sets = sb.sets(C, T, N)
    x, starts, L, blk_set, onsets, first, set_of = swb.case(C, T)
    scale_of = np.repeat(np.array(_SCALES, np.float32)[blk_set], 16)[:L]
    xf = np.zeros((C, L), np.float32)
    for s in range(5):
        cols = np.flatnonzero(scale_of == np.float32(_SCALES[s]))
        xf[:, cols] = _dequant(x[:, cols], _SCALES[s])
    xd = at_offset(torch, xf, 4)
    xd[0, :7] = torch.tensor([float("nan"), float("inf"), -float("inf"), 3.0, -3.0, 0.0, -0.0])
    xd[C - 1, L - 3:] = torch.tensor([float("nan"), -float("inf"), float("inf")])
    at = int(starts[4]) + 5  # inside recording 4, and the last sample before recording 5's first
    xd[C // 2, at: at + 3] = torch.tensor([float("inf"), float("nan"), -1e30])
    xd[1, int(starts[5]) - 1] = float("nan")
    xh = xd.cpu().numpy()
    nan = np.isnan(xh)
    assert nan.sum() == 4
    q = np.zeros((C, L), np.int64)
    for s in range(5):
        cols = np.flatnonzero(scale_of == np.float32(_SCALES[s]))
        q[:, cols] = G.quantize_to_int(np.where(nan[:, cols], np.float32(0), xh[:, cols]), np.float32(_SCALES[s]))
    planted = np.zeros((C, L), bool)
    planted[0, :7] = planted[C - 1, L - 3:] = planted[C // 2, at: at + 3] = planted[1, int(starts[5]) - 1] = True
    assert np.array_equal(q[~planted], x[~planted])  # the construction, where nothing is planted
    for c, t in zip(*np.nonzero(nan)):
        one = lib.quantize_input_torch(xd[c: c + 1, t: t + 1].reshape(1, 1, 1).clone(), float(scale_of[t]))
        q[c, t] = int(one.cpu().numpy()[0, 0])
    q = q.astype(np.int8)
    wins = windows_at(q, onsets, T)
    expect = np.zeros((len(onsets), N), np.int8)
    for s in set(swb.SETS):
        idx = np.flatnonzero(set_of == s)
        expect[idx] = want(sets[s], wins[idx])
    y1 = swb.workspace(sets, q, blk_set)
    with lib.Bank(sets, _SCALES) as bank, lib.Bank(sets) as bare:
        for cap in (1, 0):
            capped(cap)
            rows, nb, ws = _call(bank, xd, "ct", L, blk_set, onsets, f32=True)
            assert nb == [0, 0, 0]
            np.testing.assert_array_equal(rows, expect, err_msg=f"cap {cap}")
            np.testing.assert_array_equal(ws[:, :L], y1[:, :L], err_msg=f"workspace, cap {cap}")
            assert not ws[:, L:].any()
        bsd = torch.from_numpy(np.array(blk_set)).cuda()
        np.testing.assert_array_equal(lib.forward_windows_bank_torch(bank, xd, bsd, onsets).cpu().numpy(), expect)
        with pytest.raises(ValueError):
            lib.forward_windows_bank_torch(bare, xd, bsd, onsets)  # no scales
        fn = lib.load().net_model_compute_windows_bank_f32
        assert fn(bare.handle, xd.data_ptr(), L, 16, 16, 1, 16, None, 16, 2**40, 0, None) == lib.NET_ERR_INVALID
        assert bare.device_copies() == 0


# ---- the bank's life beside the loaded set ----------------------------------------------------------
def test_calls_around_a_load_of_another_geometry(gpu):
    """A call with no set loaded, net_params_load of another geometry, a second call: both results
    are correct, the loaded set computes what it did and its digest stays, and the bank adds nothing
    to the device's cache of loaded sets."""
    import torch

    C, T, N = 19, 480, 3
    x, starts, L, blk_set, onsets, first, set_of = swb.case(C, T)
    expect = swb.reference(swb.table(C, T, N), set_of)
    xd = at_offset(torch, x, 1)
    lib.params_unload()
    with lib.Bank(sb.sets(C, T, N)) as bank:
        rows, _, _ = _call(bank, xd, "ct", L, blk_set, onsets)  # no set is loaded
        np.testing.assert_array_equal(rows, expect)
        assert lib.device_images() == 0 and bank.device_copies() == 1 and lib.params_dims() == {}
        other = ParamSet.synthetic(seed=7, C=8, T=64, N=2)
        lib.params_load(other)
        trials = sb.epochs(8, 64)[:5]
        loaded = lib.forward_ct_torch(torch.from_numpy(np.array(trials)).cuda()).cpu().numpy()
        np.testing.assert_array_equal(loaded, want(other, trials))
        images, digest, info = lib.device_images(), lib.image_digest(), lib.params_info()
        rows, _, _ = _call(bank, xd, "ct", L, blk_set, onsets[::-1])
        np.testing.assert_array_equal(rows, expect[::-1])
        assert (lib.device_images(), lib.image_digest(), lib.params_info(), bank.device_copies()) == (images, digest, info, 1)
        assert lib.params_dims()["T"] == 64
        again = lib.forward_ct_torch(torch.from_numpy(np.array(trials)).cuda()).cpu().numpy()
        np.testing.assert_array_equal(again, loaded)
    lib.params_unload()


def test_two_banks_alive_at_once(banks, gpu):
    import torch

    a, b = (19, 480, 3), (64, 480, 2)
    for _ in range(2):
        for C, T, N in (a, b):
            x, starts, L, blk_set, onsets, first, set_of = swb.case(C, T)
            rows, nb, _ = _call(banks(C, T, N), at_offset(torch, x, 0), "ct", L, blk_set, onsets)
            np.testing.assert_array_equal(rows, swb.reference(swb.table(C, T, N), set_of))


def test_graph_capture_and_replay(gpu):
    """After one eager call the entry allocates nothing and does not wait: captured once on a side
    stream and replayed on other onset lists."""
    import torch

    C, T, N = 22, 1125, 4
    x, starts, L, blk_set, onsets, first, set_of = swb.case(C, T)
    expect = swb.reference(swb.table(C, T, N), set_of)
    xd = at_offset(torch, x, 1)
    bsd = torch.from_numpy(np.array(blk_set)).cuda()
    ond = torch.from_numpy(np.array(onsets)).cuda()
    order = np.random.default_rng(5).permutation(len(onsets))
    with lib.Bank(sb.sets(C, T, N)) as bank:
        lib.forward_windows_bank_torch(bank, xd, bsd, ond)  # uploads the bank
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            with torch.cuda.graph(g, stream=s):
                y = lib.forward_windows_bank_torch(bank, xd, bsd, ond, stream=s, check=False)
        for idx in (order, np.arange(len(onsets))[::-1].copy()):
            ond.copy_(torch.from_numpy(np.array(onsets)[idx]))
            g.replay()
            torch.cuda.synchronize()
            np.testing.assert_array_equal(y.cpu().numpy(), expect[idx])
        del g  # the graph goes before the bank it reads


# ---- the Python entry over a list of recordings -----------------------------------------------------
@pytest.mark.parametrize("layout", ["ct", "tc"])
@pytest.mark.parametrize("C,T,N", [(8, 64, 2), (22, 1125, 4)])
def test_python_multi_entry(C, T, N, layout, banks):
    """forward_windows_multi_bank_torch on the recordings alone (it lays them at the aligned starts
    itself, zero pads between them): rows first[r] .. first[r + 1] - 1 are the oracle's of recording
    r's windows under sets[r].  Split into chunks by a small max_bytes, the same rows."""
    import torch

    bank = banks(C, T, N)
    x, starts, L, blk_set, onsets, first, set_of = swb.case(C, T)
    expect = swb.reference(swb.table(C, T, N), set_of)
    lens = swb.lengths(T)
    recs = [_placed(torch, x[:, int(starts[r]): int(starts[r]) + lens[r]], layout, r % 4) for r in range(len(lens))]
    y, f = lib.forward_windows_multi_bank_torch(bank, recs, swb.SETS, swb.HOP, layout=layout)
    assert list(f) == first.tolist()
    np.testing.assert_array_equal(y.cpu().numpy(), expect)
    for r in range(len(lens)):
        rows = y[f[r]: f[r + 1]].cpu().numpy()
        assert len(rows) == (0 if lens[r] < T else (lens[r] - T) // swb.HOP + 1)
        np.testing.assert_array_equal(rows, expect[int(first[r]): int(first[r + 1])])
    per = max(16, C)
    y2, f2 = lib.forward_windows_multi_bank_torch(bank, recs, swb.SETS, swb.HOP, layout=layout,
                                                  max_bytes=per * (2 * (T + 60) + 40))
    assert list(f2) == first.tolist()
    np.testing.assert_array_equal(y2.cpu().numpy(), expect)
