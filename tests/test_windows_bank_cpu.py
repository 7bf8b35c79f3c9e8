"""Windows through a bank without a GPU (net_model_compute_windows_bank[_f32],
net_bank_windows_starts, net_bank_windows_lists): the layout and list helpers against a NumPy
restatement, every argument check of the two entries in the documented order (each call here fails
a check or has no window, so nothing is launched), what the Python entries reject, the
certification of the inputs tests/test_gpu_windows_bank.py uses, and the helpers' arithmetic in a
stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer."""
import ctypes

import numpy as np
import pytest

import support_bank as sb
import support_windows_bank as swb
from mibminet import lib
from support import run_host_program, want, windows_at

INV, OK = lib.NET_ERR_INVALID, lib.NET_OK
C, T, N = 22, 1125, 4


@pytest.fixture(scope="module")
def banks():
    lib.params_unload()  # no entry below may need a loaded set
    with lib.Bank(sb.sets(C, T, N), [1.0] * 5) as five, lib.Bank(sb.sets(C, T, N)[:1]) as bare:
        yield five, bare


# ---- the helpers ------------------------------------------------------------------------------------
def _c_lists(bank, lens, sets, hop, n_blk=None, cap=None, fill=0x5A):
    R = len(lens)
    A = lib.load()
    arr, sarr = (ctypes.c_size_t * max(R, 1))(*lens), (ctypes.c_int32 * max(R, 1))(*sets)
    starts = np.full(R + 1, fill, np.int64)
    L = A.net_bank_windows_starts(arr, R, starts.ctypes.data)
    W = A.net_bank_windows_lists(bank.handle, arr, sarr, R, hop, None, 0, None, 0, None)
    nb = (L + 15) // 16
    n_blk, cap = nb if n_blk is None else n_blk, W if cap is None else cap
    blk = np.full(n_blk + 1, fill, np.int32)
    on = np.full(cap + 1, fill, np.int64)
    first = (ctypes.c_size_t * (R + 1))(*([fill] * (R + 1)))
    got = A.net_bank_windows_lists(bank.handle, arr, sarr, R, hop, blk.ctypes.data, n_blk, on.ctypes.data, cap, first)
    return L, W, got, starts, blk, on, np.array(list(first), np.int64)


@pytest.mark.parametrize("lens,sets", [(swb.lengths(T), swb.SETS), ([T + 5], (3,)), ([T - 1], (0,)), ([16, 0, T], (1, 2, 1))])
@pytest.mark.parametrize("hop", [1, 3, 500])
def test_helpers_equal_their_restatement(banks, lens, sets, hop):
    five, _ = banks
    starts, L, blk_set, onsets, first = swb.layout(lens, sets, T, hop)
    cL, W, got, cstarts, blk, on, cfirst = _c_lists(five, lens, sets, hop)
    assert (cL, W, got) == (L, len(onsets), len(onsets))
    np.testing.assert_array_equal(cstarts[:-1], starts)
    np.testing.assert_array_equal(blk[:-1], blk_set)
    np.testing.assert_array_equal(on[:-1], onsets)
    np.testing.assert_array_equal(cfirst, first)
    assert cstarts[-1] == blk[-1] == on[-1] == 0x5A  # nothing past the ends
    assert (starts % 16 == 0).all() and len(blk_set) == (L + 15) // 16
    # the Python wrapper returns the same
    p = lib.bank_windows_lists(five, lens, sets, hop)
    assert p[1] == L
    for a, b in zip((p[0], p[2], p[3], p[4]), (starts, blk_set, onsets, first)):
        np.testing.assert_array_equal(a, b)
        assert a.dtype == b.dtype


def test_the_certified_case_is_the_one_described():
    starts, L, blk_set, onsets, first = swb.layout(swb.lengths(64), swb.SETS, 64, swb.HOP)
    assert L == 591 and len(onsets) == swb.W and first.tolist() == [0, 6, 7, 7, 20, 24, 30, 41]
    # hop 3 from aligned starts: every onset residue mod 4, and all but 7, 10 and 13 mod 16
    assert {int(o) % 4 for o in onsets} == set(range(4)) and len({int(o) % 16 for o in onsets}) == 13


def test_a_capacity_one_short_writes_nothing(banks):
    five, _ = banks
    lens, sets = swb.lengths(T), swb.SETS
    _, L, blk_set, onsets, first = swb.layout(lens, sets, T, 3)
    _, W, got, _, blk, on, cfirst = _c_lists(five, lens, sets, 3, n_blk=len(blk_set) - 1)
    assert got == W and (blk == 0x5A).all()
    np.testing.assert_array_equal(on[:-1], onsets)
    _, W, got, _, blk, on, cfirst = _c_lists(five, lens, sets, 3, cap=W - 1)
    assert got == W and (on == 0x5A).all()
    np.testing.assert_array_equal(blk[:-1], blk_set)
    np.testing.assert_array_equal(cfirst, first)


def test_refusals_return_zero_and_write_nothing(banks):
    five, _ = banks
    A = lib.load()
    ok = ([T + 9, T + 20], (0, 4), 3)
    for lens, sets, hop in (([T + 9, T + 20], (0, 4), 0), ([T + 9, T + 20], (0, 5), 3), ([T + 9, T + 20], (-1, 0), 3),
                            ([2**64 - 8, 8], (0, 1), 3), ([2**63 - 1, 1], (0, 1), 3), ([2**63], (0,), 3)):
        _, W, got, _, blk, on, first = _c_lists(five, lens, sets, hop, n_blk=300, cap=300)
        assert (W, got) == (0, 0), (lens, sets, hop)
        assert (blk == 0x5A).all() and (on == 0x5A).all() and (first == 0x5A).all()
    arr, sarr = (ctypes.c_size_t * 2)(*ok[0]), (ctypes.c_int32 * 2)(*ok[1])
    assert A.net_bank_windows_lists(None, arr, sarr, 2, 3, None, 0, None, 0, None) == 0  # a NULL bank
    assert A.net_bank_windows_lists(five.handle, arr, sarr, 0, 3, None, 0, None, 0, None) == 0
    assert A.net_bank_windows_lists(five.handle, arr, sarr, 2, 3, None, 0, None, 0, None) == 4 + 7
    assert A.net_bank_windows_starts(arr, 0, None) == 0
    assert A.net_bank_windows_starts((ctypes.c_size_t * 2)(2**63 - 8, 0), 2, None) == 0  # the rounding overflows
    assert A.net_bank_windows_starts((ctypes.c_size_t * 1)(2**63 - 1), 1, None) == 2**63 - 1
    for bad in (lambda: lib.bank_windows_lists(five, [T], [0, 1], 3), lambda: lib.bank_windows_lists(five, [T], [5], 3),
                lambda: lib.bank_windows_lists(five, [T], [0], 0), lambda: lib.bank_windows_lists(None, [T], [0], 3),
                lambda: lib.bank_windows_lists(five, [2**63], [0], 3), lambda: lib.bank_windows_lists(five, [], [], 3)):
        with pytest.raises(ValueError):
            bad()


# ---- the entry checks, in their documented order ----------------------------------------------------
def test_entry_checks_without_a_gpu(banks):
    five, bare = banks
    i8, f32 = lib.load().net_model_compute_windows_bank, lib.load().net_model_compute_windows_bank_f32
    L, W = 4000, 9
    wsb = lib.windows_workspace(L)
    keep = np.zeros(256, np.uint8)
    ws = (keep.ctypes.data + 15) // 16 * 16
    x, y, on, nb, bs = ws + 16, ws + 32, ws + 48, ws + 64, ws + 80  # never read: every call fails a check or has W == 0
    good = (five.handle, x, 1, L, bs, on, W, y, nb, ws, wsb, 0, None)
    names = ("bank", "x", "layout", "L", "bs", "on", "W", "y", "nb", "ws", "wsb", "dev", "st")

    def call(fn=i8, **kw):
        a = dict(zip(names, good))
        a.update(kw)
        if fn is f32:
            del a["layout"]
        return fn(*a.values())

    for fn in (i8, f32):
        # 1. a NULL bank, where NET_ERR_NO_PARAMS stands in the windows-at entries: before everything
        assert call(fn, bank=None) == INV and call(fn, bank=None, W=0) == INV
        # 2. the windows-at checks, with the bank's C and T
        assert call(fn, x=None) == INV and call(fn, y=None) == INV and call(fn, on=None) == INV and call(fn, ws=None) == INV
        for off in (1, 2, 3):
            assert call(fn, y=y + off) == INV and call(fn, nb=nb + off) == INV
            assert call(fn, y=y + off, W=0) == INV and call(fn, nb=nb + off, W=0) == INV
        for off in (1, 2, 4, 7):
            assert call(fn, on=on + off) == INV and call(fn, on=on + off, W=0) == INV
        for off in (1, 4, 8):
            assert call(fn, ws=ws + off) == INV and call(fn, ws=ws + off, W=0) == INV
        assert call(fn, wsb=wsb - 1) == INV and call(fn, wsb=0, W=0) == INV
        assert call(fn, L=T - 1, W=1, wsb=2**40) == INV and call(fn, L=0, W=1) == INV  # W > 0 with L < T (the bank's T)
        assert call(fn, W=2**31 - 65535) == INV and call(fn, W=2**40) == INV
        assert call(fn, dev=-1) == INV and call(fn, dev=1 << 20) == INV and call(fn, dev=-1, W=0) == INV
        per = 22 * (4 if fn is f32 else 1)  # the bank's C
        big = -(-2**31 // per)
        for Lb in (big, 2**31, 2**40, 2**63):
            assert call(fn, L=Lb, wsb=2**62) == INV and call(fn, L=Lb, wsb=2**62, W=0) == INV
        assert call(fn, L=big - 1, wsb=2**62, W=0) == OK
        # 3. blk_set: NULL with W > 0, misaligned for any W
        assert call(fn, bs=None) == INV and call(fn, bs=None, W=0) == OK
        for off in (1, 2, 3):
            assert call(fn, bs=bs + off) == INV and call(fn, bs=bs + off, W=0) == INV
        # an earlier check answers first: with a bad device and a bad blk_set both are INVALID, so the
        # order shows where the later check would have let W == 0 through
        assert call(fn, bs=None, dev=-1, W=0) == INV
        # 5. no window: NET_OK, nothing touched, whatever x, y and the lists are
        assert call(fn, W=0) == OK and call(fn, x=None, y=None, on=None, nb=None, bs=None, W=0) == OK
        assert call(fn, x=None, y=None, on=None, nb=None, bs=None, ws=None, wsb=0, L=0, W=0) == OK
    for layout in (2, 3, -1):
        assert call(layout=layout) == INV and call(layout=layout, W=0) == INV
    assert call(layout=0, W=0) == OK
    for off in (1, 2, 3):
        assert call(x=x + off, W=0) == OK                              # int8: any byte alignment
        assert call(f32, x=x + off) == INV and call(f32, x=x + off, W=0) == INV  # float32: 4 bytes
    assert call(f32, x=x + 4, W=0) == OK
    # 4. the float entry on a bank without scales, after blk_set's checks and before W == 0
    assert call(f32, bank=bare.handle) == INV and call(f32, bank=bare.handle, W=0) == INV
    assert call(bank=bare.handle, W=0) == OK
    assert five.device_copies() == 0 and bare.device_copies() == 0
    assert lib.params_dims() == {}  # no set was needed, none appeared


def test_fewer_than_sixteen_channels_take_the_workspace_limit():
    """C < 16: the workspace rows (16 bytes per sample over the 16 filters) set the limit, from the
    bank's C."""
    lib.params_unload()
    keep = np.zeros(128, np.uint8)
    ws = (keep.ctypes.data + 15) // 16 * 16
    with lib.Bank(sb.sets(4, 4096, 16)[:2]) as bank:
        fn = lib.load().net_model_compute_windows_bank
        assert fn(bank.handle, ws, 1, 2**27, ws, ws, 0, ws, None, ws, 2**62, 0, None) == INV
        assert fn(bank.handle, ws, 1, 2**27 - 1, ws, ws, 0, ws, None, ws, 2**62, 0, None) == OK
        assert bank.device_copies() == 0


def test_python_entries_reject_what_the_abi_cannot_see(banks):
    import torch

    five, bare = banks
    x = torch.zeros((C, 4000), dtype=torch.int8)
    bs = torch.zeros((250,), dtype=torch.int32)
    xf = torch.zeros((C, 4000), dtype=torch.float32)
    for bad in (lambda: lib.forward_windows_bank_torch(five, x, bs, [0]),                       # not on the device
                lambda: lib.forward_windows_bank_torch(five, np.zeros((C, 4000), np.int8), bs, [0]),
                lambda: lib.forward_windows_bank_torch(None, x, bs, [0]),
                lambda: lib.forward_windows_bank_torch(five, torch.zeros((C + 1, 4000), dtype=torch.int8), bs, [0]),  # C
                lambda: lib.forward_windows_bank_torch(five, x, bs, [0], layout="tc"),          # [L][C] wanted
                lambda: lib.forward_windows_bank_torch(five, x, bs, [0], layout="cl"),
                lambda: lib.forward_windows_bank_torch(bare, xf, bs, [0]),                      # no scales
                lambda: lib.forward_windows_multi_bank_torch(five, [x, x], [0], 3),             # sets of the wrong length
                lambda: lib.forward_windows_multi_bank_torch(five, [x], [0], 3),                # not on the device
                lambda: lib.forward_windows_multi_bank_torch(five, [], [], 3),
                lambda: lib.forward_windows_multi_bank_torch(five, [torch.zeros((C - 1, 4000), dtype=torch.int8)], [0], 3),
                lambda: lib.forward_windows_multi_bank_torch(bare, [xf], [0], 3),
                lambda: lib.forward_windows_multi_bank_torch(five, [x], [0], 0),
                lambda: lib.forward_windows_multi_bank_torch(sb.sets(C, T, N)[0], [x], [0], 3)):
        with pytest.raises(ValueError):
            bad()


# ---- certification of the GPU tests' inputs ---------------------------------------------------------
@pytest.mark.parametrize("C,T,N", swb.GEOMETRIES)
def test_inputs_are_certified(C, T, N):
    """A condition on the inputs of tests/test_gpu_windows_bank.py, not a measurement.  No window's row
    under its own set (or any set) is all zeros, which is what an invalid window writes; the five
    sets' rows differ pairwise on every window; and for every ordered pair (a, b) of sets whose
    recordings are neighbours and each layer k, set a with layer k's arrays taken from b changes at
    least 75 % of set a's windows (tests/test_bank_cpu.py's threshold): a kernel that ran any layer
    of a window, layer 1 of its samples included, on a neighbouring recording's state cannot pass."""
    x, _, _, _, onsets, _, set_of = swb.case(C, T)
    sets, tab = sb.sets(C, T, N), swb.table(C, T, N)
    assert tab.shape == (5, swb.W, N) and tab.any(axis=2).all()
    assert swb.reference(tab, set_of).any(axis=1).all()
    for a in range(5):
        for b in range(a):
            assert (tab[a] != tab[b]).any(axis=1).all(), (a, b)
    pairs = swb.adjacent_pairs()
    assert len(pairs) == 10
    for a, b in pairs:
        mine = np.flatnonzero(set_of == a)
        wins = windows_at(x, onsets[mine], T)
        for k in range(1, 6):
            changed = (want(sb.hybrid(sets[a], sets[b], k), wins) != tab[a][mine]).any(axis=1)
            assert changed.mean() >= 0.75, (a, b, k, float(changed.mean()))


# ---- the helpers' arithmetic under the sanitizers ---------------------------------------------------
def test_list_arithmetic_runs_clean_under_sanitizers(tmp_path):
    """tests/windows_bank_host_main.cpp includes only csrc/bank_host.hpp, is built with the host C++
    compiler and run as an ordinary child process: lengths near SIZE_MAX and INT64_MAX, R = 0, every
    list in an array of exactly its size.  Any sanitizer report, failed check or compile error fails."""
    stdout = run_host_program("windows_bank_host_main.cpp", [], tmp_path)
    assert stdout.splitlines() == ["cases 41"], stdout
