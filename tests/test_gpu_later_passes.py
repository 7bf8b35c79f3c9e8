"""The second and later passes of every persistent loop, at every geometry class.

Every forward kernel walks items blockIdx.x, + gridDim.x, ... and much of its code runs only from a
workgroup's second item on: the LDS-DMA prefetch of the trial a grid stride ahead (whose byte
alignment differs from the current trial's whenever C T is no multiple of 4), the last wave
finishing the previous item while the others write the next one's y1 rows, the LDS pads that
setup() zeroes once per workgroup and no item may dirty, the `prev` bookkeeping of gen::item_loop
and the row realignment of the window loop.  With the normal grid (about 512 workgroups) a test
needs more than 512 trials to get there; mibminet_test_grid_cap caps the grid instead, so seven or
eight trials walk one or three workgroups through up to seven passes at any geometry.

Every comparison is byte-exact against the C oracle on the materialised trials, in every row.
Inputs are seeded uniform int8 in [-127, 127] (the float entries get support.dequant of them) or
support.float_recording; int8 sources sit 1-3 bytes into their allocations.
"""
import contextlib
import ctypes

import numpy as np
import pytest

import oracle
from mibminet import lib
from mibminet.params import ParamSet, pack_trials
from support import (_BAD, NTH, SCALE, at_offset, dequant, epochs_of, float_recording, run_entries_on, sliding_windows,
                     tile_sweep, want, windows_at)
from support import capped  # noqa: F401 (a fixture)

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def _uncapped(cap):
    lib.grid_cap(0)
    try:
        yield
    finally:
        lib.grid_cap(cap)


def _set(C, T, N, kw):
    """The parameter set of a geometry: kw as ParamSet.synthetic takes it, or mids = the varying
    out-of-envelope filters of ParamSet.synthetic_extreme."""
    if "mids" in kw:
        return ParamSet.synthetic_extreme(seed=C + 3 * T + N, C=C, T=T, N=N, **kw)
    return ParamSet.synthetic(seed=5 * C + T + N, C=C, T=T, N=N, **kw)


def _load(C, T, N, kw, path="general"):
    ps = _set(C, T, N, kw)
    lib.params_load(ps)
    info = lib.params_info()
    assert info["path"] == path, info
    if "mids" in kw:
        assert info["exact_division"] == (kw["mids"] > 0)
    return ps


def _int8(shape, seed):
    return np.random.default_rng(seed).integers(-127, 128, size=shape, dtype=np.int8)


def _id(v):
    return "-".join(f"{k}={x}" for k, x in v.items()) or "std" if isinstance(v, dict) else str(v)


# ---- the geometry classes -------------------------------------------------------------------------
_SMALLG = 8 * 64 * 16 + 64 * 16 + 7 * 16 * 4 + 16  # sizeof(gen::SmallG)


def _carve(C, T, N, layout):
    """gen::carve_of (forward_gen.hpp) restated: (int8 trials staged in LDS, dynamic LDS bytes) of
    layout 0 time-major, 1 channel-major, 2 float32.  Held to the library below through the LDS
    size that net_launch_info reports."""
    def a16(v):
        return (v + 15) // 16 * 16

    T8 = T // 8
    T64A = (T8 // 8 + 3) & ~3
    NB1, NB2 = (T + 15) // 16, (8 * T8 + 31) // 32
    rest = NB2 % 32
    MT = NB2 // 32 + (1 if rest > 16 else 0)
    NTT = (2 * rest + 15) // 16 if 0 < rest <= 16 else 0
    need = max(32 + 16 * NB1, 1024 * MT + 64, 1024 * MT + 256 * NTT + 112 if NTT else 0)
    y1s = (need + 239) // 256 * 256 + 16
    w5_row = (16 * T64A + 255) // 256 * 256
    y4 = 16 * y1s + 16 * a16(T8 + 32) + a16(16 * (T8 + 3))
    stg = y4 + w5_row + _SMALLG + N * w5_row + a16(4 * N)
    base = stg + (8 * 1024 if layout in (1, 2) else 0)
    chunks = (C * T + 3 + 1023) // 1024
    region = a16(max(1024 * chunks, 16 * NB1 * C + 96, C * T + 16 * NB1 + 96))
    staged = layout in (0, 1) and base + region <= 160 * 1024
    return staged, base + (region if staged else 0)


# C, T, N: (staged, workgroups per CU) of the time-major and of the channel-major kernel, C T mod 4,
# T mod 16 (None: not what the shape is here for)
_CLASSES = {
    (19, 481, 3): ((True, 2), (True, 2), 3, 1),
    (31, 1001, 4): ((True, 2), (True, 2), 3, None),
    (33, 2001, 4): ((True, 1), (True, 1), 1, None),
    (21, 3001, 3): ((True, 1), (True, 1), 1, None),  # 145 and 153 KB of the 160
    (45, 3001, 6): ((False, 2), (False, 1), 1, None),
    (63, 2047, 5): ((False, 2), (False, 2), 1, 15),
    (64, 4096, 16): ((False, 1), (False, 1), 0, 0),
    (1, 64, 1): ((True, 2), (True, 2), 0, 0),
    (5, 100, 16): ((True, 2), (True, 2), 0, 4),
    (64, 513, 2): ((True, 2), (True, 2), 0, 1),
}
_VARIANTS = [dict(weight_bits=4), dict(stress=True), dict(mids=0), dict(mids=3)]
_GEOMETRIES = (tile_sweep() + [(C, T, N, {}) for C, T, N in _CLASSES]
               + [(C, T, N, kw) for C, T, N in ((38, 480, 2), (33, 2001, 4)) for kw in _VARIANTS])
# one workgroup: seven passes and the one that only finishes; three: 3, 3 and 2 items, so the
# prefetch guard and the final break come after different pass counts within one launch
_PASSES = [(1, 7), (3, 8)]


@pytest.mark.parametrize("C,T,N", list(_CLASSES))
def test_geometry_classes(C, T, N, gpu):
    """The shapes of the table are in the classes they were chosen for: staged or not, one or two
    workgroups per CU, C T mod 4 and T mod 16; the library's LDS size agrees with the restatement
    the classes are read from (and the 21 x 3001 shape is within 16 KB of the limit)."""
    tm, ct, ct4, t16 = _CLASSES[(C, T, N)]
    _load(C, T, N, {})
    for layout, (staged, wgs) in enumerate((tm, ct)):
        st, nbytes = _carve(C, T, N, layout)
        assert lib.launch_info(8, channel_major=bool(layout))["lds_bytes"] == nbytes
        assert (st, 2 if nbytes <= 80 * 1024 else 1) == (staged, wgs), (layout, st, nbytes)
    assert C * T % 4 == ct4 and (t16 is None or T % 16 == t16)
    if (C, T) == (21, 3001):
        assert all(145000 <= _carve(C, T, N, layout)[1] <= 160 * 1024 for layout in (0, 1))
    assert {C * T % 4 for C, T, _, _ in tile_sweep()} <= {0, 2}  # why the odd shapes are here


# ---- (a) the cap is honoured ------------------------------------------------------------------------
@pytest.mark.parametrize("C,T,N,path", [(19, 481, 3, "general"), (22, 1125, 4, "float")])
def test_cap_is_honoured(C, T, N, path, capped):
    """net_launch_info[_ct] reports min(B, cap) workgroups under a cap and the former grid after
    grid_cap(0): the pass counts the other tests claim do not rest on a guess at the occupancy."""
    _load(C, T, N, {}, path)
    sizes = (1, 2, 3, 4, 7, 8, 9, 100000)
    free = {(B, cm): lib.launch_info(B, channel_major=cm)["grid"] for B in sizes for cm in (False, True)}
    assert all(free[B, cm] == B for B in sizes[:-1] for cm in (False, True))
    assert all(9 < free[100000, cm] < 100000 for cm in (False, True))
    for cap in (1, 3):
        capped(cap)
        for B, cm in free:
            assert lib.launch_info(B, channel_major=cm)["grid"] == min(B, cap), (cap, B, cm)
    with pytest.raises(lib.NetError):
        capped(-1)
    assert lib.launch_info(8)["grid"] == 3  # a refused value changes nothing
    capped(0)
    assert {k: lib.launch_info(k[0], channel_major=k[1])["grid"] for k in free} == free


# ---- (b), (c) every entry on later passes, capped = uncapped ----------------------------------------
@pytest.mark.parametrize("cap,B", _PASSES)
@pytest.mark.parametrize("C,T,N,kw", _GEOMETRIES, ids=_id)
def test_every_entry_on_later_passes(C, T, N, kw, cap, B, capped):
    """Every forward entry of support.run_entries_on (batched time-major, channel-major and
    float32; windows in both layouts and float32; windows at shuffled onsets; epochs out of a
    wider source, int8 and float32; the single-trial entry) with B trials on `cap` workgroups,
    against the oracle in every row; the three batched entries also byte-identical to their own
    result on the normal grid."""
    ps = _load(C, T, N, kw)
    x = _int8((B, C, T), [C, T, N, B])
    expect = oracle.COracle(ps).batch(pack_trials(x), nthreads=NTH)
    capped(cap)
    for cm in (False, True):
        assert lib.launch_info(B, channel_major=cm)["grid"] == cap
    run_entries_on(f"{C}x{T}x{N} {_id(kw)} cap {cap}", ps, x, expect, again=lambda: _uncapped(cap))
    assert lib.launch_info(B)["grid"] == cap  # the second runs put the cap back


# ---- (d) the compiled kernels ------------------------------------------------------------------------
_COMPILED = [(22, 1125), (64, 1000), (64, 480)]
_COMPILED_SETS = ([(C, T, {}) for C, T in _COMPILED] + [(22, 1125, dict(weight_bits=4))]
                  + [(C, T, dict(mids=3)) for C, T in _COMPILED])


@pytest.mark.parametrize("cap,B", [(1, 9), (4, 9)])
@pytest.mark.parametrize("C,T,kw", _COMPILED_SETS, ids=_id)
def test_compiled_kernels_on_later_passes(C, T, kw, cap, B, capped):
    """The compiled kernels' three entries, nine trials on one workgroup (its DMA ring a trial
    ahead through all nine, the last-trial view met as the ninth trial, not the first) and on four
    (3, 2, 2 and 2 trials), against the oracle."""
    import torch

    ps = _load(C, T, 4, kw, "exact" if "mids" in kw else "float")
    x = _int8((B, C, T), [C, T, B])
    xp = pack_trials(x)
    expect = oracle.COracle(ps).batch(xp, nthreads=NTH)
    capped(cap)
    for cm in (False, True):
        assert lib.launch_info(B, channel_major=cm)["grid"] == cap
    for what, got in (("time-major", lib.forward_torch(torch.from_numpy(xp).cuda())),
                      ("channel-major", lib.forward_ct_torch(at_offset(torch, x, 1))),
                      ("float32", lib.forward_f32_torch(torch.from_numpy(dequant(x)).cuda(), SCALE))):
        np.testing.assert_array_equal(got.cpu().numpy(), expect, err_msg=f"{what}, cap {cap}")


# ---- (e) every row alignment inside one workgroup ----------------------------------------------------
_HOP, _W = 5, 51


@pytest.mark.parametrize("kind", ["ct", "tc", "f32"])
@pytest.mark.parametrize("C,T,N,kw", [(19, 481, 3, {}), (33, 2001, 4, {}), tile_sweep()[16]], ids=_id)
def test_every_row_alignment_in_one_workgroup(C, T, N, kw, kind, capped):
    """Sliding windows at hop 5 on three workgroups: workgroup k sees the onsets 5 (k + 3 p), a
    step of 15 samples, so its consecutive items walk every residue mod 16 (and mod 4) of the
    workspace rows.  Every window against the oracle; nothing written past the W N logits or the
    workspace."""
    import torch

    cap = 3
    ps = _load(C, T, N, kw)
    L = T + 250
    assert lib.windows_count(L, _HOP) == _W
    for k in range(cap):
        onsets = [_HOP * w for w in range(k, _W, cap)]
        assert {o % 16 for o in onsets} == set(range(16)) and all(b - a == 15 for a, b in zip(onsets, onsets[1:]))
    if kind == "f32":
        x, q_ct = float_recording(torch, C, L, 4 * (C % 2), C + T)
    else:
        q_ct = _int8((C, L), [C, T, 5])
        x = at_offset(torch, q_ct if kind == "ct" else q_ct.T, 1 + (C + len(kind)) % 3)
    expect = want(ps, sliding_windows(q_ct, T, _HOP))
    assert expect.shape == (_W, N)
    wsb = lib.windows_workspace(L)
    y = torch.full((_W * N + 64,), 0x5A, dtype=torch.int8, device="cuda")
    ws = torch.full((wsb + 64,), 0x5A, dtype=torch.int8, device="cuda")
    capped(cap)
    if kind == "f32":
        rc = lib.load().net_model_compute_windows_f32(x.data_ptr(), L, _HOP, SCALE, y.data_ptr(), ws.data_ptr(), wsb, 0,
                                                      None)
    else:
        rc = lib.load().net_model_compute_windows(x.data_ptr(), 1 if kind == "ct" else 0, L, _HOP, y.data_ptr(),
                                                  ws.data_ptr(), wsb, 0, None)
    assert rc == lib.NET_OK
    torch.cuda.synchronize()
    assert bool((y[_W * N:] == 0x5A).all()) and bool((ws[wsb:] == 0x5A).all())
    np.testing.assert_array_equal(y[: _W * N].view(_W, N).cpu().numpy(), expect)


# ---- (f) invalid items between passes ---------------------------------------------------------------
_NON = 24
_BAD_AT = [0, 9, 12, 22]  # workgroup 0's first pass, its fourth and fifth, workgroup 1's last
_ENTRIES = ["windows_at-ct", "windows_at-tc", "windows_at-f32", "epochs-i8", "epochs-f32"]
_F_GEOMETRIES = [(19, 481, 3, {}), (31, 1001, 4, {}), tile_sweep()[1]]


def _onsets(last, seed, shift):
    """24 unsorted onsets in 0 .. last, the residue mod 4 stepping by one from each item of a
    workgroup (of three) to its next, those at _BAD_AT replaced by invalid values (support._BAD from
    `shift` on); returns (onsets, the valid indices)."""
    draw = np.random.default_rng(seed).integers(0, last // 4, size=_NON)
    on = [4 * int(v) + (i // 3) % 4 for i, v in enumerate(draw)]
    on[1], on[5] = last, 0
    for j, i in enumerate(_BAD_AT):
        v = _BAD[(j + shift) % len(_BAD)]
        on[i] = last + 1 if v is None else v
    ok = [i for i in range(_NON) if i not in _BAD_AT]
    return on, ok


@pytest.mark.parametrize("entry", _ENTRIES)
@pytest.mark.parametrize("C,T,N,kw", _F_GEOMETRIES, ids=_id)
def test_invalid_items_between_passes(C, T, N, kw, entry, capped):
    """24 onsets on three workgroups, four of them invalid: on a first pass, on two consecutive
    passes of one workgroup and on a last pass.  The invalid rows are exactly N zeros (y is
    prefilled, so that shows at N = 1 too), *n_bad is their count and its neighbours untouched,
    every valid row equals the oracle's and the guard bytes hold."""
    import torch

    cap = 3
    assert [i % cap for i in _BAD_AT] == [0, 0, 0, 1] and _BAD_AT[2] - _BAD_AT[1] == cap
    assert _BAD_AT[0] < cap and _BAD_AT[3] + cap >= _NON
    ps = _load(C, T, N, kw)
    f32 = entry.endswith("f32")
    shift = _ENTRIES.index(entry) + [g[:2] for g in _F_GEOMETRIES].index((C, T))
    y = torch.full((_NON * N + 64,), 0x5A, dtype=torch.int8, device="cuda")
    nb = torch.zeros((3,), dtype=torch.int32, device="cuda")
    if entry.startswith("windows_at"):
        L = T + 137
        last = L - T
        on, ok = _onsets(last, [C, T, 1], shift)
        x_ct = _int8((C, L), [C, T, 6])
        expect = want(ps, windows_at(x_ct, [on[i] for i in ok], T))
        wsb = lib.windows_workspace(L)
        ws = torch.full((wsb + 64,), 0x5A, dtype=torch.int8, device="cuda")
        ond = torch.tensor(on, dtype=torch.int64, device="cuda")
        capped(cap)
        if f32:
            x = at_offset(torch, dequant(x_ct), 4)
            rc = lib.load().net_model_compute_windows_at_f32(x.data_ptr(), L, ond.data_ptr(), _NON, SCALE, y.data_ptr(),
                                                             nb.data_ptr() + 4, ws.data_ptr(), wsb, 0, None)
        else:
            ct = entry.endswith("ct")
            x = at_offset(torch, x_ct if ct else x_ct.T, 1 + shift % 3)
            rc = lib.load().net_model_compute_windows_at(x.data_ptr(), 1 if ct else 0, L, ond.data_ptr(), _NON,
                                                         y.data_ptr(), nb.data_ptr() + 4, ws.data_ptr(), wsb, 0, None)
    else:
        R, L = C + 3, T + 137  # odd rows: the alignment of an epoch's rows differs from row to row
        channels = [int(c) for c in np.random.default_rng([C, T, 2]).permutation(R)[:C]]
        channels[C // 2] = R - 1
        last = R * L - ((R - 1) * L + T)  # n_elems - span
        on, ok = _onsets(last, [C, T, 3], shift)
        src = _int8((R, L), [C, T, 7])
        expect = want(ps, epochs_of(src, [on[i] for i in ok], channels, L, T))
        ond = torch.tensor(on, dtype=torch.int64, device="cuda")
        tab = (ctypes.c_int32 * C)(*channels)
        capped(cap)
        if f32:
            x = at_offset(torch, dequant(src), 4)
            rc = lib.load().net_model_compute_epochs_f32(x.data_ptr(), x.numel(), L, tab, ond.data_ptr(), _NON, SCALE,
                                                         y.data_ptr(), nb.data_ptr() + 4, 0, None)
        else:
            x = at_offset(torch, src, 1 + shift % 3)
            rc = lib.load().net_model_compute_epochs(x.data_ptr(), x.numel(), L, tab, ond.data_ptr(), _NON, y.data_ptr(),
                                                     nb.data_ptr() + 4, 0, None)
        ws, wsb = None, 0
    # the onsets: unsorted, every alignment among each workgroup's valid ones, and the invalid
    # values whose low 32 bits would be valid among them over the entries
    valid = [on[i] for i in ok]
    assert valid != sorted(valid) and all(0 <= v <= last for v in valid) and {0, last} <= set(valid)
    assert all(len({on[i] % 4 for i in ok if i % cap == k}) >= 3 for k in range(cap))
    assert all(not 0 <= on[i] <= last for i in _BAD_AT)
    assert rc == lib.NET_OK
    torch.cuda.synchronize()
    assert nb.cpu().tolist() == [0, len(_BAD_AT), 0]
    assert bool((y[_NON * N:] == 0x5A).all()) and (ws is None or bool((ws[wsb:] == 0x5A).all()))
    rows = y[: _NON * N].view(_NON, N).cpu().numpy()
    assert not rows[_BAD_AT].any()
    np.testing.assert_array_equal(rows[ok], expect)
