"""A wider montage (net_blob_widen, ParamSet.widened; no GPU): the set whose layer-1 weight column
channels[c] is the original's column c, zeros elsewhere, over R source rows.

The guarantee is held against the C oracle, never against the library: on random int8 u[R][T] the
widened set's layer-1 rows and logits equal the original's on u[channels].  So that a widen which
ignored the map could not pass, each case also asserts that the oracle's logit rows under the true
map differ from its rows under the map 0 .. C-1 in at least 23 of the 24 trials (the seeds below were
picked so that they do; the count is printed).  Then: the Python and the C transform byte-equal, every
refusal code, the size query, the int4 round trip, net_params_info before and after, and a bank of a
19- and a 38-channel set, which agree on C only once both are widened to 64."""
import ctypes

import numpy as np
import pytest

import oracle
from mibminet import lib
from mibminet.params import ParamSet, pack_trials
from support import NTH

S, X = ParamSet.synthetic, ParamSet.synthetic_extreme
B = 24  # trials per case

# (name, the original set, R, seed of the map and the input)
CASES = [
    ("19->64", lambda: S(seed=31, C=19, T=480, N=3), 64, 1),
    ("8->13", lambda: S(seed=32, C=8, T=64, N=2), 13, 2),
    ("22->64 plain-BN", lambda: S(seed=33, C=22, T=1125, N=4, reorder_bn=False), 64, 3),
    ("4->5 int4", lambda: S(seed=34, C=4, T=64, N=2, weight_bits=4), 5, 4),
    ("38->64 balanced clip", lambda: S(seed=35, C=38, T=480, N=2, clip_balanced=True), 64, 5),
    ("64->64 permutation", lambda: S(seed=36, C=64, T=480, N=4), 64, 6),
]
IDS = [c[0] for c in CASES]


def channel_map(C, R, seed):
    """C distinct rows of R in no order, and never the map 0 .. C-1."""
    ch = np.random.default_rng([seed, 99]).permutation(R)[:C]
    assert not np.array_equal(ch, np.arange(C))
    return [int(c) for c in ch]


def logits(ps, x):
    return oracle.COracle(ps).batch(pack_trials(x), nthreads=NTH)


@pytest.mark.parametrize("name,make,R,seed", CASES, ids=IDS)
def test_widened_set_equals_the_original_on_the_gathered_rows(name, make, R, seed):
    ps = make()
    d = ps.dims
    ch = channel_map(d.C, R, seed)
    wide = ps.widened(R, ch)
    assert wide.dims.C == R and wide.dims == type(d)(C=R, T=d.T, F1=d.F1, F2=d.F2, D=d.D, N=d.N)
    u = np.random.default_rng([seed, 7]).integers(-128, 128, size=(B, R, d.T)).astype(np.int8)
    want = logits(ps, u[:, ch])
    assert np.array_equal(logits(wide, u), want), name
    # layer 1, the only layer whose parameters changed, on one trial; every later field is shared
    y1 = oracle.COracle(ps).layer1(oracle.to_tc_align(u[0][ch], d.C_ALIGN))
    assert np.array_equal(oracle.COracle(wide).layer1(oracle.to_tc_align(u[0], wide.dims.C_ALIGN)), y1), name
    for f in ("l1_factor", "l1_offset", "l2_factor", "l2_offset", "l2_weight_reverse", "l3_weight", "l4_factor",
              "l4_offset", "l4_weight", "l5_bias", "l5_weight"):
        assert np.array_equal(getattr(wide, f), getattr(ps, f)), f
    assert (wide.l3_factor, wide.l5_factor, wide.weight_bits, wide.flags) == (ps.l3_factor, ps.l5_factor, ps.weight_bits,
                                                                             ps.flags)
    # a widen that ignored the map would give the rows of channels 0 .. C-1: those differ
    naive = logits(ps, u[:, : d.C])
    differ = int((naive != want).any(1).sum())
    print(f"{name}: {differ} of {B} trials differ under the map 0 .. C-1")
    assert differ >= B - 1, (name, differ)


@pytest.mark.parametrize("name,make,R,seed", CASES, ids=IDS)
def test_python_and_c_transforms_are_byte_equal(name, make, R, seed):
    ps = make()
    ch = channel_map(ps.dims.C, R, seed)
    blob = ps.to_blob()
    wide = lib.blob_widen(blob, R, ch)
    assert wide == ps.widened(R, ch).to_blob(), name
    # everything but the header's C and the layer-1 weight section is the input's bytes
    at = 64 + 8 * ps.dims.F2
    old = ps.dims.F2 * ps.dims.C_ALIGN * ps.weight_bits // 8
    new = ps.dims.F2 * ((R + 3) // 4 * 4) * ps.weight_bits // 8
    assert len(wide) == len(blob) - old + new
    assert wide[:12] == blob[:12] and wide[16:at] == blob[16:at] and wide[at + new:] == blob[at + old:]
    assert int.from_bytes(wide[12:16], "little") == R


def test_int4_widened_set_survives_the_blob_round_trip():
    ps = S(seed=34, C=4, T=64, N=2, weight_bits=4)
    wide = ps.widened(5, [4, 0, 3, 1])
    back = ParamSet.from_blob(wide.to_blob())
    assert back.dims == wide.dims and back.weight_bits == 4
    assert np.array_equal(back.l1_weight_align, wide.l1_weight_align)
    assert np.array_equal(back.l1_weight_align[:, [4, 0, 3, 1]], ps.w1()) and not back.l1_weight_align[:, 2].any()
    assert back.to_blob() == wide.to_blob() == lib.blob_widen(ps.to_blob(), 5, [4, 0, 3, 1])


def _widen(blob, R, ch, cap=None, want_out=True, null_channels=False):
    """net_blob_widen through ctypes: (rc, out_len, the output bytes)."""
    L = lib.load()
    src = ctypes.create_string_buffer(bytes(blob), len(blob))
    arr = None if null_channels else (ctypes.c_int32 * 64)(*ch, *([-1] * (64 - len(ch))))
    n = ctypes.c_size_t(12345)
    cap = len(blob) + 4096 if cap is None else cap
    out = ctypes.create_string_buffer(b"\xAA" * (cap + 8), cap + 8) if want_out else None
    rc = L.net_blob_widen(src, len(blob), R, arr, out, cap, ctypes.byref(n))
    return rc, n.value, None if out is None else out.raw


def test_refusals_and_the_size_query():
    INV, BLOB = lib.NET_ERR_INVALID, lib.NET_ERR_BLOB
    ps = S(seed=32, C=8, T=64, N=2)
    blob, ch = ps.to_blob(), [12, 0, 5, 3, 9, 1, 7, 2]
    good = ps.widened(13, ch).to_blob()
    # the size query: out == NULL writes the size only; with the size exactly, the bytes and nothing past them
    rc, need, _ = _widen(blob, 13, ch, cap=0, want_out=False)
    assert (rc, need) == (lib.NET_OK, len(good))
    rc, n, out = _widen(blob, 13, ch, cap=need)
    assert (rc, n) == (lib.NET_OK, need) and out[:need] == good and out[need:] == b"\xAA" * 8
    assert lib.load().net_blob_widen(blob, len(blob), 13, (ctypes.c_int32 * 8)(*ch), None, 0, None) == lib.NET_OK
    # one byte short: refused, the size reported, nothing written
    rc, n, out = _widen(blob, 13, ch, cap=need - 1)
    assert (rc, n) == (INV, need) and out == b"\xAA" * (need + 7)
    # the parser's verdict comes first, whatever the other arguments are
    for bad in (b"", b"x" * 100, blob[:-4], blob + b"\0\0\0\0", blob[:63], b"MIBMINEX" + blob[8:]):
        for R, c, nullc in ((13, ch, False), (0, ch, False), (13, ch, True)):
            rc, n, _ = _widen(bad, R, c, null_channels=nullc)
            assert (rc, n) == (BLOB, 12345), (len(bad), R)
    flagged = bytearray(blob)
    flagged[48] = 4  # an unknown flag bit
    assert _widen(bytes(flagged), 13, ch)[0] == BLOB
    # R and the channels
    for R in (0, -1, 65, 7, 2**31 - 1, -(2**31)):  # 7 < C: no 8 distinct rows
        assert _widen(blob, R, ch)[:2] == (INV, 12345), R
    assert _widen(blob, 13, ch, null_channels=True)[:2] == (INV, 12345)
    for i, v in ((0, -1), (7, 13), (3, 2**31 - 1), (3, -(2**31)), (5, 12), (7, 0)):  # out of range, duplicates
        c = list(ch)
        c[i] = v
        assert _widen(blob, 13, c)[:2] == (INV, 12345), (i, v)
    # the limits that pass: R = C with the identity (the same blob back), R = 64, rows 0 and R - 1 used
    assert _widen(blob, 8, list(range(8)))[2][:len(blob)] == blob
    rc, n, out = _widen(blob, 64, [63, 0, 1, 2, 3, 4, 5, 62])
    assert rc == lib.NET_OK and out[:n] == ps.widened(64, [63, 0, 1, 2, 3, 4, 5, 62]).to_blob()
    # the Python wrappers say the same
    for R, c in ((0, ch), (65, ch), (13, ch[:-1] + [ch[0]]), (13, ch[:-1] + [13])):
        with pytest.raises(ValueError):
            ps.widened(R, c)
        with pytest.raises(lib.NetError) as e:
            lib.blob_widen(blob, R, c)
        assert e.value.code == INV
    for c in (ch[:-1], ch + [4]):
        with pytest.raises(ValueError):
            ps.widened(13, c)
        with pytest.raises(ValueError):
            lib.blob_widen(blob, 13, c)
    with pytest.raises(lib.NetError) as e:
        lib.blob_widen(b"x" * 100, 13, ch)
    assert e.value.code == BLOB


INFO_CASES = CASES + [
    ("38->64 exact division", lambda: X(seed=79, C=38, T=480, N=2, mids=3), 64, 7),
    ("19->64 exact division, plain-BN", lambda: X(seed=80, C=19, T=480, N=3, mids=3, reorder_bn=False), 64, 8),
]


@pytest.mark.parametrize("name,make,R,seed", INFO_CASES, ids=[c[0] for c in INFO_CASES])
def test_params_info_is_the_same_before_and_after(name, make, R, seed):
    """The reachable ranges are the same, so the widened blob loads as the original does and takes the
    same requant path (info[4]); a compiled geometry becomes a general-path one once R != C."""
    ps = make()
    ch = channel_map(ps.dims.C, R, seed)
    try:
        lib.params_load(ps)
        before, folded = lib.params_info(), lib.folded_filters()
        lib.params_load_blob(lib.blob_widen(ps.to_blob(), R, ch))
        after = lib.params_info()
        assert lib.params_dims()["C"] == R
        assert after["exact_division"] == before["exact_division"] and lib.folded_filters() == folded, name
        if before["path"] == "general" or R == ps.dims.C:
            assert after == before, name
        else:  # 22 x 1125 over 64 rows: no compiled kernel has that shape
            assert before["path"] in ("float", "exact") and (after["path"], after["shape"]) == ("general", -1), name
    finally:
        lib.params_unload()


def test_exact_division_case_is_one():
    """INFO_CASES' last two do divide exactly (else they would show nothing about info[4])."""
    for _, make, _, _ in INFO_CASES[-2:]:
        try:
            lib.params_load(make())
            assert lib.params_info()["exact_division"]
        finally:
            lib.params_unload()


def test_a_set_the_loader_refuses_is_refused_widened_too():
    ps = S(seed=32, C=8, T=64, N=2)
    ps.l1_offset[0] = 2**31 - 1  # acc + offset overflows int32
    L = lib.load()
    blob = ps.to_blob()
    wide = lib.blob_widen(blob, 13, [12, 0, 5, 3, 9, 1, 7, 2])
    assert L.net_params_load(blob, len(blob)) == L.net_params_load(wide, len(wide)) == lib.NET_ERR_RANGE


def test_sets_of_different_C_share_a_bank_once_widened():
    a, b = S(seed=41, C=19, T=480, N=3), S(seed=42, C=38, T=480, N=3)
    with pytest.raises(lib.NetError) as e:
        lib.Bank([a, b], scales=[3.0, 2.0])
    assert e.value.code == lib.NET_ERR_UNSUPPORTED and e.value.failed == 1
    wa, wb = a.widened(64, channel_map(19, 64, 11)), lib.blob_widen(b.to_blob(), 64, channel_map(38, 64, 12))
    with lib.Bank([wa, wb], scales=[3.0, 2.0]) as bank:
        assert bank.info()[:4] == [2, 64, 480, 3] and bank.dims.C == 64  # net_bank_info reports R as C
