"""Parameter banks on the GPU (net_model_compute_epochs_bank[_f32], forward_bank.hpp): epoch e is
classified by set set_of[e] of a bank of five networks.

The reference of every row is the C oracle of set set_of[e] on the materialised epoch
(support_bank.table, computed once per geometry), never another GPU entry, and every comparison is
byte-exact in every row.  tests/test_bank_cpu.py certifies the inputs: swapping any one layer's
parameters between two sets that a pattern places next to each other changes at least 75 % of the
rows, no row is all zeros and the five sets' rows differ pairwise, so an item that ran any layer on
a neighbour's state shows.  Under lib.grid_cap(1) one workgroup walks every switch and every later
pass of a list; that is where a wrong finish shows.
"""
import ctypes

import numpy as np
import pytest

import oracle
import support_bank as sb
from mibminet import lib
from mibminet.params import ParamSet
from oracle import golden_np as G
from support import _BAD, CAPS, NTH, at_offset, capped, scattered, want  # noqa: F401 (capped: a fixture)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def banks(gpu):
    """The banks of the module, by key, built once and closed at the end."""
    cache = {}

    def get(key, make):
        if key not in cache:
            cache[key] = make()
        return cache[key]

    yield get
    for b in cache.values():
        b.close()


def _five(banks, C, T, N, **kw):
    return banks((C, T, N, tuple(sorted(kw.items()))), lambda: lib.Bank(sb.sets(C, T, N, **kw)))


def _call(bank, x, row_stride, channels, onsets, set_of, f32=False):
    """The C entry on a prefilled logits buffer and a counter between two guards: (rows [E][N], the
    three counters).  Nothing past the E N logits may be written."""
    import torch

    E, N = len(onsets), bank.dims.N
    y = torch.full((E * N + 64,), 0x5A, dtype=torch.int8, device="cuda")
    nb = torch.zeros((3,), dtype=torch.int32, device="cuda")
    ond = torch.tensor([int(o) for o in onsets], dtype=torch.int64, device="cuda")
    sod = None if set_of is None else torch.tensor([int(s) for s in set_of], dtype=torch.int32, device="cuda")
    tab = None if channels is None else (ctypes.c_int32 * len(channels))(*channels)
    fn = lib.load().net_model_compute_epochs_bank_f32 if f32 else lib.load().net_model_compute_epochs_bank
    rc = fn(bank.handle, x.data_ptr(), x.numel(), row_stride, tab, ond.data_ptr(),
            None if sod is None else sod.data_ptr(), E, y.data_ptr(), nb.data_ptr() + 4, 0, None)
    assert rc == lib.NET_OK, rc
    torch.cuda.synchronize()
    assert bool((y[E * N:] == 0x5A).all())
    return y[: E * N].view(E, N).cpu().numpy(), nb.cpu().tolist()


def _source(torch, C, T):
    src, onsets, channels = sb.case(C, T)
    return at_offset(torch, src, 1 + C % 3), src.shape[1], list(onsets), list(channels)


# ---- every geometry x set_of pattern x grid cap -----------------------------------------------------
@pytest.mark.parametrize("pattern", list(sb.patterns(sb.E_MAX)))
@pytest.mark.parametrize("C,T,N", sb.GEOMETRIES)
def test_patterns(C, T, N, pattern, banks, capped):
    import torch

    bank, tab = _five(banks, C, T, N), sb.table(C, T, N)
    x, rs, onsets, channels = _source(torch, C, T)
    for E in sb.SIZES:
        so = sb.patterns(E)[pattern]
        expect = sb.reference(tab[:, :E], so)
        for cap in CAPS:
            capped(cap)
            rows, nb = _call(bank, x, rs, channels, onsets[:E], so)
            assert nb == [0, 0, 0], (E, cap)
            np.testing.assert_array_equal(rows, expect, err_msg=f"{pattern}, E {E}, cap {cap}")
    assert bank.device_copies() == 1


# ---- invalid items around switches and range ends -----------------------------------------------------
_SO = [0] * 5 + [1] * 6 + [2] * 2 + [3] * 7 + [4] * 4  # switches at 5, 11, 13 and 20
# with three workgroups the ranges are [0, 8), [8, 16) and [16, 24).  "set": an index outside the
# bank, "onset": an onset outside the source.  0: first of a range, before any set is there; 4:
# directly before a switch; 8: first of a range; 11: directly after a switch (the switch moves to
# 12); 15: last of a range; 16, 17: two in a row from a range's start; 23: last of all, both invalid
_BAD_AT = {0: "set", 4: "set", 8: "set", 11: "onset", 15: "onset", 16: "onset", 17: "set", 23: "both"}


@pytest.mark.parametrize("C,T,N", sb.GEOMETRIES)
def test_invalid_items(C, T, N, banks, capped):
    import torch

    E = len(_SO)
    assert E == 24 and [i for i in range(1, E) if _SO[i] != _SO[i - 1]] == [5, 11, 13, 20]
    bank, tab = _five(banks, C, T, N), sb.table(C, T, N)
    x, rs, onsets, channels = _source(torch, C, T)
    shift = sb.GEOMETRIES.index((C, T, N))
    on, so = onsets[:E], list(_SO)
    bad_sets = [-1, bank.n_sets, 2**31 - 1, -(2**31)]
    for j, (i, what) in enumerate(sorted(_BAD_AT.items())):
        if what in ("set", "both"):
            so[i] = bad_sets[(j + shift) % len(bad_sets)]
        if what in ("onset", "both"):
            v = _BAD[(j + shift) % len(_BAD)]
            on[i] = sb.last_onset(C, T) + 1 if v is None else v
    ok = [i for i in range(E) if i not in _BAD_AT]
    expect = sb.reference(tab[:, :E], _SO)[ok]
    for cap in CAPS:
        capped(cap)
        rows, nb = _call(bank, x, rs, channels, on, so)
        assert nb == [0, len(_BAD_AT), 0], cap  # once per epoch, the one with both included
        assert not rows[sorted(_BAD_AT)].any(), cap
        np.testing.assert_array_equal(rows[ok], expect, err_msg=f"cap {cap}")
    # the Python entry counts them and says what they are
    with pytest.raises(ValueError, match="8 of 24 onsets or set indices"):
        lib.forward_epochs_bank_torch(bank, x, on, so, channels=channels, row_stride=rs)


# ---- the build variants -----------------------------------------------------------------------------
@pytest.mark.parametrize("variant", list(sb.VARIANTS))
@pytest.mark.parametrize("C,T,N", sb.VARIANT_GEOMETRIES)
def test_variants(C, T, N, variant, capped):
    import torch

    sets = sb.VARIANTS[variant](C, T, N)
    E = sb.VARIANT_E
    tab = np.stack([want(ps, sb.epochs(C, T)[:E]) for ps in sets])
    x, rs, onsets, channels = _source(torch, C, T)
    with lib.Bank(sets) as bank:
        assert bank.exact_division == (variant in sb.EXACT)
        for name in ("random", "alternating"):
            so = sb.patterns(E)[name]
            for cap in (1, 0):
                capped(cap)
                rows, nb = _call(bank, x, rs, channels, onsets[:E], so)
                assert nb == [0, 0, 0]
                np.testing.assert_array_equal(rows, sb.reference(tab, so), err_msg=f"{variant} {name} cap {cap}")


# ---- float32 input, one scale per set ------------------------------------------------------------------
_SCALES = [0.5, 1.3, 3.0, 7.25, 100.0]


def _dequant(q, scale):
    """support.dequant's construction for `scale`: the middle of each int8 value's interval."""
    v = np.arange(-127, 128)
    lut = ((v + 0.5 * np.sign(v)) * (scale / 127.0)).astype(np.float32)
    assert np.array_equal(G.quantize_to_int(lut, scale), v)
    return lut[np.asarray(q, np.int16) + 127]


@pytest.mark.parametrize("C,T,N", [(19, 480, 3), (22, 1125, 4), (64, 480, 2)])
def test_float32_with_five_scales(C, T, N, capped):
    """Epoch e holds float samples that scale[set_of[e]] quantises to the int8 epoch, with
    non-finite samples planted as support.float_recording plants them; the result is the oracle's
    on the epochs as the two-pass quantiser (net_quantize_input_f32) quantises them with each
    epoch's own scale."""
    import torch

    E = 23
    sets, q = sb.sets(C, T, N), sb.epochs(C, T)[:E]
    so = sb.patterns(E)["random"]
    xf = np.stack([_dequant(q[e], _SCALES[so[e]]) for e in range(E)])
    x = at_offset(torch, xf, 4)
    x[0, 0, :7] = torch.tensor([float("nan"), float("inf"), -float("inf"), 3.0, -3.0, 0.0, -0.0])
    x[E - 1, C - 1, T - 3:] = torch.tensor([float("nan"), -float("inf"), float("inf")])
    x[7, C // 2, 5:8] = torch.tensor([float("inf"), float("nan"), -1e30])
    expect = np.zeros((E, N), np.int8)
    for s in range(5):
        at = np.flatnonzero(so == s)
        qs = lib.quantize_input_torch(x[torch.from_numpy(at).cuda()].contiguous(), _SCALES[s]).cpu().numpy()
        keep = [i for i, e in enumerate(at) if e not in (0, 7, E - 1)]  # the construction, where nothing is planted
        packed = qs[:, : T * C].reshape(len(at), T, C).transpose(0, 2, 1)
        assert np.array_equal(packed[keep], q[at[keep]])
        expect[at] = oracle.COracle(sets[s]).batch(qs, nthreads=NTH)
    onsets = [e * C * T for e in range(E)]
    with lib.Bank(sets, _SCALES) as bank, lib.Bank(sets) as bare:
        for cap in (1, 0):
            capped(cap)
            rows, nb = _call(bank, x, T, None, onsets, so, f32=True)
            assert nb == [0, 0, 0]
            np.testing.assert_array_equal(rows, expect, err_msg=f"cap {cap}")
        np.testing.assert_array_equal(lib.forward_bank_torch(bank, x, so).cpu().numpy(), expect)
        with pytest.raises(ValueError):
            lib.forward_bank_torch(bare, x, so)  # no scales
        fn = lib.load().net_model_compute_epochs_bank_f32
        assert fn(bare.handle, x.data_ptr(), x.numel(), T, None, 16, 16, 1, 16, None, 0, None) == lib.NET_ERR_INVALID


# ---- channel map, row stride and byte offsets ------------------------------------------------------------
@pytest.mark.parametrize("offset", [0, 1, 2, 3])
@pytest.mark.parametrize("C,T,N", [(19, 480, 3), (64, 480, 2)])
def test_scattered_source_at_every_byte_offset(C, T, N, offset, banks, capped):
    import torch

    B = 23
    bank, tab = _five(banks, C, T, N), sb.table(C, T, N)
    src, onsets, channels = scattered(sb.epochs(C, T)[:B], np.random.default_rng([C, offset]))
    so = sb.patterns(B)["random"]
    capped(3)
    rows, nb = _call(bank, at_offset(torch, src, offset), src.shape[1], channels, onsets, so)
    assert nb == [0, 0, 0]
    np.testing.assert_array_equal(rows, sb.reference(tab[:, :B], so))


# ---- the bank's life beside the loaded set -----------------------------------------------------------------
def test_one_set_bank_with_null_set_of(gpu):
    import torch

    C, T, N = 19, 480, 3
    x, rs, onsets, channels = _source(torch, C, T)
    tab = sb.table(C, T, N)
    with lib.Bank(sb.sets(C, T, N)[2:3]) as bank:
        rows, nb = _call(bank, x, rs, channels, onsets, None)
        np.testing.assert_array_equal(rows, tab[2])
        got = lib.forward_epochs_bank_torch(bank, x, onsets, None, channels=channels, row_stride=rs)
        np.testing.assert_array_equal(got.cpu().numpy(), tab[2])
        trials = torch.from_numpy(np.array(sb.epochs(C, T))).cuda()
        np.testing.assert_array_equal(lib.forward_bank_torch(bank, trials, None).cpu().numpy(), tab[2])
        assert lib.forward_epochs_bank_torch(bank, x, [], None, channels=channels, row_stride=rs).shape == (0, N)
    with lib.Bank(sb.sets(C, T, N)[:2]) as two:
        with pytest.raises(ValueError):
            lib.forward_epochs_bank_torch(two, x, onsets, None, channels=channels, row_stride=rs)
        assert lib.load().net_model_compute_epochs_bank(two.handle, x.data_ptr(), x.numel(), rs, None, 16, None, 1, 16,
                                                        None, 0, None) == lib.NET_ERR_INVALID


def test_bank_calls_around_a_load_of_another_geometry(gpu):
    """A bank call, net_params_load of another geometry, a second bank call: both bank results are
    correct, the loaded set computes what it did, and the bank adds nothing to the device's cache of
    loaded sets."""
    import torch

    C, T, N = 19, 480, 3
    x, rs, onsets, channels = _source(torch, C, T)
    tab, so = sb.table(C, T, N), sb.patterns(sb.E_MAX)["random"]
    lib.params_unload()
    with lib.Bank(sb.sets(C, T, N)) as bank:
        rows, _ = _call(bank, x, rs, channels, onsets, so)  # no set is loaded
        np.testing.assert_array_equal(rows, sb.reference(tab, so))
        assert lib.device_images() == 0 and bank.device_copies() == 1
        other = ParamSet.synthetic(seed=7, C=8, T=64, N=2)
        lib.params_load(other)
        trials = sb.epochs(8, 64)[:5]
        loaded = lib.forward_ct_torch(torch.from_numpy(np.array(trials)).cuda()).cpu().numpy()
        np.testing.assert_array_equal(loaded, want(other, trials))
        images, digest = lib.device_images(), lib.image_digest()
        rows, _ = _call(bank, x, rs, channels, onsets, so[::-1])
        np.testing.assert_array_equal(rows, sb.reference(tab, so[::-1]))
        assert (lib.device_images(), lib.image_digest(), bank.device_copies()) == (images, digest, 1)
        assert lib.params_dims()["T"] == 64
    lib.params_unload()


def test_two_banks_alive_at_once(banks, gpu):
    import torch

    a, b = (19, 480, 3), (64, 480, 2)
    ba, bb = _five(banks, *a), _five(banks, *b)
    for _ in range(2):
        for (C, T, N), bank in ((a, ba), (b, bb)):
            x, rs, onsets, channels = _source(torch, C, T)
            so = sb.patterns(sb.E_MAX)["alternating"]
            rows, _ = _call(bank, x, rs, channels, onsets, so)
            np.testing.assert_array_equal(rows, sb.reference(sb.table(C, T, N), so))


def test_destroy_then_create_reuses_nothing_stale(gpu):
    """A bank of the same sets in reverse order, created right after the first is destroyed (where
    the allocator may hand out the same addresses): its results follow its own order."""
    import torch

    C, T, N = 19, 480, 3
    x, rs, onsets, channels = _source(torch, C, T)
    tab, so = sb.table(C, T, N), sb.patterns(sb.E_MAX)["grouped"]
    for order in (slice(None), slice(None, None, -1), slice(None)):
        with lib.Bank(sb.sets(C, T, N)[order]) as bank:
            rows, _ = _call(bank, x, rs, channels, onsets, so)
            np.testing.assert_array_equal(rows, sb.reference(tab[order], so))
            assert bank.device_copies() == 1


def test_graph_capture_and_replay(gpu):
    """After one eager call the entry allocates nothing and does not wait: captured once on a side
    stream and replayed on other set indices."""
    import torch

    C, T, N = 22, 1125, 4
    x, rs, onsets, channels = _source(torch, C, T)
    tab = sb.table(C, T, N)
    lists = [sb.patterns(sb.E_MAX)[k] for k in ("grouped", "random", "alternating")]
    ond = torch.tensor(onsets, dtype=torch.int64, device="cuda")
    sod = torch.tensor(lists[0], dtype=torch.int32, device="cuda")
    with lib.Bank(sb.sets(C, T, N)) as bank:
        lib.forward_epochs_bank_torch(bank, x, ond, sod, channels=channels, row_stride=rs)  # uploads the bank
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            with torch.cuda.graph(g, stream=s):
                y = lib.forward_epochs_bank_torch(bank, x, ond, sod, channels=channels, row_stride=rs, stream=s,
                                                  check=False)
        for so in lists:
            sod.copy_(torch.from_numpy(so.astype(np.int32)))
            g.replay()
            torch.cuda.synchronize()
            np.testing.assert_array_equal(y.cpu().numpy(), sb.reference(tab, so))
        del g  # the graph goes before the bank it reads
