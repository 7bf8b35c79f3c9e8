"""Parameter banks without a GPU: what net_bank_create builds and refuses, its independence from
the loaded set, every argument check of the epochs-bank entries (each call here fails a check or has
no epoch, so nothing is launched), and the certification of the inputs tests/test_gpu_bank.py uses."""
import ctypes

import numpy as np
import pytest

import support_bank as sb
from mibminet import lib
from mibminet.params import ParamSet
from support import want

INV, RNG, UNS, BLOB, OK = lib.NET_ERR_INVALID, lib.NET_ERR_RANGE, lib.NET_ERR_UNSUPPORTED, lib.NET_ERR_BLOB, lib.NET_OK
C, T, N = 22, 1125, 4


def _alone(ps):
    """The window image of a set loaded alone."""
    lib.params_load(ps)
    return lib.image_copy(1)


def _refused(param_sets, scales=None):
    with pytest.raises(lib.NetError) as e:
        lib.Bank(param_sets, scales)
    return e.value.code, e.value.failed


@pytest.mark.parametrize("C,T,N", [(22, 1125, 4), (19, 480, 3)])
def test_slices_are_the_images_of_the_sets_loaded_alone(C, T, N):
    sets = sb.sets(C, T, N)
    with lib.Bank(sets, [1.0, 2.0, 3.0, 4.0, 5.0]) as bank:
        assert (bank.n_sets, bank.exact_division, bank.has_scales) == (5, False, True)
        assert (bank.dims.C, bank.dims.T, bank.dims.N) == (C, T, N)
        images = [bank.image(s) for s in range(5)]
        assert bank.info()[:4] == [5, C, T, N] and bank.info()[6] == len(images[0])
        assert bank.device_copies() == 0  # nothing touches a device at creation
    for s, ps in enumerate(sets):
        assert images[s] == _alone(ps), s
    assert len(set(images)) == 5
    lib.params_unload()


def test_blobs_and_param_sets_build_the_same_bank():
    sets = sb.sets(19, 480, 3)[:2]
    with lib.Bank(sets) as a, lib.Bank([ps.to_blob() for ps in sets]) as b:
        assert not a.has_scales and [a.image(s) for s in range(2)] == [b.image(s) for s in range(2)]
        with pytest.raises(lib.NetError):
            a.image(2)
    with pytest.raises(ValueError):
        a.info()  # closed


def test_mixed_bank_runs_exact_division():
    """A float set beside one that needs exact division: the bank reports exact division, the exact
    set's slice is its own image and the float set's slice differs from its float image (its float
    forms are zero, its xr flag set) while an all-float and an all-exact bank keep theirs."""
    fl, ex = ParamSet.synthetic(seed=101), ParamSet.synthetic_extreme(seed=77, mids=3)
    with lib.Bank([fl, ex]) as bank, lib.Bank([fl]) as bf, lib.Bank([ex, ex]) as bx:
        assert (bank.exact_division, bf.exact_division, bx.exact_division) == (True, False, True)
        mixed = [bank.image(0), bank.image(1)]
        only = [bf.image(0), bx.image(1)]
    assert only == [_alone(fl), _alone(ex)]
    assert lib.params_info()["exact_division"]  # ex is the loaded set
    assert mixed[1] == only[1] and mixed[0] != only[0]
    # the xr flag is the 16th int of gen::GenParams (C, T, N, T8, T64, T64A, NB1, MT, NTT, K7, K7T1,
    # pad2, rb, lo, xstride, xr); the geometry before it is unchanged
    head = lambda img: np.frombuffer(img[:64], np.int32)
    assert head(mixed[0])[15] == 1 and head(only[0])[15] == 0
    assert np.array_equal(head(mixed[0])[:15], head(only[0])[:15])
    lib.params_unload()


def test_the_loaded_set_is_untouched():
    ps = ParamSet.synthetic(seed=5)
    lib.params_load(ps)
    before = (lib.image_digest(), lib.params_info(), lib.params_dims(), lib.image_copy(1), lib.device_images())
    bank = lib.Bank(sb.sets(19, 480, 3), [1.0] * 5)
    bank.info()
    assert (lib.image_digest(), lib.params_info(), lib.params_dims(), lib.image_copy(1), lib.device_images()) == before
    bank.close()
    bank.close()  # idempotent
    lib.load().net_bank_destroy(None)  # NULL is allowed
    assert (lib.image_digest(), lib.params_info(), lib.params_dims(), lib.image_copy(1), lib.device_images()) == before
    lib.params_unload()
    with lib.Bank(sb.sets(19, 480, 3)[:1]) as b:  # a bank needs no loaded set
        assert b.n_sets == 1 and lib.params_dims() == {}


def test_refusals_name_the_set():
    S = ParamSet.synthetic
    good = list(sb.sets(C, T, N))
    for at, other in ((1, S(seed=9, C=C, T=1000, N=N)), (4, S(seed=9, C=C, T=T, N=3)), (2, S(seed=9, C=21, T=T, N=N)),
                      (3, S(seed=9, C=C, T=T, N=N, clip_balanced=True)), (1, S(seed=9, C=C, T=T, N=N, reorder_bn=False))):
        sets = list(good)
        sets[at] = other
        assert _refused(sets) == (UNS, at)
    blobs = [ps.to_blob() for ps in good]
    assert _refused(blobs[:3] + [blobs[3][:-4]] + blobs[4:]) == (BLOB, 3)     # truncated
    assert _refused([b"MIBMINET" + bytes(56)] + blobs[1:]) == (BLOB, 0)
    assert _refused([S(seed=9, C=65, T=T, N=N)]) == (UNS, 0)                   # outside the family
    # l3_factor = 0, where the reference would divide by zero: the int32 after the header, layer 1's
    # factors, offsets and weights and layer 2's factors, offsets and weights
    at = 64 + 2 * 64 + 16 * 24 + 2 * 64 + 16 * 64
    assert np.frombuffer(blobs[2][at: at + 4], np.int32)[0] == good[2].l3_factor
    assert _refused(blobs[:2] + [blobs[2][:at] + bytes(4) + blobs[2][at + 4:]]) == (RNG, 2)
    # a mismatch and a bad blob: the first of the two is named
    assert _refused([blobs[0], blobs[1][:100], S(seed=9, C=C, T=1000, N=N).to_blob()]) == (BLOB, 1)
    for scale, code in ((0.0, INV), (-1.0, INV), (float("nan"), INV), (float("inf"), INV), (1e-30, RNG), (2.0**61, RNG)):
        assert _refused(good, [1.0, 1.0, 1.0, scale, 1.0]) == (code, 3), scale
    with lib.Bank(good, [2.0**-60, 1.0, 1.0, 1.0, 2.0**60]) as b:
        assert b.has_scales
    with pytest.raises(ValueError):
        lib.Bank(good, [1.0])
    L = lib.load()
    h, failed = ctypes.c_void_p(5), ctypes.c_size_t(77)
    one = (ctypes.c_void_p * 1)(None)
    size = (ctypes.c_size_t * 1)(0)
    for n in (0, 1025, 2**40):  # NET_BANK_MAX_SETS = 1024
        assert L.net_bank_create(one, size, None, n, ctypes.byref(h), ctypes.byref(failed)) == INV
        assert h.value is None
    assert L.net_bank_create(None, size, None, 1, ctypes.byref(h), None) == INV
    assert L.net_bank_create(one, None, None, 1, ctypes.byref(h), None) == INV
    assert L.net_bank_create(one, size, None, 1, None, None) == INV
    assert L.net_bank_create(one, size, None, 1, ctypes.byref(h), None) == BLOB  # failed may be NULL
    assert L.net_bank_info(None, (ctypes.c_int32 * 7)()) == INV


# ---- the entry checks, in epochs_async's order ------------------------------------------------------
@pytest.fixture
def ptrs():
    """x, onsets, y, n_bad, set_of: 16-byte aligned addresses inside one host buffer."""
    buf = np.zeros(160, np.uint8)
    a = (buf.ctypes.data + 15) // 16 * 16
    yield a, a + 16, a + 32, a + 48, a + 64
    del buf


@pytest.fixture(scope="module")
def banks():
    lib.params_unload()  # no entry below may need a loaded set
    with lib.Bank(sb.sets(C, T, N), [1.0] * 5) as five, lib.Bank(sb.sets(C, T, N)[:1]) as one:
        yield five, one


def _chan(values):
    return (ctypes.c_int32 * len(values))(*values)


def test_entry_checks_without_a_gpu(banks, ptrs):
    five, one = banks
    i8, f32 = lib.load().net_model_compute_epochs_bank, lib.load().net_model_compute_epochs_bank_f32
    x, on, y, nb, so = ptrs
    L = 4000
    n = C * L
    good = (five.handle, x, n, L, None, on, so, 7, y, nb, 0, None)

    def call(fn=i8, **kw):
        a = dict(zip(("bank", "x", "n", "rs", "ch", "on", "so", "E", "y", "nb", "dev", "st"), good))
        a.update(kw)
        return fn(*a.values())

    assert call(bank=None) == INV and call(bank=None, E=0) == INV  # where NET_ERR_NO_PARAMS stands
    assert call(x=None) == INV and call(y=None) == INV and call(on=None) == INV
    for off in (1, 2, 3):
        assert call(y=y + off) == INV and call(nb=nb + off) == INV and call(so=so + off) == INV
        assert call(so=so + off, E=0) == INV
    for off in (1, 2, 4, 7):
        assert call(on=on + off) == INV
    assert call(rs=0) == INV and call(dev=-1) == INV and call(dev=1 << 20) == INV
    assert call(E=2**31 - 65535) == INV and call(E=2**40) == INV
    assert call(so=None) == INV and call(so=None, E=0) == OK        # NULL: a bank of one set only
    assert call(bank=one.handle, so=None, E=0) == OK
    assert call(bank=one.handle, so=None, dev=-1) == INV
    for off in (0, 1, 2, 3):
        assert call(x=x + off, E=0) == OK
    assert call(nb=None, E=0) == OK
    assert i8(five.handle, None, n, L, None, None, None, 0, None, None, 0, None) == OK
    # the span, from the bank's C and T
    span = (C - 1) * L + T
    assert call(n=span, E=0) == OK and call(n=span - 1, E=0) == INV
    ch = _chan([3, 0, 63, 7] + list(range(18)))
    assert call(ch=ch, n=63 * L + T, E=0) == OK and call(ch=ch, n=63 * L + T - 1, E=0) == INV
    assert call(ch=_chan([-1] + list(range(21))), n=2**40, E=0) == INV
    assert call(ch=_chan([1] + [0] * 21), n=2**62, rs=2**31 - 7 - T, E=0) == OK
    assert call(ch=_chan([1] + [0] * 21), n=2**62, rs=2**31 - 6 - T, E=0) == INV
    # float32: x 4-byte aligned, the limit counts bytes, and a bank without scales is refused
    assert call(f32, E=0) == OK and call(f32, x=x + 4, E=0) == OK
    for off in (1, 2, 3):
        assert call(f32, x=x + off, E=0) == INV
    ok32 = (2**31 - 7) // 4 - T
    assert call(f32, ch=_chan([1] + [0] * 21), n=2**62, rs=ok32, E=0) == OK
    assert call(f32, ch=_chan([1] + [0] * 21), n=2**62, rs=ok32 + 1, E=0) == INV
    assert call(f32, bank=one.handle, so=None, E=0) == INV and call(bank=one.handle, so=None, E=0) == OK
    assert five.device_copies() == 0 and one.device_copies() == 0


def test_python_entries_reject_what_the_abi_cannot_see(banks):
    import torch

    five, one = banks
    x = torch.zeros((C, 4000), dtype=torch.int8)
    for bad in (lambda: lib.forward_epochs_bank_torch(five, x, [0], [0]),                      # not on the device
                lambda: lib.forward_epochs_bank_torch(five, np.zeros((C, 4000), np.int8), [0], [0]),
                lambda: lib.forward_epochs_bank_torch(None, x, [0], [0]),
                lambda: lib.forward_epochs_bank_torch(five, None, [0], [0]),
                lambda: lib.forward_bank_torch(five, [[0]], [0]),
                lambda: lib.forward_bank_torch(five, torch.zeros((2, C, T + 1), dtype=torch.int8), [0, 1]),
                lambda: lib.forward_bank_torch(sb.sets(C, T, N)[0], x, [0])):
        with pytest.raises(ValueError):
            bad()


# ---- certification of the GPU tests' inputs -----------------------------------------------------------
@pytest.mark.parametrize("C,T,N", sb.GEOMETRIES)
def test_inputs_are_certified(C, T, N):
    """A condition on the inputs of tests/test_gpu_bank.py, not a measurement.  For every ordered
    pair (a, b) of sets that a set_of pattern places next to each other and each layer k, the set a
    with layer k's arrays taken from b gives other logits than a on at least 75 % of the epochs (of
    the first 23 and of all 48): a kernel that ran any layer of an item on its neighbour's state,
    such as one finishing an item on its successor's layer 4-5 state, cannot pass.  No row under any
    set is all zeros (what an invalid item writes), and the five sets' rows differ pairwise."""
    _certify(sb.sets(C, T, N), sb.table(C, T, N), sb.epochs(C, T), sb.SIZES)


def _certify(sets, tab, ep, sizes):
    assert tab.shape == (5, len(ep), sets[0].dims.N) and tab.any(axis=2).all()
    for a in range(5):
        for b in range(a):
            assert (tab[a] != tab[b]).any(axis=1).all(), (a, b)
    pairs = sb.adjacent_pairs()
    assert len(pairs) == 20  # the patterns put every set next to every other
    for a, b in pairs:
        for k in range(1, 6):
            changed = (want(sb.hybrid(sets[a], sets[b], k), ep) != tab[a]).any(axis=1)
            for E in sizes:
                assert changed[:E].mean() >= 0.75, (a, b, k, E, float(changed[:E].mean()))


@pytest.mark.parametrize("variant", list(sb.VARIANTS))
@pytest.mark.parametrize("C,T,N", sb.VARIANT_GEOMETRIES)
def test_variant_inputs_are_certified(C, T, N, variant):
    """The same condition on the banks of test_gpu_bank.py's test_variants (plain BN, balanced clip,
    int4 weights, exact division, mixed), on the 23 epochs it uses."""
    sets, ep = sb.VARIANTS[variant](C, T, N), sb.epochs(C, T)[: sb.VARIANT_E]
    _certify(sets, np.stack([want(ps, ep) for ps in sets]), ep, (sb.VARIANT_E,))
