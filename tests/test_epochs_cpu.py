"""Epochs from a wider array (net_model_compute_epochs): the ctypes signatures and every argument
check, none of which needs a GPU.  Every call here either fails a check or has no epoch (E == 0),
so nothing is launched where a GPU is present either; the pointers are host buffers that no call
reads (only the channel table is a host array by contract)."""
import ctypes

import numpy as np
import pytest

from mibminet import lib
from mibminet.params import ParamSet
from support import loaded  # noqa: F401 (a fixture)

INV, NOP, RNG, UNS, OK = (lib.NET_ERR_INVALID, lib.NET_ERR_NO_PARAMS, lib.NET_ERR_RANGE, lib.NET_ERR_UNSUPPORTED,
                          lib.NET_OK)
C, T = 22, 1125


@pytest.fixture
def ptrs():
    """x, onsets, y, n_bad: 16-byte aligned addresses inside one host buffer."""
    buf = np.zeros(128, np.uint8)
    a = (buf.ctypes.data + 15) // 16 * 16
    yield a, a + 16, a + 32, a + 48
    del buf


def _chan(values):
    return (ctypes.c_int32 * len(values))(*values)


def test_ctypes_signatures():
    L = lib.load()
    names = lambda fn: [t.__name__ for t in fn.argtypes]
    assert names(L.net_model_compute_epochs) == ["c_void_p", "c_ulong", "c_ulong", "c_void_p", "c_void_p", "c_ulong",
                                                 "c_void_p", "c_void_p", "c_int", "c_void_p"]
    assert names(L.net_model_compute_epochs_f32) == ["c_void_p", "c_ulong", "c_ulong", "c_void_p", "c_void_p",
                                                     "c_ulong", "c_float", "c_void_p", "c_void_p", "c_int", "c_void_p"]
    assert L.net_model_compute_epochs.restype is ctypes.c_int
    assert L.net_model_compute_epochs_f32.restype is ctypes.c_int
    assert {"net_model_compute_epochs", "net_model_compute_epochs_f32"} <= set(lib.EXPORTED_SYMBOLS)


def test_no_params_comes_first():
    lib.params_unload()
    L = lib.load()
    assert L.net_model_compute_epochs(None, 0, 0, None, 3, 5, 1, 2, -1, None) == NOP
    assert L.net_model_compute_epochs(None, 10**6, 1125, None, None, 0, None, None, 0, None) == NOP
    assert L.net_model_compute_epochs_f32(None, 0, 0, None, 3, 5, float("nan"), 1, 2, -1, None) == NOP


def test_invalid_arguments_without_a_gpu(loaded, ptrs):
    fn = lib.load().net_model_compute_epochs
    x, on, y, nb = ptrs
    L = 4000
    n = C * L  # a [22][L] recording
    good = (x, n, L, None, on, 7, y, nb, 0, None)

    def call(**kw):
        a = dict(zip(("x", "n", "rs", "ch", "on", "E", "y", "nb", "dev", "st"), good))
        a.update(kw)
        return fn(*a.values())

    assert call(x=None) == INV and call(y=None) == INV and call(on=None) == INV  # null with E > 0
    for off in (1, 2, 3):
        assert call(y=y + off) == INV and call(nb=nb + off) == INV  # 4-byte alignment
    for off in (1, 2, 4, 7):
        assert call(on=on + off) == INV                             # 8-byte alignment
    assert call(rs=0) == INV
    assert call(dev=-1) == INV and call(dev=1 << 20) == INV
    assert call(E=2**31 - 65535) == INV and call(E=2**40) == INV     # E > INT32_MAX - 65,535
    # int8 x has no alignment requirement and n_bad may be NULL: with E == 0 both pass every check
    for off in (0, 1, 2, 3):
        assert call(x=x + off, E=0) == OK
    assert call(nb=None, E=0) == OK
    # E == 0 touches nothing, whatever the pointers are
    assert fn(None, n, L, None, None, 0, None, None, 0, None) == OK


def test_span_must_fit_in_the_source(loaded, ptrs):
    fn = lib.load().net_model_compute_epochs
    x, on, y, nb = ptrs
    L = 4000
    span = (C - 1) * L + T  # channels = NULL: rows 0 .. C - 1
    assert fn(x, span, L, None, on, 0, y, nb, 0, None) == OK        # span == n_elems
    assert fn(x, span - 1, L, None, on, 0, y, nb, 0, None) == INV   # span == n_elems + 1
    assert fn(x, span - 1, L, None, on, 3, y, nb, 0, None) == INV
    assert fn(x, 0, L, None, on, 0, y, nb, 0, None) == INV
    # the channel table sets the span: max(channels) row_stride + T
    ch = _chan([3, 0, 63, 7] + list(range(18)))
    span = 63 * L + T
    assert fn(x, span, L, ch, on, 0, y, nb, 0, None) == OK
    assert fn(x, span - 1, L, ch, on, 0, y, nb, 0, None) == INV
    ch0 = _chan([0] * C)  # every network channel reads row 0: span = T, whatever the row stride
    assert fn(x, T, 2**62, ch0, on, 0, y, nb, 0, None) == OK
    assert fn(x, T - 1, 2**62, ch0, on, 0, y, nb, 0, None) == INV
    # span overflows size_t
    assert fn(x, 2**64 - 1, 2**62, _chan([4] + [0] * (C - 1)), on, 0, y, nb, 0, None) == INV
    assert fn(x, 2**64 - 1, 2**64 - 1, None, on, 0, y, nb, 0, None) == INV


def test_negative_channel(loaded, ptrs):
    fn = lib.load().net_model_compute_epochs
    x, on, y, nb = ptrs
    for bad in (-1, -2**31):
        for pos in (0, C - 1):
            ch = list(range(C))
            ch[pos] = bad
            assert fn(x, 2**40, 4000, _chan(ch), on, 0, y, nb, 0, None) == INV
    assert fn(x, 2**40, 4000, _chan(list(range(C))[::-1]), on, 0, y, nb, 0, None) == OK  # unsorted
    assert fn(x, 2**40, 4000, _chan([5] * C), on, 0, y, nb, 0, None) == OK               # duplicates


def test_span_limit_of_one_buffer_view(loaded, ptrs):
    """elem_size span + 6 >= 2^31 is refused; n_elems itself has no limit."""
    x, on, y, nb = ptrs
    i8, f32 = lib.load().net_model_compute_epochs, lib.load().net_model_compute_epochs_f32
    ch = _chan([1] + [0] * (C - 1))  # span = row_stride + T
    big = 2**62
    ok8 = 2**31 - 7 - T  # span = 2^31 - 7: span + 6 = 2^31 - 1
    assert i8(x, big, ok8, ch, on, 0, y, nb, 0, None) == OK
    assert i8(x, big, ok8 + 1, ch, on, 0, y, nb, 0, None) == INV
    assert i8(x, big, 2**40, ch, on, 0, y, nb, 0, None) == INV
    ok32 = (2**31 - 7) // 4 - T  # 4 span + 6 <= 2^31 - 1
    assert 4 * (ok32 + T) + 6 < 2**31 <= 4 * (ok32 + 1 + T) + 6
    assert f32(x, big, ok32, ch, on, 0, 1.0, y, nb, 0, None) == OK
    assert f32(x, big, ok32 + 1, ch, on, 0, 1.0, y, nb, 0, None) == INV
    assert i8(x, big, ok32 + 1, ch, on, 0, y, nb, 0, None) == OK  # the limit counts bytes


def test_float_entry_alignment_and_scale_domain(loaded, ptrs):
    fn = lib.load().net_model_compute_epochs_f32
    x, on, y, nb = ptrs
    L = 4000
    n = C * L
    assert fn(x, n, L, None, on, 0, 1.0, y, nb, 0, None) == OK
    for off in (1, 2, 3):
        assert fn(x + off, n, L, None, on, 0, 1.0, y, nb, 0, None) == INV  # float32 not 4-byte aligned
    assert fn(x + 4, n, L, None, on, 0, 1.0, y, nb, 0, None) == OK
    for scale in (0.0, -1.0, float("nan"), float("inf")):
        assert fn(x, n, L, None, on, 0, scale, y, nb, 0, None) == INV
    for scale in (2.0**-61, 2.0**61, 1e-30, 3e38):
        assert fn(x, n, L, None, on, 0, scale, y, nb, 0, None) == RNG
    for scale in (2.0**-60, 2.0**60):
        assert fn(x, n, L, None, on, 0, scale, y, nb, 0, None) == OK
    # an invalid argument is reported before the scale's range
    assert fn(x, n, 0, None, on, 0, 1e-30, y, nb, 0, None) == INV


def test_channel_count_follows_the_loaded_network(ptrs):
    x, on, y, nb = ptrs
    lib.params_load(ParamSet.synthetic(seed=5, C=19, T=480, N=3))
    fn = lib.load().net_model_compute_epochs
    ch = _chan([63] + list(range(18)) + [-1, -1, -1])  # entries past C = 19 are not read
    assert fn(x, 63 * 640 + 480, 640, ch, on, 0, y, nb, 0, None) == OK
    assert fn(x, 63 * 640 + 479, 640, ch, on, 0, y, nb, 0, None) == INV
    lib.params_unload()


def test_python_entries_reject_what_the_abi_cannot_see(loaded):
    import torch

    x = torch.zeros((C, 4000), dtype=torch.int8)
    with pytest.raises(ValueError):
        lib.forward_epochs_torch(x, [0, 1])                      # not on the device
    with pytest.raises(ValueError):
        lib.forward_epochs_torch(np.zeros((C, 4000), np.int8), [0])
    with pytest.raises(ValueError):
        lib.forward_crop_torch(torch.zeros((3, 64, 1000), dtype=torch.int8), 0)       # T = 1125 > Tf
    with pytest.raises(ValueError):
        lib.forward_crop_torch(torch.zeros((3, 64, 1200), dtype=torch.int8), 76)      # t0 + T > Tf
    with pytest.raises(ValueError):
        lib.forward_crop_torch(torch.zeros((3, 64, 1200), dtype=torch.int8), 0, channels=[64] + list(range(21)))
    with pytest.raises(ValueError):
        lib.forward_crop_torch(torch.zeros((3, 64, 1200), dtype=torch.int8), 0, channels=list(range(21)))
    with pytest.raises(ValueError):
        lib.forward_crop_torch(torch.zeros((64, 1200), dtype=torch.int8), 0)           # not a batch
