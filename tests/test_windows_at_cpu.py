"""Windows at given onsets (net_model_compute_windows_at, net_windows_multi_onsets): the argument
checks, the host-side onset lists of many recordings and the chunk planner, none of which needs a
GPU.  Every device-entry call here either fails a check or has no window (W == 0), so nothing is
launched where a GPU is present either; the pointers are host buffers that no call reads."""
import ctypes

import numpy as np
import pytest

from mibminet import lib
from mibminet.params import ParamSet
from support import aligned, loaded  # noqa: F401 (loaded: a fixture)

INV, NOP, RNG, OK = lib.NET_ERR_INVALID, lib.NET_ERR_NO_PARAMS, lib.NET_ERR_RANGE, lib.NET_OK
T = 1125


def test_ctypes_signatures():
    L = lib.load()
    names = lambda fn: [t.__name__ for t in fn.argtypes]
    assert names(L.net_model_compute_windows_at) == ["c_void_p", "c_int", "c_ulong", "c_void_p", "c_ulong", "c_void_p",
                                                     "c_void_p", "c_void_p", "c_ulong", "c_int", "c_void_p"]
    assert names(L.net_model_compute_windows_at_f32) == ["c_void_p", "c_ulong", "c_void_p", "c_ulong", "c_float",
                                                         "c_void_p", "c_void_p", "c_void_p", "c_ulong", "c_int",
                                                         "c_void_p"]
    assert L.net_model_compute_windows_at.restype is ctypes.c_int
    assert L.net_model_compute_windows_at_f32.restype is ctypes.c_int
    assert names(L.net_windows_multi_count) == ["c_void_p", "c_ulong", "c_ulong"]
    assert names(L.net_windows_multi_onsets) == ["c_void_p", "c_ulong", "c_ulong", "c_void_p", "c_ulong", "c_void_p"]
    assert L.net_windows_multi_count.restype is ctypes.c_size_t
    assert L.net_windows_multi_onsets.restype is ctypes.c_size_t


def test_invalid_arguments_without_a_gpu(loaded):
    fn = lib.load().net_model_compute_windows_at
    L, W = 4000, 9
    wsb = lib.windows_workspace(L)
    keep, ws = aligned(128)
    x, y, on, nb = ws + 16, ws + 32, ws + 48, ws + 64  # never read: every call below fails a check
    for layout in (2, 3, -1):
        assert fn(x, layout, L, on, W, y, nb, ws, wsb, 0, None) == INV
    assert fn(None, 1, L, on, W, y, nb, ws, wsb, 0, None) == INV   # null x, y, onsets, ws with W > 0
    assert fn(x, 0, L, on, W, None, nb, ws, wsb, 0, None) == INV
    assert fn(x, 1, L, None, W, y, nb, ws, wsb, 0, None) == INV
    assert fn(x, 1, L, on, W, y, nb, None, wsb, 0, None) == INV
    for off in (1, 2, 3):
        assert fn(x, 1, L, on, W, y + off, nb, ws, wsb, 0, None) == INV   # logits not 4-byte aligned
        assert fn(x, 1, L, on, W, y, nb + off, ws, wsb, 0, None) == INV   # counter not 4-byte aligned
    for off in (1, 2, 4, 7):
        assert fn(x, 1, L, on + off, W, y, nb, ws, wsb, 0, None) == INV   # onsets not 8-byte aligned
    for off in (1, 4, 8):
        assert fn(x, 1, L, on, W, y, nb, ws + off, wsb, 0, None) == INV   # workspace not 16-byte aligned
    assert fn(x, 1, L, on, W, y, nb, ws, wsb - 1, 0, None) == INV         # workspace too small
    assert fn(x, 1, L, on, W, y, nb, ws, 0, 0, None) == INV
    assert fn(x, 1, T - 1, on, 1, y, nb, ws, lib.windows_workspace(T - 1), 0, None) == INV  # W > 0 with L < T
    assert fn(x, 0, 0, on, 1, y, nb, ws, 0, 0, None) == INV
    assert fn(x, 1, L, on, 2**31 - 65535, y, nb, ws, wsb, 0, None) == INV  # W > INT32_MAX - 65,535
    assert fn(x, 1, L, on, 2**40, y, nb, ws, wsb, 0, None) == INV
    for dev in (-1, 1 << 20):
        assert fn(x, 1, L, on, W, y, nb, ws, wsb, dev, None) == INV
    # one buffer view with 32-bit offsets: L max(16, C) >= 2^31 (C = 22)
    big = -(-2**31 // 22)
    assert big * 22 >= 2**31 > (big - 1) * 22
    for Lb in (big, 2**31, 2**40, 2**63):
        assert fn(x, 1, Lb, on, W, y, nb, ws, 2**62, 0, None) == INV
        assert fn(x, 0, Lb, on, W, y, nb, ws, 2**62, 0, None) == INV
    # no window: nothing to do, whatever x, y and the onsets are (n_bad may be NULL)
    assert fn(None, 1, L, None, 0, None, None, ws, wsb, 0, None) == OK
    assert fn(None, 0, T - 1, None, 0, None, nb, ws, lib.windows_workspace(T - 1), 0, None) == OK
    assert fn(None, 0, 0, None, 0, None, None, None, 0, 0, None) == OK


def test_float_entry_checks(loaded):
    fn = lib.load().net_model_compute_windows_at_f32
    L, W = 4000, 9
    wsb = lib.windows_workspace(L)
    keep, ws = aligned(128)
    x, y, on, nb = ws + 16, ws + 32, ws + 48, ws + 64
    for scale in (0.0, -1.0, float("nan"), float("inf")):
        assert fn(x, L, on, W, scale, y, nb, ws, wsb, 0, None) == INV
    for scale in (2.0**-61, 2.0**61, 1e-30, 3e38):
        assert fn(x, L, on, W, scale, y, nb, ws, wsb, 0, None) == RNG
    for off in (1, 2, 3):
        assert fn(x + off, L, on, W, 1.0, y, nb, ws, wsb, 0, None) == INV  # float32 not 4-byte aligned
    big = -(-2**31 // 88)  # C sizeof(float) = 88 bytes per sample
    assert fn(x, big, on, W, 1.0, y, nb, ws, 2**62, 0, None) == INV
    assert fn(x, T - 1, on, 1, 1.0, y, nb, ws, lib.windows_workspace(T - 1), 0, None) == INV
    assert fn(x, L, on + 4, W, 1.0, y, nb, ws, wsb, 0, None) == INV
    assert fn(None, L, None, 0, 1.0, None, None, ws, wsb, 0, None) == OK


def test_sixteen_bytes_per_sample_limit_with_few_channels():
    """C < 16: the workspace rows (16 bytes per sample over the 16 filters) set the limit."""
    lib.params_load(ParamSet.synthetic(seed=3, C=5, T=100, N=16))
    keep, ws = aligned(128)
    x, y, on = ws + 16, ws + 32, ws + 48
    assert lib.load().net_model_compute_windows_at(x, 1, 2**27, on, 3, y, None, ws, 2**62, 0, None) == INV
    assert lib.load().net_model_compute_windows_at_f32(x, 2**27, on, 3, 1.0, y, None, ws, 2**62, 0, None) == INV
    lib.params_unload()


def test_no_params_comes_first():
    lib.params_unload()
    L = lib.load()
    assert L.net_model_compute_windows_at(None, 7, 0, 3, 5, 1, 2, 1, 0, -1, None) == NOP
    assert L.net_model_compute_windows_at(None, 1, 4000, None, 0, None, None, None, 0, 0, None) == NOP
    assert L.net_model_compute_windows_at_f32(None, 4000, 4, 1, 0.0, None, 1, 3, 0, 0, None) == NOP


# ---- the onset lists of many recordings -----------------------------------------------------
def _restate(lengths, hop, T):
    """The issue's definition, restated."""
    onsets, first, start = [], [0], 0
    for n in lengths:
        onsets += [start + k * hop for k in range(0 if n < T else (n - T) // hop + 1)]
        first.append(len(onsets))
        start += n
    return onsets, first


def _c_multi(lengths, hop, cap=None, want_first=True, fill=0x5A):
    R = len(lengths)
    arr = (ctypes.c_size_t * max(R, 1))(*lengths)
    A = lib.load()
    W = A.net_windows_multi_count(arr, R, hop)
    cap = W if cap is None else cap
    onsets = np.full(cap + 1, fill, np.int64)
    first = (ctypes.c_size_t * (R + 1))(*([fill] * (R + 1)))
    got = A.net_windows_multi_onsets(arr, R, hop, onsets.ctypes.data, cap, first if want_first else None)
    return W, got, onsets, list(first)


def _length_lists(T, hop, rng):
    special = [0, T - 1, T, T + hop - 1, T + hop, 1, 2 * T + 1]
    yield []
    yield [0]
    yield [T - 1, 0, T - 1]
    yield special
    for _ in range(6):
        n = int(rng.integers(1, 9))
        yield [int(rng.choice(special)) if rng.random() < 0.5 else int(rng.integers(0, 4 * T)) for _ in range(n)]


@pytest.mark.parametrize("hop", [1, 7, 8, 1125, 1126, 5000])
def test_multi_onsets_against_the_definition(hop, loaded):
    rng = np.random.default_rng(hop)
    for lengths in _length_lists(T, hop, rng):
        want_on, want_first = _restate(lengths, hop, T)
        W, got, onsets, first = _c_multi(lengths, hop)
        assert W == got == len(want_on), lengths
        assert onsets[:W].tolist() == want_on and onsets[W] == 0x5A, lengths
        assert first == want_first, lengths
        assert all(a <= b for a, b in zip(first, first[1:])) and first[-1] == W
        # each recording's count is net_windows_count's
        assert [b - a for a, b in zip(first, first[1:])] == [lib.windows_count(n, hop) for n in lengths]
        # the Python wrapper
        on_py, first_py = lib.windows_multi_onsets(lengths, hop)
        assert on_py.dtype == np.int64 and on_py.tolist() == want_on and first_py == want_first


def test_multi_onsets_follow_the_loaded_T():
    lib.params_load(ParamSet.synthetic(seed=5, C=19, T=480, N=3))
    lengths = [480 + 5 * 7 + 3, 0, 479, 480, 487, 961]
    on, first = lib.windows_multi_onsets(lengths, 7)
    assert (on.tolist(), first) == _restate(lengths, 7, 480)
    assert first == [0, 6, 6, 6, 7, 9, 78]
    lib.params_unload()


def test_multi_onsets_cap_and_null_arguments(loaded):
    lengths, hop = [T + 20, T - 1, T + 8], 8
    want_on, want_first = _restate(lengths, hop, T)
    W = len(want_on)
    assert W == 5
    for cap in (0, 1, W - 1):  # too small: nothing written, W still returned, first still filled
        Wc, got, onsets, first = _c_multi(lengths, hop, cap=cap)
        assert Wc == got == W and (onsets == 0x5A).all() and first == want_first
    Wc, got, onsets, first = _c_multi(lengths, hop, cap=W + 3)
    assert got == W and onsets[:W].tolist() == want_on and (onsets[W:] == 0x5A).all()
    Wc, got, onsets, first = _c_multi(lengths, hop, want_first=False)
    assert got == W and onsets[:W].tolist() == want_on
    arr = (ctypes.c_size_t * 3)(*lengths)
    assert lib.load().net_windows_multi_onsets(arr, 3, hop, None, 1 << 20, None) == W  # null onsets: the count
    assert lib.load().net_windows_multi_count(None, 0, hop) == 0                        # R == 0


def test_multi_onsets_return_zero(loaded):
    A = lib.load()
    arr = (ctypes.c_size_t * 2)(T + 9, T + 1)
    first = (ctypes.c_size_t * 3)(7, 7, 7)
    on = np.full(64, 0x5A, np.int64)
    assert A.net_windows_multi_count(arr, 2, 0) == 0  # hop == 0
    assert A.net_windows_multi_onsets(arr, 2, 0, on.ctypes.data, 64, first) == 0
    over = (ctypes.c_size_t * 3)(2**63 - 1, T, 2**62)  # the sum overflows
    assert A.net_windows_multi_count(over, 3, 2**40) == 0
    assert A.net_windows_multi_onsets(over, 3, 2**40, on.ctypes.data, 64, first) == 0
    wrap = (ctypes.c_size_t * 2)(2**64 - 1, 2)
    assert A.net_windows_multi_count(wrap, 2, 2**40) == 0
    lib.params_unload()  # no set loaded
    assert A.net_windows_multi_count(arr, 2, 8) == 0
    assert A.net_windows_multi_onsets(arr, 2, 8, on.ctypes.data, 64, first) == 0
    assert list(first) == [7, 7, 7] and (on == 0x5A).all()  # an error writes nothing
    with pytest.raises(lib.NetError):
        lib.windows_multi_onsets([T], 8)
    lib.params_load(ParamSet.synthetic(seed=5))
    for lengths, hop in (([T], 0), ([T, -1], 8), ([2**63 - 1, 1], 8)):
        with pytest.raises(ValueError):
            lib.windows_multi_onsets(lengths, hop)


# ---- the chunk planner -------------------------------------------------------------------------
def test_plan_chunks_properties():
    rng = np.random.default_rng(11)
    for trial in range(200):
        R = int(rng.integers(0, 12))
        per = int(rng.choice([16, 22, 64, 88, 256]))
        lengths = [int(v) for v in rng.integers(0, 50, size=R)]
        if R and rng.random() < 0.3:
            lengths[int(rng.integers(0, R))] = 0
        limit = per * int(rng.integers(50, 160))  # every recording (< 50 samples) is under the limit
        chunks = lib._plan_chunks(lengths, per, limit)
        # every recording in exactly one chunk, in order, no empty chunk
        assert [r for a, b in chunks for r in range(a, b)] == list(range(R))
        assert all(a < b for a, b in chunks)
        size = lambda a, b: sum(lengths[a:b]) * per
        # no chunk reaches the limit
        assert all(size(a, b) < limit for a, b in chunks)
        # greedy-maximal: the next chunk's first recording would not have fitted
        for (a, b), (b2, c) in zip(chunks, chunks[1:]):
            assert b == b2 and size(a, b + 1) >= limit
    assert lib._plan_chunks([], 16, 100) == []
    assert lib._plan_chunks([0, 0], 16, 1) == [(0, 2)]
    assert lib._plan_chunks([3, 3, 3], 16, 16 * 6 + 1) == [(0, 2), (2, 3)]
    assert lib._plan_chunks([3, 3, 3], 16, 16 * 6) == [(0, 1), (1, 2), (2, 3)]   # "below": 6 samples do not fit
    assert lib._plan_chunks([2**27 - 1] * 3, 16, 2**31) == [(0, 1), (1, 2), (2, 3)]


def test_plan_chunks_rejects_a_recording_over_the_limit():
    for lengths, per, limit in (([5, 100, 5], 16, 1600), ([101], 16, 1600), ([2**27], 16, 2**31),
                                ([1, -(-2**31 // 88)], 88, 2**31)):
        with pytest.raises(ValueError, match="overlap"):
            lib._plan_chunks(lengths, per, limit)


def test_python_entries_reject_host_tensors_and_wrong_types(loaded):
    """The torch entries refuse what is not a device recording before any pointer is taken."""
    import torch

    x = torch.zeros((22, 2000), dtype=torch.int8)
    for kw in (dict(), dict(layout="tc"), dict(layout="xx"), dict(scale=1.0), dict(check=False)):
        with pytest.raises(ValueError):
            lib.forward_windows_at_torch(x, [0, 8], **kw)
    for bad in (x.to(torch.float32), x.to(torch.int16), x.to(torch.float64), np.zeros((22, 2000), np.int8)):
        with pytest.raises(ValueError):
            lib.forward_windows_at_torch(bad, [0], scale=1.0)
    for rec in ([x], [x, x], (x, [2000]), (x, [1000, 1000]), [], [np.zeros((22, 2000), np.int8)],
                [x.to(torch.float32)]):
        with pytest.raises(ValueError):
            lib.forward_windows_multi_torch(rec, 8)
    with pytest.raises(ValueError):
        lib.forward_windows_multi_torch([x], 0)
    with pytest.raises(ValueError):
        lib.forward_windows_multi_torch([x], 8, layout="xx")
