"""Sliding windows over a recording (net_model_compute_windows): the counts, the workspace layout
and every argument check, none of which needs a GPU.  Every call here either fails a check or has
no window (W == 0), so nothing is launched where a GPU is present either; the pointers are host
buffers that no call reads."""
import ctypes

import numpy as np
import pytest

from mibminet import lib
from mibminet.params import ParamSet
from support import aligned, loaded  # noqa: F401 (loaded: a fixture)

INV, NOP, RNG, OK = lib.NET_ERR_INVALID, lib.NET_ERR_NO_PARAMS, lib.NET_ERR_RANGE, lib.NET_OK


def test_windows_count(loaded):
    T = 1125
    assert lib.windows_count(T - 1, 1) == 0 and lib.windows_count(0, 1) == 0
    assert lib.windows_count(T, 1) == 1 and lib.windows_count(T, 5000) == 1
    assert lib.windows_count(T + 1, 1) == 2 and lib.windows_count(T + 7, 8) == 1 and lib.windows_count(T + 8, 8) == 2
    assert lib.windows_count(T + 4999, 5000) == 1 and lib.windows_count(T + 5000, 5000) == 2  # hop > T: gaps
    assert lib.windows_count(10 * T, 2000) == (10 * T - T) // 2000 + 1
    assert lib.windows_count(10 * T, 0) == 0
    lib.params_unload()
    assert lib.windows_count(10 * T, 1) == 0


def test_windows_count_follows_the_loaded_T():
    lib.params_load(ParamSet.synthetic(seed=5, C=19, T=480, N=3))
    assert lib.windows_count(479, 1) == 0 and lib.windows_count(480, 1) == 1 and lib.windows_count(1000, 16) == 33
    lib.params_unload()


@pytest.mark.parametrize("L", [0, 1, 15, 16, 17, 1125, 1136, 2**20 + 1, 97612893])
def test_workspace_layout(L):
    rs = lib.windows_row_stride(L)
    assert rs >= L and rs % 16 == 0 and rs < L + 16
    assert lib.windows_workspace(L) == 16 * rs


def test_ctypes_signatures():
    L = lib.load()
    names = lambda fn: [t.__name__ for t in fn.argtypes]
    assert names(L.net_model_compute_windows) == ["c_void_p", "c_int", "c_ulong", "c_ulong", "c_void_p", "c_void_p",
                                                  "c_ulong", "c_int", "c_void_p"]
    assert names(L.net_model_compute_windows_f32) == ["c_void_p", "c_ulong", "c_ulong", "c_float", "c_void_p",
                                                      "c_void_p", "c_ulong", "c_int", "c_void_p"]
    assert L.net_model_compute_windows.restype is ctypes.c_int
    assert L.net_model_compute_windows_f32.restype is ctypes.c_int
    assert names(L.net_windows_count) == ["c_ulong", "c_ulong"] and L.net_windows_count.restype is ctypes.c_size_t
    assert L.net_windows_workspace.restype is ctypes.c_size_t and L.net_windows_row_stride.restype is ctypes.c_size_t


def test_invalid_arguments_without_a_gpu(loaded):
    fn = lib.load().net_model_compute_windows
    L, hop = 4000, 8
    wsb = lib.windows_workspace(L)
    keep, ws = aligned(64)
    x, y = ws + 16, ws + 32  # never read: every call below fails a check
    assert fn(x, 1, L, 0, y, ws, wsb, 0, None) == INV            # hop == 0
    for layout in (2, 3, -1):
        assert fn(x, layout, L, hop, y, ws, wsb, 0, None) == INV
    assert fn(None, 1, L, hop, y, ws, wsb, 0, None) == INV       # null x, y, ws with W > 0
    assert fn(x, 0, L, hop, None, ws, wsb, 0, None) == INV
    assert fn(x, 1, L, hop, y, None, wsb, 0, None) == INV
    for off in (1, 4, 8):
        assert fn(x, 1, L, hop, y, ws + off, wsb, 0, None) == INV  # workspace not 16-byte aligned
    assert fn(x, 1, L, hop, y, ws, wsb - 1, 0, None) == INV      # workspace too small
    assert fn(x, 1, L, hop, y, ws, 0, 0, None) == INV
    assert fn(x, 1, L, hop, y + 2, ws, wsb, 0, None) == INV      # logits not 4-byte aligned
    assert fn(x, 1, L, hop, y, ws, wsb, -1, None) == INV
    # one buffer view with 32-bit offsets: L max(16, C) >= 2^31 (C = 22)
    big = -(-2**31 // 22)
    assert big * 22 >= 2**31 > (big - 1) * 22
    for Lb in (big, 2**31, 2**40):
        assert fn(x, 1, Lb, 2**20, y, ws, 2**62, 0, None) == INV
        assert fn(x, 0, Lb, 2**20, y, ws, 2**62, 0, None) == INV
    # W > INT32_MAX - 65,535 (such a recording is also past the offset limit)
    assert lib.windows_count(2**32, 1) > 2**31 - 65536
    assert fn(x, 1, 2**32, 1, y, ws, 2**62, 0, None) == INV
    # no window: nothing to do, whatever x and y are
    assert fn(None, 1, 1124, 1, None, ws, lib.windows_workspace(1124), 0, None) == OK
    assert fn(None, 0, 0, 3, None, ws, 0, 0, None) == OK


def test_offset_limit_counts_float_elements(loaded):
    fn = lib.load().net_model_compute_windows_f32
    keep, ws = aligned(64)
    x, y = ws + 16, ws + 32
    big = -(-2**31 // 88)  # C sizeof(float) = 88 bytes per sample
    assert fn(x, big, 2**20, 1.0, y, ws, 2**62, 0, None) == INV
    assert fn(x + 2, 4000, 8, 1.0, y, ws, lib.windows_workspace(4000), 0, None) == INV  # float32 not 4-byte aligned


def test_sixteen_bytes_per_sample_limit_with_few_channels():
    """C < 16: the workspace rows (16 bytes per sample over the 16 filters) set the limit."""
    lib.params_load(ParamSet.synthetic(seed=3, C=5, T=100, N=16))
    keep, ws = aligned(64)
    assert lib.load().net_model_compute_windows(ws + 16, 1, 2**27, 2**20, ws + 32, ws, 2**62, 0, None) == INV
    assert lib.load().net_model_compute_windows_f32(ws + 16, 2**27, 2**20, 1.0, ws + 32, ws, 2**62, 0, None) == INV
    lib.params_unload()


def test_float_scale_domain(loaded):
    fn = lib.load().net_model_compute_windows_f32
    L, hop = 4000, 8
    wsb = lib.windows_workspace(L)
    keep, ws = aligned(64)
    x, y = ws + 16, ws + 32
    for scale in (0.0, -1.0, float("nan"), float("inf")):
        assert fn(x, L, hop, scale, y, ws, wsb, 0, None) == INV
    for scale in (2.0**-61, 2.0**61, 1e-30, 3e38):
        assert fn(x, L, hop, scale, y, ws, wsb, 0, None) == RNG
    assert fn(x, L, 0, 1.0, y, ws, wsb, 0, None) == INV
    assert fn(None, 1124, 1, 1.0, None, ws, lib.windows_workspace(1124), 0, None) == OK


def test_no_params_comes_first():
    lib.params_unload()
    L = lib.load()
    assert L.net_model_compute_windows(None, 7, 0, 0, None, 1, 0, -1, None) == NOP
    assert L.net_model_compute_windows(None, 1, 4000, 8, None, None, 0, 0, None) == NOP
    assert L.net_model_compute_windows_f32(None, 4000, 0, 0.0, None, 3, 0, 0, None) == NOP


def test_python_entries_reject_host_tensors_and_unknown_layouts(loaded):
    """The torch entries refuse what is not a device recording before any pointer is taken."""
    import torch

    x = torch.zeros((22, 2000), dtype=torch.int8)
    for kw in (dict(), dict(layout="tc"), dict(layout="xx"), dict(layout=1)):
        with pytest.raises(ValueError):
            lib.forward_windows_torch(x, 8, **kw)
    with pytest.raises(ValueError):
        lib.forward_windows_f32_torch(x.to(torch.float32), 8, 1.0)
    with pytest.raises(ValueError):
        lib.forward_windows_torch(np.zeros((22, 2000), np.int8), 8)


@pytest.mark.parametrize("kw,digest,shape", [
    (dict(seed=42), 0x4CB99661AE2E985F, 0),
    (dict(seed=9, C=64, T=1000), 0x4572132575AB237C, 1),
    (dict(seed=11, C=64, T=480, reorder_bn=False, clip_balanced=True), 0x26BE86B5FF09FE11, 2),
])
def test_compiled_sets_keep_their_image_and_path(kw, digest, shape):
    """The window kernels' parameter image of a compiled geometry is built at load beside the
    compiled kernels' image, which stays what it was (digests taken before the window kernels
    existed), as does what net_params_info reports."""
    lib.params_load(ParamSet.synthetic(**kw))
    assert lib.image_digest() == digest
    info = lib.params_info()
    assert info["path"] == "float" and info["shape"] == shape and not info["exact_division"]
    lib.params_unload()


@pytest.mark.parametrize("mids,path", [(0, "float"), (3, "exact")])
def test_compiled_extreme_sets_keep_their_path(mids, path):
    lib.params_load(ParamSet.synthetic_extreme(seed=77, mids=mids))
    info = lib.params_info()
    assert info["path"] == path and info["shape"] == 0 and info["exact_division"] == (mids > 0)
    lib.params_unload()
