"""The parameter images as pinned bytes (no GPU): for ten sets, loaded normally and on the general
path (mibminet_test_force_general), the FNV-1a digest of the batched kernels' image, what
net_params_info reports and the folded-filter count; the window kernels' image of a normal load is
the general image of the same set (both are laid out from one requant plan, images.hpp)."""
import ctypes

import pytest

from mibminet import lib
from mibminet.params import ParamSet

S, X = ParamSet.synthetic, ParamSet.synthetic_extreme

# (set, digest of a normal load, digest under force_general, path, (layer, filter) of the first
# unproven requant, exact division, folded filters).  The digests were taken before the host library
# was split into headers, except the three force_general digests marked "plan": those are
# gen::GenParams images on the exact-division path, which used to carry whatever float constants
# were proven before the first unproven requant.  The exact-division kernels read none of them, and
# the requant plan leaves them zero (l1_r, l1_c, l2_r, l2_c, l3_r, l3_c, sg.l4_r, sg.l4_c, sg.l4_ci);
# every other byte of those images is what it was (0x9ac8cb6cbfd30bfc, 0x3d9d268dc4fc7608 and
# 0xc536a2f9bb5612a8 before).
ROWS = [
    (lambda: S(seed=42), 0x4CB99661AE2E985F, 0x62C068192A10D240, "float", (0, -1), False, 0),
    (lambda: S(seed=11, C=64, T=480, reorder_bn=False, clip_balanced=True), 0x26BE86B5FF09FE11, 0xA16C3DCD74DBE89C,
     "float", (0, -1), False, 0),
    (lambda: S(seed=5, weight_bits=4), 0xF07E14F27F874034, 0x95498DF6658C7CD3, "float", (0, -1), False, 0),
    (lambda: X(seed=77, mids=0), 0xDCBEF0D736030AC9, 0x34FFA648D22236AC, "float", (0, -1), False, 15),
    (lambda: X(seed=77, mids=3), 0x34B6676BA8094F89, 0xD1B7969D33B1A627, "exact", (1, 1), True, 14),  # plan
    (lambda: X(seed=78, mids=3, reorder_bn=False), 0x983A5A7FBC4895E1, 0x44003711BD83F9D8, "exact", (1, 0), True,
     15),  # plan
    (lambda: S(seed=3, C=3, T=64, N=1), 0x1D5848C8AD998815, 0x1D5848C8AD998815, "general", (0, -1), False, 0),
    (lambda: S(seed=4, C=19, T=1125, N=3), 0xC434B9F175686C68, 0xC434B9F175686C68, "general", (0, -1), False, 0),
    (lambda: S(seed=6, C=64, T=4096, N=16), 0xC44B5C39C8356693, 0xC44B5C39C8356693, "general", (0, -1), False, 0),
    (lambda: X(seed=79, C=38, T=480, N=2, mids=3), 0x8FF2E4FC03D11552, 0x8FF2E4FC03D11552, "general", (0, -1), True,
     14),  # plan
]
SHAPES = {(22, 1125, 4): 0, (64, 1000, 4): 1, (64, 480, 4): 2}


def _fnv(b):
    h = 1469598103934665603
    for x in b:
        h = ((h ^ x) * 1099511628211) & (2 ** 64 - 1)
    return h


def _digest():
    A = lib.load()
    A.mibminet_test_image_digest.argtypes = [ctypes.c_void_p]
    v = ctypes.c_uint64(0)
    assert A.mibminet_test_image_digest(ctypes.byref(v)) == lib.NET_OK
    return v.value


def _image(which):
    """(return code, bytes) of mibminet_test_image_copy."""
    A = lib.load()
    A.mibminet_test_image_copy.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    n = ctypes.c_size_t(12345)
    rc = A.mibminet_test_image_copy(which, None, 0, ctypes.byref(n))
    if rc:
        assert n.value == 0
        return rc, b""
    buf = ctypes.create_string_buffer(n.value)
    assert A.mibminet_test_image_copy(which, buf, n.value - 1, ctypes.byref(n)) == lib.NET_ERR_INVALID
    assert n.value == len(buf)
    assert A.mibminet_test_image_copy(which, buf, n.value, ctypes.byref(n)) == lib.NET_OK
    return rc, buf.raw


@pytest.fixture(autouse=True)
def _clean():
    yield
    lib.force_general(False)
    lib.params_unload()


@pytest.mark.parametrize("row", range(len(ROWS)))
def test_images_are_pinned(row):
    make, normal, general, path, first, exact, folded = ROWS[row]
    ps = make()
    d = ps.dims
    shape = SHAPES.get((d.C, d.T, d.N), -1)
    lib.params_load(ps)
    assert _digest() == normal
    rc, img0 = _image(0)
    assert rc == lib.NET_OK and _fnv(img0) == normal
    info = lib.params_info()
    assert (info["path"], info["layer"], info["filter"]) == (path, *first)
    assert info["shape"] == shape and info["exact_division"] == exact
    assert lib.folded_filters() == folded
    rc, img1 = _image(1)
    assert rc == lib.NET_OK and _fnv(img1) == general  # the window kernels' image
    lib.force_general(True)
    lib.params_load(ps)
    assert _digest() == general
    info = lib.params_info()
    assert (info["path"], info["layer"], info["filter"], info["shape"]) == ("general", 0, -1, -1)
    assert info["exact_division"] == exact and lib.folded_filters() == folded
    assert _image(0) == (lib.NET_OK, img1) and _image(1) == (lib.NET_OK, img1)


def test_image_copy_without_an_image():
    A = lib.load()
    A.mibminet_test_image_copy.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    lib.params_unload()
    assert _image(0) == (lib.NET_ERR_NO_PARAMS, b"") and _image(1) == (lib.NET_ERR_NO_PARAMS, b"")
    lib.params_load(S(seed=42))
    assert _image(2)[0] == lib.NET_ERR_INVALID and _image(-1)[0] == lib.NET_ERR_INVALID
    assert A.mibminet_test_image_copy(0, None, 0, None) == lib.NET_ERR_INVALID
