"""The parameter images as pinned bytes (no GPU): for ten sets, loaded normally and on the general
path (mibminet_test_force_general), the FNV-1a digest of the batched kernels' image, what
net_params_info reports and the folded-filter count; the window kernels' image of a normal load is
the general image of the same set (both are laid out from one requant plan, images.hpp)."""
import ctypes

import pytest

from mibminet import lib
from mibminet.params import ParamSet
from support import ROWS

SHAPES = {(22, 1125, 4): 0, (64, 1000, 4): 1, (64, 480, 4): 2}


def _fnv(b):
    h = 1469598103934665603
    for x in b:
        h = ((h ^ x) * 1099511628211) & (2 ** 64 - 1)
    return h


def _image(which):
    """(return code, bytes) of mibminet_test_image_copy."""
    A = lib.load()
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
    assert lib.image_digest() == normal
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
    assert lib.image_digest() == general
    info = lib.params_info()
    assert (info["path"], info["layer"], info["filter"], info["shape"]) == ("general", 0, -1, -1)
    assert info["exact_division"] == exact and lib.folded_filters() == folded
    assert _image(0) == (lib.NET_OK, img1) and _image(1) == (lib.NET_OK, img1)


def test_image_copy_without_an_image():
    lib.params_unload()
    assert _image(0) == (lib.NET_ERR_NO_PARAMS, b"") and _image(1) == (lib.NET_ERR_NO_PARAMS, b"")
    lib.params_load(ParamSet.synthetic(seed=42))
    assert _image(2)[0] == lib.NET_ERR_INVALID and _image(-1)[0] == lib.NET_ERR_INVALID
    assert lib.load().mibminet_test_image_copy(0, None, 0, None) == lib.NET_ERR_INVALID
