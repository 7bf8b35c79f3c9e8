"""ctypes binding of libmibminet.so (include/mibminet.h) — the Python mirror of the reference's
C model/layer API (edge-eegnet_wolf/src/cl/net/model.h, layers.h).

There is no CPU fallback: if the library cannot be loaded, or a call fails, a ``NetError`` is
raised.  Single-trial functions take host NumPy arrays in the reference layouts; the batched
function takes device pointers (e.g. ``torch.Tensor.data_ptr()`` of CUDA/HIP tensors).
"""
from __future__ import annotations

import ctypes
import os
from typing import Optional

import numpy as np

from .params import ParamSet

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmibminet.so")

NET_OK = 0
NET_ERR_INVALID = -1
NET_ERR_NO_PARAMS = -2
NET_ERR_UNSUPPORTED = -3
NET_ERR_BLOB = -4
NET_ERR_RANGE = -5
NET_ERR_HIP = -100

# Every C function the library declares, as "return (arguments)" in the words of _CTYPES: the net_*
# entries in the order of include/mibminet.h, then every hook of include/mibminet_testing.h in that
# header's order.  tests/test_lib_cpu.py holds each to its declaration in its header, so tests and
# tools call the hooks through load() or the wrappers below and bind nothing themselves.
_CTYPES = {"void": None, "int": ctypes.c_int, "size_t": ctypes.c_size_t, "int32_t": ctypes.c_int32,
           "int64_t": ctypes.c_int64, "float": ctypes.c_float, "double": ctypes.c_double,
           "ptr": ctypes.c_void_p, "str": ctypes.c_char_p}
PROTOTYPES = {
    "net_model_compute": "void (ptr, ptr)",
    "net_forward": "int (ptr, ptr)",
    "net_layer1": "void (ptr, ptr)",
    "net_layer2": "void (ptr, ptr)",
    "net_layer3": "void (ptr, ptr)",
    "net_layer3_flip_inplace": "void (ptr)",
    "net_layer4": "void (ptr, ptr)",
    "net_layer5": "void (ptr, ptr)",
    "net_last_error": "int ()",
    "net_params_load": "int (ptr, size_t)",
    "net_params_info": "int (ptr)",
    "net_blob_widen": "int (ptr, size_t, int, ptr, ptr, size_t, ptr)",
    "net_params_load_arrays": "int (ptr)",
    "net_params_dims": "int (ptr)",
    "net_params_unload": "void ()",
    "net_trial_stride": "size_t ()",
    "net_model_compute_batch": "int (ptr, ptr, size_t, int)",
    "net_model_compute_batch_ct_sync": "int (ptr, ptr, size_t, int)",
    "net_model_compute_batch_async": "int (ptr, ptr, size_t, int, ptr)",
    "net_model_compute_batch_ct": "int (ptr, ptr, size_t, int, ptr)",
    "net_model_compute_batch_f32": "int (ptr, ptr, size_t, float, int, ptr)",
    "net_windows_count": "size_t (size_t, size_t)",
    "net_windows_row_stride": "size_t (size_t)",
    "net_windows_workspace": "size_t (size_t)",
    "net_model_compute_windows": "int (ptr, int, size_t, size_t, ptr, ptr, size_t, int, ptr)",
    "net_model_compute_windows_f32": "int (ptr, size_t, size_t, float, ptr, ptr, size_t, int, ptr)",
    "net_model_compute_windows_f32_tm": "int (ptr, size_t, size_t, float, ptr, ptr, size_t, int, ptr)",
    "net_model_compute_windows_at": "int (ptr, int, size_t, ptr, size_t, ptr, ptr, ptr, size_t, int, ptr)",
    "net_model_compute_windows_at_f32": "int (ptr, size_t, ptr, size_t, float, ptr, ptr, ptr, size_t, int, ptr)",
    "net_model_compute_windows_at_f32_tm": "int (ptr, size_t, ptr, size_t, float, ptr, ptr, ptr, size_t, int, ptr)",
    "net_windows_multi_count": "size_t (ptr, size_t, size_t)",
    "net_windows_multi_onsets": "size_t (ptr, size_t, size_t, ptr, size_t, ptr)",
    "net_model_compute_epochs": "int (ptr, size_t, size_t, ptr, ptr, size_t, ptr, ptr, int, ptr)",
    "net_model_compute_epochs_f32": "int (ptr, size_t, size_t, ptr, ptr, size_t, float, ptr, ptr, int, ptr)",
    "net_bank_create": "int (ptr, ptr, ptr, size_t, ptr, ptr)",
    "net_bank_info": "int (ptr, ptr)",
    "net_bank_destroy": "void (ptr)",
    "net_bank_replace": "int (ptr, size_t, ptr, size_t, float, int, ptr)",
    "net_bank_feature_bytes": "size_t (ptr)",
    "net_model_compute_epochs_bank": "int (ptr, ptr, size_t, size_t, ptr, ptr, ptr, size_t, ptr, ptr, int, ptr)",
    "net_model_compute_epochs_bank_f32": "int (ptr, ptr, size_t, size_t, ptr, ptr, ptr, size_t, ptr, ptr, int, ptr)",
    "net_model_compute_epochs_bank_feat": "int (ptr, ptr, size_t, size_t, ptr, ptr, ptr, size_t, ptr, ptr, ptr, int, ptr)",
    "net_model_compute_epochs_bank_feat_f32": "int (ptr, ptr, size_t, size_t, ptr, ptr, ptr, size_t, ptr, ptr, ptr, int, ptr)",
    "net_model_compute_windows_bank": "int (ptr, ptr, int, size_t, ptr, ptr, size_t, ptr, ptr, ptr, size_t, int, ptr)",
    "net_model_compute_windows_bank_f32": "int (ptr, ptr, size_t, ptr, ptr, size_t, ptr, ptr, ptr, size_t, int, ptr)",
    "net_model_compute_windows_bank_f32_tm": "int (ptr, ptr, size_t, ptr, ptr, size_t, ptr, ptr, ptr, size_t, int, ptr)",
    "net_bank_windows_starts": "size_t (ptr, size_t, ptr)",
    "net_bank_windows_lists": "size_t (ptr, ptr, ptr, size_t, size_t, ptr, size_t, ptr, size_t, ptr)",
    "net_streams_ring_samples": "size_t (ptr, size_t)",
    "net_streams_push_windows": "size_t (ptr, size_t, size_t, size_t)",
    "net_streams_create": "int (ptr, ptr, size_t, size_t, size_t, int, ptr)",
    "net_streams_destroy": "void (ptr)",
    "net_streams_info": "int (ptr, ptr)",
    "net_streams_origin": "int (ptr, size_t, ptr, ptr)",
    "net_streams_push": "int (ptr, ptr, int, size_t, ptr, ptr, ptr)",
    "net_streams_push_f32": "int (ptr, ptr, size_t, ptr, ptr, ptr)",
    "net_streams_push_f32_tm": "int (ptr, ptr, size_t, ptr, ptr, ptr)",
    "net_streams_restart": "int (ptr, size_t, int32_t, ptr)",
    "net_streams_set_decimator": "int (ptr, size_t, ptr, size_t, ptr)",
    "net_streams_raw_samples": "size_t (size_t, size_t, size_t)",
    "net_streams_push_raw_f32_tm": "int (ptr, ptr, size_t, ptr, ptr, ptr)",
    "net_streams_raw_info": "int (ptr, ptr)",
    "net_streams_create_each": "int (ptr, ptr, size_t, size_t, size_t, int, ptr)",
    "net_streams_each_rows": "size_t (size_t, size_t)",
    "net_streams_push_each": "int (ptr, ptr, int, ptr, size_t, ptr, ptr, ptr, ptr, ptr)",
    "net_streams_push_each_f32": "int (ptr, ptr, ptr, size_t, ptr, ptr, ptr, ptr, ptr)",
    "net_streams_push_each_f32_tm": "int (ptr, ptr, ptr, size_t, ptr, ptr, ptr, ptr, ptr)",
    "net_streams_positions": "int (ptr, ptr, ptr)",
    "net_streams_set_decimator_each": "int (ptr, size_t, ptr, size_t, ptr)",
    "net_streams_each_raw_rows": "size_t (size_t, size_t, size_t)",
    "net_streams_push_each_raw_f32_tm": "int (ptr, ptr, ptr, size_t, ptr, ptr, ptr, ptr, ptr)",
    "net_streams_raw_positions": "int (ptr, ptr, ptr)",
    "net_streams_set_prefilter": "int (ptr, ptr, size_t, ptr)",
    "net_streams_prefilter_info": "int (ptr, ptr)",
    "net_streams_windows_at": "int (ptr, ptr, ptr, size_t, ptr, ptr, ptr)",
    "net_streams_windows_at_feat": "int (ptr, ptr, ptr, size_t, ptr, ptr, ptr, ptr)",
    "net_streams_at_span": "int (ptr, ptr, ptr)",
    "net_model_compute_batch_multi": "int (int, ptr, ptr, ptr, ptr, ptr)",
    "net_model_compute_batch_multi_ct": "int (int, ptr, ptr, ptr, ptr, ptr)",
    "net_quantize_input_f32": "int (ptr, ptr, size_t, int, int, float, int, ptr)",
    "net_quantize_input_f64": "int (ptr, ptr, size_t, int, int, double, int, ptr)",
    "net_argmax_batch": "int (ptr, ptr, size_t, int, int, ptr)",
    "net_pack_trials_i8": "int (ptr, ptr, size_t, int, int, int, ptr)",
    "net_set_device": "int (int)",
    "net_launch_info": "int (size_t, int, ptr)",
    "net_launch_info_ct": "int (size_t, int, ptr)",
    "net_error_string": "str (int)",
    "net_version": "int ()",
    "mibminet_test_reciprocal": "int (int32_t, int64_t, int32_t, int32_t, ptr, ptr)",
    "mibminet_test_floor_form": "int (int32_t, int64_t, int64_t, ptr, ptr, ptr)",
    "mibminet_test_quantize_f32": "int (ptr, ptr, size_t, float, int, ptr)",
    "mibminet_test_multi_order": "int (int, ptr, int, ptr, size_t)",
    "mibminet_test_upload_stats": "int (ptr, ptr)",
    "mibminet_test_device_images": "int (int)",
    "mibminet_test_xdiv_host": "int (ptr, size_t, int32_t, ptr)",
    "mibminet_test_xdiv_gpu": "int (int32_t, int64_t, int64_t, ptr, int)",
    "mibminet_test_pool_consts": "int (int32_t, int32_t, ptr, ptr)",
    "mibminet_test_params_xr": "int ()",
    "mibminet_test_force_general": "int (int)",
    "mibminet_test_grid_cap": "int (int)",
    "mibminet_test_image_digest": "int (ptr)",
    "mibminet_test_image_copy": "int (int, ptr, size_t, ptr)",
    "mibminet_test_folded_filters": "int (ptr)",
    "mibminet_test_bank_copy": "int (ptr, size_t, ptr, size_t, ptr)",
    "mibminet_test_bank_device_copies": "int (ptr)",
    "mibminet_test_streams_ring": "int (ptr, size_t, ptr)",
    "mibminet_test_streams_seek": "int (ptr, ptr, ptr)",
    "mibminet_test_fir_decimate": "int (ptr, size_t, size_t, ptr, ptr, size_t, size_t, size_t, ptr, int, ptr)",
    "mibminet_test_sos_filter": "int (ptr, size_t, size_t, ptr, size_t, ptr, ptr, ptr, int, ptr)",
}
EXPORTED_SYMBOLS = tuple(n for n in PROTOTYPES if n.startswith("net_"))
NET_PATH_FLOAT, NET_PATH_EXACT, NET_PATH_GENERAL = 0, 1, 2


class NetError(RuntimeError):
    def __init__(self, code: int, what: str = ""):
        self.code = code
        msg = _lib_error_string(code)
        super().__init__(f"{what}: {msg} (code {code})" if what else f"{msg} (code {code})")


_lib: Optional[ctypes.CDLL] = None


def _lib_error_string(code: int) -> str:
    try:
        return load().net_error_string(code).decode()
    except Exception:  # pragma: no cover - library missing
        return "error"


def prototype(name: str):
    """(restype, argtypes) of PROTOTYPES[name] as ctypes types."""
    ret, _, args = PROTOTYPES[name].rstrip(")").partition("(")
    return _CTYPES[ret.strip()], [_CTYPES[a.strip()] for a in args.split(",") if a.strip()]


def bind(L: ctypes.CDLL, names=None) -> ctypes.CDLL:
    """Gives the functions ``names`` (default: all of PROTOTYPES) their restype and argtypes on
    ``L``, a loaded build of the library.  load() binds everything on the one the package uses; the
    tools that time other builds side by side, some of an older revision, name what they call."""
    for name in PROTOTYPES if names is None else names:
        fn = getattr(L, name)
        fn.restype, fn.argtypes = prototype(name)
    return L


def load(path: str = LIB_PATH) -> ctypes.CDLL:
    """Load libmibminet.so (raises OSError — loudly — if it is missing or fails to load)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise OSError(f"libmibminet.so not found at {path}: build it with `make -C mi-bminet_amd`"
                      " (there is no CPU fallback)")
    _lib = bind(ctypes.CDLL(path))
    return _lib


def _check(rc: int, what: str) -> None:
    if rc != NET_OK:
        raise NetError(rc, what)


# ---- parameters -------------------------------------------------------------------------------
_loaded: Optional[ParamSet] = None


def _load_blob(blob: bytes, ps: Optional[ParamSet]) -> None:
    global _loaded
    buf = ctypes.create_string_buffer(blob, len(blob))
    _check(load().net_params_load(buf, len(blob)), "net_params_load")
    _loaded = ParamSet.from_blob(blob) if ps is None else ps


def params_load(ps: ParamSet) -> None:
    """net_params_load(blob) — replaces the generated net.h globals of the reference."""
    _load_blob(ps.to_blob(), ps)


def params_load_blob(blob: bytes) -> None:
    _load_blob(blob, None)


def blob_widen(blob: bytes, R: int, channels) -> bytes:
    """net_blob_widen: ``blob`` over ``R`` source rows, its channel c reading row ``channels[c]``
    (ParamSet.widened is the same transform in Python).  Host only."""
    ch = [int(c) for c in channels]
    if any(c < -2**31 or c >= 2**31 for c in ch):
        raise ValueError("channels must be int32 row indices")
    src = ctypes.create_string_buffer(bytes(blob), len(blob))
    # the entry reads the blob's C entries (C <= R <= 64 once it reads any): -1, refused, past the list's end
    arr = (ctypes.c_int32 * max(len(ch), 64))(*ch, *([-1] * (64 - len(ch))))
    n = ctypes.c_size_t(0)
    rc = load().net_blob_widen(src, len(blob), R, arr, None, 0, ctypes.byref(n))
    C = int.from_bytes(bytes(blob)[12:16], "little")
    if rc != NET_ERR_BLOB and len(ch) != C:  # (a blob the parser took has its C there)
        raise ValueError(f"channels must list the blob's {C} channels, got {len(ch)}")
    _check(rc, "net_blob_widen")
    out = ctypes.create_string_buffer(max(n.value, 1))
    _check(load().net_blob_widen(src, len(blob), R, arr, out, n.value, ctypes.byref(n)), "net_blob_widen")
    return out.raw[:n.value]


def params_dims() -> dict:
    arr = (ctypes.c_int32 * 7)()
    rc = load().net_params_dims(arr)
    if rc == NET_ERR_NO_PARAMS:
        return {}
    _check(rc, "net_params_dims")
    return dict(zip(("C", "T", "F1", "F2", "N", "weight_bits", "loaded"), list(arr)))


def params_unload() -> None:
    global _loaded
    load().net_params_unload()
    _loaded = None


def trial_stride() -> int:
    return int(load().net_trial_stride())


def _dims():
    if _loaded is None:
        raise NetError(NET_ERR_NO_PARAMS, "no parameters loaded")
    return _loaded.dims


class _Handle:
    """A handle of the library's with ``close()``, usable as a context manager.  A subclass names its
    destroy entry (``_destroy``) and what ``handle`` says once it is closed (``_closed``).  ``_h`` is
    None until the create entry has returned, so ``__del__`` after a failed constructor is harmless."""

    _h = _destroy = _closed = None

    @property
    def handle(self) -> int:
        if self._h is None:
            raise ValueError(self._closed)
        return self._h

    def close(self) -> None:
        if self._h is not None:
            getattr(load(), self._destroy)(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:  # pragma: no cover - interpreter shutdown
            pass


class Bank(_Handle):
    """net_bank_create: many parameter sets of one geometry resident side by side, for
    forward_epochs_bank_torch and forward_bank_torch.  ``param_sets`` holds ParamSets or blobs,
    ``scales`` nothing or one input-quantiser scale per set (needed for float32 input).  Independent
    of the loaded set.  A set the library refuses raises NetError with its index in ``.failed``.
    ``close()`` (or leaving the ``with`` block) frees the bank and its device copies after
    synchronising the devices that hold one; no call on the bank may be in flight then."""

    _destroy, _closed = "net_bank_destroy", "the bank is closed"

    def __init__(self, param_sets, scales=None):
        blobs = [p.to_blob() if isinstance(p, ParamSet) else bytes(p) for p in param_sets]
        n = len(blobs)
        if scales is not None and len(scales) != n:
            raise ValueError(f"{len(scales)} scales for {n} parameter sets")
        bufs = [ctypes.create_string_buffer(b, len(b)) for b in blobs]
        ptrs = (ctypes.c_void_p * max(n, 1))(*[ctypes.addressof(b) for b in bufs])
        sizes = (ctypes.c_size_t * max(n, 1))(*[len(b) for b in blobs])
        sc = None if scales is None else (ctypes.c_float * max(n, 1))(*[float(v) for v in scales])
        h, failed = ctypes.c_void_p(), ctypes.c_size_t(0)
        rc = load().net_bank_create(ptrs, sizes, sc, n, ctypes.byref(h), ctypes.byref(failed))
        if rc != NET_OK:
            err = NetError(rc, f"net_bank_create, set {failed.value}" if n else "net_bank_create")
            err.failed = failed.value
            raise err
        self._h = h.value
        info = self.info()
        self.n_sets, self.exact_division, self.has_scales = info[0], bool(info[4]), bool(info[5])
        self.dims = ParamSet.from_blob(blobs[0]).dims

    def info(self) -> list:
        """net_bank_info: [n_sets, C, T, N, exact_division, has_scales, bytes per set]."""
        arr = (ctypes.c_int32 * 7)()
        _check(load().net_bank_info(self.handle, arr), "net_bank_info")
        return list(arr)

    def image(self, s: int) -> bytes:
        """Test hook (mibminet_test_bank_copy): the parameter image of set ``s`` as the devices get it."""
        n = ctypes.c_size_t(0)
        _check(load().mibminet_test_bank_copy(self.handle, s, None, 0, ctypes.byref(n)), "mibminet_test_bank_copy")
        buf = ctypes.create_string_buffer(n.value)
        _check(load().mibminet_test_bank_copy(self.handle, s, buf, n.value, ctypes.byref(n)), "mibminet_test_bank_copy")
        return buf.raw

    def device_copies(self) -> int:
        """Test hook (mibminet_test_bank_device_copies): devices that hold a copy of the bank."""
        return int(load().mibminet_test_bank_device_copies(self.handle))

    def feature_bytes(self) -> int:
        """net_bank_feature_bytes: bytes of one item's layer-4 feature row, 16 * (T // 64)."""
        return int(load().net_bank_feature_bytes(self.handle))

    def replace(self, s: int, param_set_or_blob, scale: Optional[float] = None, device: int = 0, stream=None) -> None:
        """net_bank_replace: set ``s`` becomes ``param_set_or_blob`` (a ParamSet or a blob), ordered on
        ``stream`` (a torch stream; default: the current one of ``device``): the calls enqueued on it
        before read the old set, those after it the new one, and every other set stays as it is.
        The new set must agree with what the bank was created with (C, T, N, REORDER_BN, clip); a
        bank that runs the float form refuses a set that needs exact division.  ``scale`` is the
        set's input-quantiser scale, required iff the bank has scales.  Only ``device``'s copy of the
        bank is updated (a bank resident on another device is refused); before any device holds a
        copy only the host master changes and no stream is needed.  A refused call raises NetError
        and changes nothing.  Sessions of a stream group under set ``s`` need a restart afterwards
        unless the new set shares the old one's layer 1 (ParamSet.with_head)."""
        blob = param_set_or_blob.to_blob() if isinstance(param_set_or_blob, ParamSet) else bytes(param_set_or_blob)
        if self.has_scales and scale is None:
            raise ValueError("the bank has scales: the new set needs one")
        st = stream.cuda_stream if stream is not None else None
        if stream is None and self.device_copies():
            st = _torch().cuda.current_stream(device).cuda_stream
        buf = ctypes.create_string_buffer(blob, len(blob))
        _check(load().net_bank_replace(self.handle, s, buf, len(blob), 0.0 if scale is None else float(scale), device, st),
               f"net_bank_replace, set {s}")


def image_copy(which: int) -> bytes:
    """Test hook (mibminet_test_image_copy): image ``which`` of the loaded set (0 the batched
    kernels', 1 the window and epoch kernels')."""
    n = ctypes.c_size_t(0)
    _check(load().mibminet_test_image_copy(which, None, 0, ctypes.byref(n)), "mibminet_test_image_copy")
    buf = ctypes.create_string_buffer(n.value)
    _check(load().mibminet_test_image_copy(which, buf, n.value, ctypes.byref(n)), "mibminet_test_image_copy")
    return buf.raw


# ---- reference single-trial API (host arrays, reference layouts) --------------------------------
def _call_void(name: str, *arrays: np.ndarray) -> np.ndarray:
    """A void entry on host arrays, its status read from net_last_error; returns the last array."""
    L = load()
    getattr(L, name)(*(a.ctypes.data for a in arrays))
    _check(L.net_last_error(), name)
    return arrays[-1]


def net_model_compute(x_tc_align: np.ndarray) -> np.ndarray:
    """model.h:40 — x: [T][C_ALIGN] int8 -> logits [N] int8."""
    d = _dims()
    x = np.ascontiguousarray(x_tc_align, np.int8).reshape(d.T, d.C_ALIGN)
    return _call_void("net_model_compute", x, np.empty(d.N, np.int8))


def net_layer1(x_tc_align: np.ndarray) -> np.ndarray:
    d = _dims()
    x = np.ascontiguousarray(x_tc_align, np.int8).reshape(d.T, d.C_ALIGN)
    return _call_void("net_layer1", x, np.empty((d.F1, d.T_ALIGN), np.int8))


def net_layer2(y1: np.ndarray) -> np.ndarray:
    d = _dims()
    x = np.ascontiguousarray(y1, np.int8).reshape(d.F1, d.T_ALIGN)
    return _call_void("net_layer2", x, np.empty((d.F2, d.T8_ALIGN), np.int8))


def net_layer3(y2: np.ndarray) -> np.ndarray:
    d = _dims()
    x = np.ascontiguousarray(y2, np.int8).reshape(d.F2, d.T8_ALIGN)
    return _call_void("net_layer3", x, np.empty((d.F2, d.T8_ALIGN), np.int8))


def net_layer3_flip_inplace(y3: np.ndarray) -> np.ndarray:
    """layers.h:107 — [F2][T8_ALIGN] -> [T8][F2] (in place on a copy; returned)."""
    d = _dims()
    buf = np.ascontiguousarray(y3, np.int8).reshape(d.F2 * d.T8_ALIGN).copy()
    return _call_void("net_layer3_flip_inplace", buf)


def net_layer4(y3t: np.ndarray) -> np.ndarray:
    d = _dims()
    x = np.zeros(d.F2 * d.T8_ALIGN, np.int8)
    src = np.ascontiguousarray(y3t, np.int8).ravel()
    x[: min(src.size, x.size)] = src[: x.size]
    return _call_void("net_layer4", x, np.empty((d.F2, d.T64_ALIGN), np.int8))


def net_layer5(y4: np.ndarray) -> np.ndarray:
    d = _dims()
    x = np.ascontiguousarray(y4, np.int8).reshape(d.F2, d.T64_ALIGN)
    return _call_void("net_layer5", x, np.empty(d.N, np.int8))


def set_device(device: int) -> None:
    _check(load().net_set_device(device), "net_set_device")


# ---- batched device API -----------------------------------------------------------------------
def model_compute_batch(x_ptr: int, y_ptr: int, B: int, device: int = 0, stream: Optional[int] = None) -> None:
    """net_model_compute_batch(_async): x_ptr/y_ptr are device pointers ([B][trial_stride] int8
    and [B][N] int8).  With ``stream`` the launch is enqueued without a host sync."""
    L = load()
    if stream is None:
        _check(L.net_model_compute_batch(x_ptr, y_ptr, B, device), "net_model_compute_batch")
    else:
        _check(L.net_model_compute_batch_async(x_ptr, y_ptr, B, device, stream), "net_model_compute_batch_async")


def model_compute_batch_ct_sync(x_ptr: int, y_ptr: int, B: int, device: int = 0) -> None:
    """net_model_compute_batch_ct_sync (SURVEY §8(b)'s signature): channel-major [B][C][T] int8
    trials and [B][N] logits, device pointers; waits for completion."""
    _check(load().net_model_compute_batch_ct_sync(x_ptr, y_ptr, B, device), "net_model_compute_batch_ct_sync")


def params_info() -> dict:
    """net_params_info: which kernels the loaded set runs ("float", "exact" or "general"), and for
    "exact" the first layer / filter whose requant has no proven float form."""
    arr = (ctypes.c_int32 * 5)()
    _check(load().net_params_info(arr), "net_params_info")
    path = {NET_PATH_FLOAT: "float", NET_PATH_EXACT: "exact", NET_PATH_GENERAL: "general"}[arr[0]]
    return {"path": path, "layer": arr[1], "filter": arr[2], "shape": arr[3], "exact_division": bool(arr[4])}


def force_general(on: bool) -> None:
    """Test hook (mibminet_test_force_general): later loads run the run-time-dimension kernels
    even for the compiled geometries."""
    _check(load().mibminet_test_force_general(1 if on else 0), "mibminet_test_force_general")


def grid_cap(workgroups: int) -> None:
    """Test hook (mibminet_test_grid_cap): later persistent grids have at most ``workgroups``
    workgroups, so a few items walk a workgroup through its later passes; 0 restores the normal choice."""
    _check(load().mibminet_test_grid_cap(int(workgroups)), "mibminet_test_grid_cap")


def folded_filters() -> int:
    """Test hook (mibminet_test_folded_filters): constant filters the loaded set had folded."""
    v = ctypes.c_int32(0)
    _check(load().mibminet_test_folded_filters(ctypes.byref(v)), "mibminet_test_folded_filters")
    return v.value


def params_exact_division() -> bool:
    """True when the loaded set runs the exact integer-division kernels (Cfg::XR: a set outside the
    float requant envelope), False for the float-requant kernels."""
    rc = load().mibminet_test_params_xr()
    if rc < 0:
        raise NetError(rc, "mibminet_test_params_xr")
    return bool(rc)


def xdiv_host(e: np.ndarray, d: int) -> np.ndarray:
    """The exact-division kernels' integer division emulated on the host (mibminet_test_xdiv_host)."""
    e = np.ascontiguousarray(e, dtype=np.int32)
    q = np.empty_like(e)
    _check(load().mibminet_test_xdiv_host(e.ctypes.data, e.size, int(d), q.ctypes.data), "mibminet_test_xdiv_host")
    return q


def xdiv_gpu_mismatches(d: int, e0: int, count: int, device: int = 0) -> int:
    """The device xdiv over e0 .. e0 + count - 1 against C division (mibminet_test_xdiv_gpu)."""
    n = ctypes.c_int64(0)
    _check(load().mibminet_test_xdiv_gpu(int(d), int(e0), int(count), ctypes.byref(n), device), "mibminet_test_xdiv_gpu")
    return int(n.value)


def image_digest() -> int:
    """Test hook (mibminet_test_image_digest): FNV-1a digest of the loaded set's device parameter image."""
    v = ctypes.c_uint64(0)
    _check(load().mibminet_test_image_digest(ctypes.byref(v)), "mibminet_test_image_digest")
    return v.value


def upload_stats() -> tuple:
    """Test hook (mibminet_test_upload_stats): (parameter-image uploads so far, how many of them
    happened while the multi-device entries were enqueueing shards)."""
    a, b = ctypes.c_int64(0), ctypes.c_int64(0)
    _check(load().mibminet_test_upload_stats(ctypes.byref(a), ctypes.byref(b)), "mibminet_test_upload_stats")
    return a.value, b.value


def device_images(device: int = 0) -> int:
    """Test hook (mibminet_test_device_images): parameter-image copies resident on ``device``."""
    n = load().mibminet_test_device_images(device)
    if n < 0:
        raise NetError(n, "mibminet_test_device_images")
    return n


def quantize_f32_flat(x_ptr: int, q_ptr: int, n: int, scale: float, device: int = 0, stream: Optional[int] = None) -> None:
    """Test hook (mibminet_test_quantize_f32): the fused float entries' in-kernel quantiser on a flat
    device array, q[i] = quantize(x[i]) for i < n (x_ptr float32, q_ptr int8), enqueued on ``stream``."""
    _check(load().mibminet_test_quantize_f32(x_ptr, q_ptr, n, scale, device, stream), "mibminet_test_quantize_f32")


def pool_consts(off: int, layer: int) -> tuple:
    """Test hook (mibminet_test_pool_consts): (threshold, offset term) of the REORDER_BN pooling of
    ``layer`` (2 or 4) for offset ``off``, as the kernels use them."""
    thr, offm = ctypes.c_int32(0), ctypes.c_int32(0)
    _check(load().mibminet_test_pool_consts(off, layer, ctypes.byref(thr), ctypes.byref(offm)), "mibminet_test_pool_consts")
    return thr.value, offm.value


def launch_info(B: int, device: int = 0, channel_major: bool = False) -> dict:
    arr = (ctypes.c_int32 * 3)()
    fn = load().net_launch_info_ct if channel_major else load().net_launch_info
    _check(fn(B, device, arr), "net_launch_info")
    return {"grid": arr[0], "threads": arr[1], "lds_bytes": arr[2]}


# ---- the torch entries' shared steps ----------------------------------------------------------
def _torch():
    """torch, imported on first use: importing this module must work where torch is never imported."""
    import torch

    return torch


def _stream_on(device, stream):
    """The stream to launch on: ``stream``, or without one the current stream of ``device``."""
    return _torch().cuda.current_stream(device) if stream is None else stream


def _launch(x, stream):
    """(launch stream, device index) for the device tensor ``x`` and an optional ``stream``."""
    return _stream_on(x.device, stream), x.device.index or 0


def _logits(x, rows: int):
    """An uninitialised [rows][N] int8 logits tensor on ``x``'s device."""
    return _torch().empty((rows, _dims().N), dtype=_torch().int8, device=x.device)


def _check_tensor(x, noun: str, dtypes, dims=None, device: bool = True, contiguous: bool = True) -> str:
    """Raises ValueError unless ``x`` is a tensor of one of ``dtypes`` (names such as "int8"), on
    the device (``device=False``: anywhere, and a NumPy array passes too), contiguous unless
    ``contiguous`` is false and, given ``dims``, of that rank with every int entry matched (a str
    entry names a free dimension: ("B", 22, 1125)).  ``noun`` opens the message.  Returns the
    dtype's name.  The C ABI sees only pointers and counts, so another element type, orientation
    or stride would otherwise run and its bytes be read as something else."""
    dt = str(getattr(x, "dtype", "")).rpartition(".")[2]
    ok = dt in dtypes and (not device or getattr(x, "is_cuda", False))
    if ok and contiguous:
        ok = x.is_contiguous() if hasattr(x, "is_contiguous") else bool(x.flags["C_CONTIGUOUS"])
    if ok and dims is not None:
        shape = tuple(x.shape)
        ok = len(shape) == len(dims) and all(isinstance(d, str) or d == n for d, n in zip(dims, shape))
    if not ok:
        want = " ".join(w for w in ("contiguous" if contiguous else "", "/".join(dtypes), "device" if device else "",
                                    "tensor", "".join(f"[{d}]" for d in dims or ())) if w)
        got = f"{dt} {tuple(x.shape)}" if dt and hasattr(x, "shape") else type(x).__name__
        raise ValueError(f"{noun} must be a {want}, got {got}")
    return dt


def _layout_code(layout: str) -> int:
    """The C ABI's integer of a recording layout: "ct" ([C][L], channel-major) = 1, "tc" = 0."""
    if layout not in ("ct", "tc"):
        raise ValueError('layout must be "ct" ([C][L]) or "tc" ([L][C])')
    return 1 if layout == "ct" else 0


def _packed_stride(C: int, T: int) -> int:
    """Bytes per trial of the batched time-major layout: C*T rounded up to 16."""
    return (C * T + 15) // 16 * 16


def forward_torch(x, params: Optional[ParamSet] = None, stream=None):
    """Convenience: x is a CUDA/HIP int8 torch tensor [B][trial_stride] -> logits [B][N] tensor."""
    if params is not None:
        params_load(params)
    _dims()
    _check_tensor(x, "x", ("int8",))
    B = x.shape[0]
    if x.numel() != B * trial_stride():
        raise ValueError(f"x must be [B][{trial_stride()}]")
    y = _logits(x, B)
    s, dev = _launch(x, stream)
    model_compute_batch(x.data_ptr(), y.data_ptr(), B, dev, s.cuda_stream)
    return y


def forward_ct_torch(x, stream=None):
    """net_model_compute_batch_ct: x is a CUDA/HIP int8 tensor [B][C][T] (channel-major, the
    reference's input.npz layout; any byte alignment) -> logits [B][N] tensor, with no separate
    transpose pass."""
    d = _dims()
    _check_tensor(x, "x", ("int8",), ("B", d.C, d.T))
    y = _logits(x, x.shape[0])
    s, dev = _launch(x, stream)
    _check(load().net_model_compute_batch_ct(x.data_ptr(), y.data_ptr(), x.shape[0], dev, s.cuda_stream),
           "net_model_compute_batch_ct")
    return y


def forward_f32_torch(x, scale: float, stream=None):
    """net_model_compute_batch_f32: x is a CUDA/HIP float32 tensor [B][C][T] (float EEG, the
    reference's input.npz layout) -> logits [B][N], quantised inside the fused kernel."""
    d = _dims()
    _check_tensor(x, "x", ("float32",), ("B", d.C, d.T))
    y = _logits(x, x.shape[0])
    s, dev = _launch(x, stream)
    _check(load().net_model_compute_batch_f32(x.data_ptr(), y.data_ptr(), x.shape[0], scale, dev, s.cuda_stream),
           "net_model_compute_batch_f32")
    return y


def windows_count(L: int, hop: int) -> int:
    """net_windows_count: windows of the loaded network's T samples at hop ``hop`` in L samples."""
    return int(load().net_windows_count(L, hop))


def windows_row_stride(L: int) -> int:
    """net_windows_row_stride: bytes between the rows of the layer-1 workspace of L samples."""
    return int(load().net_windows_row_stride(L))


def windows_workspace(L: int) -> int:
    """net_windows_workspace: bytes of the layer-1 workspace ([16][row_stride] int8) of L samples."""
    return int(load().net_windows_workspace(L))


def _check_recording(x, dtypes, channels_first: bool, C: int, noun: str = "the recording"):
    """_check_tensor for a recording of C channels ([C][L] or [L][C]) of one of ``dtypes``; returns
    (L, whether it is float32)."""
    dt = _check_tensor(x, noun, dtypes, (C, "L") if channels_first else ("L", C))
    return int(x.shape[1 if channels_first else 0]), dt == "float32"


def _workspace(x, L: int):
    """An uninitialised layer-1 workspace [16][row_stride] of L samples on ``x``'s device."""
    return _torch().empty((16, windows_row_stride(L)), dtype=_torch().int8, device=x.device)


def _windows_buffers(x, L: int, hop: int):
    if hop < 1:
        raise ValueError("hop must be at least 1")
    return _logits(x, windows_count(L, hop)), _workspace(x, L)


def forward_windows_torch(x, hop: int, layout: str = "ct", stream=None, return_y1: bool = False):
    """net_model_compute_windows: x is a CUDA/HIP int8 recording, ``layout`` "ct" = [C][L]
    (channel-major) or "tc" = [L][C] (time-major), any byte alignment.  Returns the logits [W][N]
    of the windows x[:, w*hop : w*hop + T], W = windows_count(L, hop), each row what
    forward_ct_torch returns for that window; with ``return_y1`` also the workspace
    [16][row_stride] int8, whose row f holds layer 1's filter f over the whole recording."""
    code = _layout_code(layout)
    L, _ = _check_recording(x, ("int8",), layout == "ct", _dims().C)
    y, ws = _windows_buffers(x, L, hop)
    s, dev = _launch(x, stream)
    _check(load().net_model_compute_windows(x.data_ptr(), code, L, hop, y.data_ptr(), ws.data_ptr(), ws.numel(), dev,
                                            s.cuda_stream), "net_model_compute_windows")
    return (y, ws) if return_y1 else y


def forward_windows_f32_torch(x, hop: int, scale: float, stream=None, layout: str = "ct", return_y1: bool = False):
    """net_model_compute_windows_f32 / _f32_tm: x is a CUDA/HIP float32 recording, ``layout`` "ct" =
    [C][L] or "tc" = [L][C] (sample-major frames), quantised per sample as forward_f32_torch does;
    returns the logits [W][N] of its sliding windows, with ``return_y1`` also the workspace."""
    _layout_code(layout)
    L, _ = _check_recording(x, ("float32",), layout == "ct", _dims().C)
    y, ws = _windows_buffers(x, L, hop)
    s, dev = _launch(x, stream)
    name = "net_model_compute_windows_f32" + ("" if layout == "ct" else "_tm")
    _check(getattr(load(), name)(x.data_ptr(), L, hop, scale, y.data_ptr(), ws.data_ptr(), ws.numel(), dev, s.cuda_stream),
           name)
    return (y, ws) if return_y1 else y


def _require_bank(bank):
    if not isinstance(bank, Bank):
        raise ValueError(f"bank must be a Bank, got {type(bank).__name__}")
    return bank


class _Net:
    """The network a forward entry runs, the loaded set or ``bank``: its dims, the handle that leads the
    C call's arguments, and a float32 input's scale: an argument for the loaded set, a bank has its own."""

    def __init__(self, bank=None):
        self.bank, self.handle, self.scale = bank, () if bank is None else (bank.handle,), ()
        self.f32_suffix = "_f32"  # "_f32_tm": float32 input in sample-major frames (_windows_source)

    dims = property(lambda self: _dims() if self.bank is None else self.bank.dims)

    def float_input(self, f32: bool, scale, noun: str) -> None:
        if self.bank is not None and f32 and not self.bank.has_scales:
            raise ValueError("a float32 source needs a bank created with scales")
        if self.bank is None and f32 != (scale is not None):
            raise ValueError(f"scale is required for a float32 {noun} and not accepted for an int8 one")
        self.scale = () if scale is None else (scale,)


def _index_list(v, dtype, what: str):
    """A 1-D tensor of ``dtype`` from one (checked) or from a sequence of ints."""
    torch = _torch()
    if not isinstance(v, torch.Tensor):
        return torch.as_tensor([int(o) for o in v], dtype=dtype).reshape(-1)
    if v.dtype != dtype or v.dim() != 1:
        raise ValueError(f"{what} must be a 1-D {str(dtype).rpartition('.')[2]} tensor or a sequence of ints")
    return v


def _forward_onsets(net, name: str, x, head, onsets, mid, stream, check: bool, noun: str, set_of=False,
                    features: bool = False):
    """The call of an entry of ``net`` (a _Net) that takes an onset list, ``name`` or, for a float32
    ``x``, ``name``_f32: entry([bank,] x, *head, onsets, [set_of,] n, [scale,] y, n_bad, *mid, device,
    stream).  ``onsets`` is a 1-D int64 tensor or a sequence of ints; ``set_of`` False (the entry takes
    no set index per item), as many indices (a 1-D int32 tensor or a sequence), or None (NULL: set 0
    for every item, a bank of one set only).  The lists' device copies and, with ``check``, the zeroed
    counter are made on the launch stream.  An empty list passes NULL for the lists and the logits,
    ``check=False`` NULL for the counter.  With ``check`` and a non-empty list the stream is
    synchronised, the count of items outside the ``noun`` read back and a ValueError raised if it is
    not zero.  Returns the logits [n][N]; with ``features`` the entry is ``name``_feat[_f32], which takes
    a feature buffer after the logits, and (logits, features [n][16][T64] int8) is returned."""
    torch = _torch()
    lists = [_index_list(onsets, torch.int64, "onsets")]
    n = int(lists[0].numel())
    if set_of is None:
        if net.bank.n_sets != 1:
            raise ValueError(f"set_of may be None only for a bank of one set, this one has {net.bank.n_sets}")
    elif set_of is not False:
        lists.append(_index_list(set_of, torch.int32, "set_of"))
        if int(lists[1].numel()) != n:
            raise ValueError(f"{int(lists[1].numel())} set indices for {n} onsets")
    s, dev = _launch(x, stream)
    with torch.cuda.stream(s):  # the lists' copies and the counter's zeroing precede the launch on its stream
        lists = [v.to(x.device).contiguous() for v in lists]
        nbad = torch.zeros((1,), dtype=torch.int32, device=x.device) if check else None
    y = torch.empty((n, net.dims.N), dtype=torch.int8, device=x.device)
    feat = torch.empty((n, net.dims.F2, net.dims.T64), dtype=torch.int8, device=x.device) if features else None
    name += ("_feat" if features else "") + (net.f32_suffix if x.dtype == torch.float32 else "")
    ptrs = [v.data_ptr() if n else None for v in lists] + [None] * (set_of is None)
    y_ptr, nbad_ptr = y.data_ptr() if n else None, nbad.data_ptr() if check else None
    feat_ptr = ((feat.data_ptr() if n else None),) if features else ()
    _check(getattr(load(), name)(*net.handle, x.data_ptr(), *head, *ptrs, n, *net.scale, y_ptr, *feat_ptr, nbad_ptr, *mid,
                                 dev, s.cuda_stream), name)
    if check and n:
        s.synchronize()
        bad = int(nbad.item())
        if bad:
            what = "onsets" if set_of is False else "onsets or set indices"
            raise ValueError(f"{bad} of {n} {what} lie outside the {noun} (their logit rows are zero)")
    return (y, feat) if features else y


def _windows_source(net, x, layout: str, scale, noun: str):
    """The checks of the array ``x`` (``noun``) the windows-at entries of ``net`` read: int8 ("ct" =
    [C][L] or "tc" = [L][C]) or float32 (the same two: the _f32 entry or the _f32_tm one).  Returns (L,
    the arguments that follow x)."""
    code = _layout_code(layout)
    L, f32 = _check_recording(x, ("int8", "float32"), layout == "ct", net.dims.C, noun)
    net.float_input(f32, scale, "recording")
    net.f32_suffix = "_f32" if layout == "ct" else "_f32_tm"
    return L, ((L,) if f32 else (code, L))


def forward_windows_at_torch(x, onsets, layout: str = "ct", scale: Optional[float] = None, stream=None,
                             check: bool = True, return_y1: bool = False):
    """net_model_compute_windows_at / _f32: the windows x[:, onsets[i] : onsets[i] + T] of one
    CUDA/HIP recording, layer 1 run once over the whole of it.  ``x`` is int8 ("ct" = [C][L] or
    "tc" = [L][C]) or float32 (either layout; ``scale`` is required iff it is float32), ``onsets`` an int64
    tensor or a sequence, in any order, duplicates allowed.  Returns the logits [W][N] int8, row i
    what forward_ct_torch returns for that window; with ``return_y1`` also the workspace
    [16][row_stride].  The rows of onsets outside 0 .. L - T are zero; with ``check`` their count
    is read back (a host sync) and a ValueError names it."""
    net = _Net()
    L, lead = _windows_source(net, x, layout, scale, "the recording")
    ws = _workspace(x, L)
    y = _forward_onsets(net, "net_model_compute_windows_at", x, lead, onsets, (ws.data_ptr(), ws.numel()), stream, check,
                        "recording")
    return (y, ws) if return_y1 else y


def windows_multi_onsets(lengths, hop: int):
    """net_windows_multi_onsets: the sliding-window onsets of recordings of ``lengths`` samples laid
    end to end along time, no window crossing a boundary.  Returns (onsets as a NumPy int64 array,
    first as a list of R + 1 ints: first[r] = the index of recording r's first window, first[R] =
    the number of windows)."""
    lens = [int(v) for v in lengths]
    if hop < 1 or any(v < 0 for v in lens) or sum(lens) >= 2**63:
        raise ValueError("hop must be at least 1, the lengths non-negative and their sum below 2^63")
    _dims()
    R = len(lens)
    arr = (ctypes.c_size_t * max(R, 1))(*lens)
    first = (ctypes.c_size_t * (R + 1))()
    W = int(load().net_windows_multi_count(arr, R, hop))
    onsets = np.empty(W, np.int64)
    load().net_windows_multi_onsets(arr, R, hop, onsets.ctypes.data if W else None, W, first)
    return onsets, [int(v) for v in first]


def _plan_chunks(lengths, bytes_per_sample: int, max_bytes: int):
    """Whole recordings, in order, greedily into chunks whose total length times
    ``bytes_per_sample`` stays below ``max_bytes``.  Returns the chunks as (first recording, one
    past the last) pairs; a single recording at or over the limit raises ValueError."""
    lengths = [int(v) for v in lengths]
    chunks, start, total = [], 0, 0
    for r, n in enumerate(lengths):
        if n * bytes_per_sample >= max_bytes:
            raise ValueError(f"recording {r} ({n} samples of {bytes_per_sample} bytes) reaches the limit of {max_bytes}"
                             " bytes per call: feed it in chunks that overlap by T - hop samples (INTEGRATION.md,"
                             ' "Continuous recordings")')
        if (total + n) * bytes_per_sample >= max_bytes:
            chunks.append((start, r))
            start, total = r, 0
        total += n
    if start < len(lengths):
        chunks.append((start, len(lengths)))
    return chunks


def _check_recordings(net, tensors, layout: str, hop: int):
    """Layout, hop and the list of recordings of a sliding-windows call on ``net``, all on one device
    and of one element type.  Returns (the time axis, their lengths, whether they are float32)."""
    _layout_code(layout)
    if hop < 1:
        raise ValueError("hop must be at least 1")
    C = net.dims.C
    if not tensors:
        raise ValueError("recordings must hold at least one tensor")
    for t in tensors:
        _, f32 = _check_recording(t, ("int8", "float32"), layout == "ct", C)
        if t.device != tensors[0].device or t.dtype != tensors[0].dtype:
            raise ValueError("the recordings must be on one device and of one element type")
    axis = 1 if layout == "ct" else 0
    return axis, [int(t.shape[axis]) for t in tensors], f32


def _stitch(net, x, out):
    """The chunks' logits [W_k][N] as one tensor on ``x``'s device (no chunk: no rows)."""
    if not out:
        return _torch().empty((0, net.dims.N), dtype=_torch().int8, device=x.device)
    return out[0] if len(out) == 1 else _torch().cat(out, dim=0)


def forward_windows_multi_torch(recordings, hop: int, layout: str = "ct", scale: Optional[float] = None, stream=None,
                                max_bytes: Optional[int] = None):
    """The sliding windows (hop ``hop``) of many recordings in one call per chunk, no window
    crossing a recording boundary.  ``recordings`` is a list of CUDA/HIP tensors ([C][L_r] each, or
    [L_r][C] for "tc"; int8, or float32 with ``scale``), or a pair (x, lengths) of one concatenated
    tensor and its recordings' lengths.  Returns (logits [W][N] int8, first): rows first[r] ..
    first[r + 1] - 1 are what forward_windows_torch returns for recording r.  Whole recordings are
    grouped into chunks whose samples times max(16, C * element size) stay below ``max_bytes``
    (default: the entries' 2^31 limit), each chunk one forward_windows_at_torch call; no host sync."""
    torch = _torch()
    net = _Net()
    pair = (isinstance(recordings, (tuple, list)) and len(recordings) == 2 and hasattr(recordings[0], "is_cuda")
            and not hasattr(recordings[1], "is_cuda"))
    tensors = [recordings[0]] if pair else list(recordings)
    axis, lengths, f32 = _check_recordings(net, tensors, layout, hop)
    if pair:
        x, n, lengths = tensors[0], lengths[0], [int(v) for v in recordings[1]]
        if min(lengths, default=0) < 0 or sum(lengths) != n:
            raise ValueError(f"the lengths must be non-negative and sum to the tensor's {n} samples")
    net.float_input(f32, scale, "recording")
    per = max(16, net.dims.C * (4 if f32 else 1))
    chunks = _plan_chunks(lengths, per, 2**31 if max_bytes is None else int(max_bytes))
    s, _ = _launch(tensors[0], stream)
    starts = np.concatenate(([0], np.cumsum(lengths))).tolist()
    out, first = [], [0]
    with torch.cuda.stream(s):  # the chunks' copies precede their launches on the stream
        for a, b in chunks:
            onsets, f = windows_multi_onsets(lengths[a:b], hop)
            first += [first[a] + v for v in f[1:]]
            if pair:
                xc = x if (a, b) == (0, len(lengths)) else x.narrow(axis, starts[a], starts[b] - starts[a]).contiguous()
            else:
                xc = tensors[a] if b == a + 1 else torch.cat(tensors[a:b], dim=axis)
            # every generated onset is valid: no counter, no host sync
            out.append(forward_windows_at_torch(xc, torch.from_numpy(onsets), layout=layout, scale=scale, stream=s,
                                                check=False))
        return _stitch(net, tensors[0], out), first


def _channel_table(channels, C: int):
    """The ctypes int32[C] host table of ``channels`` (None: NULL, rows 0 .. C-1)."""
    if channels is None:
        return None
    ch = [int(c) for c in (channels.tolist() if hasattr(channels, "tolist") else channels)]
    if len(ch) != C:
        raise ValueError(f"channels must list the network's {C} channels, got {len(ch)}")
    if min(ch) < 0 or max(ch) >= 2**31:
        raise ValueError("channels must be non-negative row indices")
    return (ctypes.c_int32 * C)(*ch)


def _epoch_source(net, x, channels, row_stride, scale):
    """The checks of the flat source ``x`` the epochs entries of ``net`` read, its ``row_stride``
    (None: x.shape[-1]) and ``channels``.  Returns the arguments that follow x."""
    C = net.dims.C
    f32 = _check_tensor(x, "x", ("int8", "float32")) == "float32"
    net.float_input(f32, scale, "source")
    if x.dim() < 1:
        raise ValueError("x must have at least one dimension")
    rs = int(x.shape[-1]) if row_stride is None else int(row_stride)
    if rs < 1:
        raise ValueError("row_stride must be at least 1")
    return x.numel(), rs, _channel_table(channels, C)


def forward_epochs_torch(x, onsets, channels=None, row_stride: Optional[int] = None, scale: Optional[float] = None,
                         stream=None, check: bool = True):
    """net_model_compute_epochs / _f32: epochs of the loaded network's C x T read straight out of a
    wider array.  ``x`` is any contiguous CUDA/HIP int8 or float32 tensor, used flat (``scale`` is
    required iff it is float32: the input quantiser's, as forward_f32_torch); epoch e, channel c,
    sample t is flat element ``onsets[e] + channels[c] * row_stride + t``.  ``row_stride`` defaults
    to ``x.shape[-1]``, ``channels`` (C row indices on the host) to 0 .. C-1, and ``onsets`` is an
    int64 tensor or a sequence.  Returns the logits [E][N] int8, row e what forward_ct_torch
    returns for the materialised epoch.  The rows of onsets outside the source are zero; with
    ``check`` their count is read back (a host sync) and a ValueError names it."""
    net = _Net()
    return _forward_onsets(net, "net_model_compute_epochs", x, _epoch_source(net, x, channels, row_stride, scale), onsets,
                           (), stream, check, "source")


def forward_crop_torch(x, t0: int, channels=None, scale: Optional[float] = None, stream=None):
    """Every trial of a batch ``x`` [B][R][Tf] (int8, or float32 with ``scale``) cropped to samples
    t0 .. t0 + T - 1 of the rows ``channels`` (C row indices < R; default 0 .. C-1), through
    forward_epochs_torch: row_stride = Tf, onsets[b] = b R Tf + t0, built on the device.  Returns
    the logits [B][N]."""
    torch = _torch()
    d = _dims()
    if not hasattr(x, "dim") or x.dim() != 3:
        raise ValueError("x must be a batch [B][R][Tf]")
    B, R, Tf = (int(v) for v in x.shape)
    if t0 < 0 or t0 + d.T > Tf:
        raise ValueError(f"the crop t0 = {t0}, T = {d.T} does not fit in Tf = {Tf}")
    ch = list(range(d.C)) if channels is None else [int(c) for c in channels]
    if len(ch) != d.C or min(ch) < 0 or max(ch) >= R:
        raise ValueError(f"channels must be {d.C} row indices below R = {R}")
    if not x.is_cuda:
        raise ValueError("x must be a device tensor")
    s, _ = _launch(x, stream)
    with torch.cuda.stream(s):
        onsets = torch.arange(B, dtype=torch.int64, device=x.device) * (R * Tf) + t0
    # every onset is in range by the checks above: no counter, no host sync
    return forward_epochs_torch(x, onsets, channels=ch, row_stride=Tf, scale=scale, stream=s, check=False)


def forward_epochs_bank_torch(bank, x, onsets, set_of, channels=None, row_stride: Optional[int] = None, stream=None,
                              check: bool = True, features: bool = False):
    """net_model_compute_epochs_bank / _f32: forward_epochs_torch with the network chosen per
    epoch: epoch e is classified by set ``set_of[e]`` of ``bank`` (a Bank; the loaded set plays no
    part).  ``x``, ``onsets``, ``channels`` and ``row_stride`` are forward_epochs_torch's, C and T
    the bank's; a float32 ``x`` needs a bank with scales and is quantised with the scale of each
    epoch's set.  ``set_of`` is an int32 tensor or a sequence, one index per onset (None: a bank of
    one set).  Returns the logits [E][N] int8, row e what forward_epochs_torch returns for that
    epoch with set ``set_of[e]`` loaded.  Any order is correct; grouped by set is fast.  The rows
    of invalid onsets and of indices outside the bank are zero; with ``check`` their count is read
    back (a host sync) and a ValueError names it.  With ``features``
    (net_model_compute_epochs_bank_feat / _f32) returns (logits, features [E][16][T // 64] int8): row e
    is layer 4's output of epoch e under its set, the bytes layer 5 multiplies, zeros for an invalid
    epoch; a head refitted on them goes back through ParamSet.with_head and Bank.replace."""
    net = _Net(_require_bank(bank))
    return _forward_onsets(net, "net_model_compute_epochs_bank", x, _epoch_source(net, x, channels, row_stride, None),
                           onsets, (), stream, check, "source or the bank", set_of=set_of, features=features)


def forward_bank_torch(bank, x, set_of, stream=None, check: bool = True):
    """A batch ``x`` [B][C][T] (int8, or float32 for a bank with scales), trial b classified by set
    ``set_of[b]`` of ``bank``, through forward_epochs_bank_torch as forward_crop_torch does it:
    row_stride = T, onsets[b] = b C T, built on the device.  Returns the logits [B][N]."""
    torch = _torch()
    d = _require_bank(bank).dims
    _check_tensor(x, "x", ("int8", "float32"), ("B", d.C, d.T))
    s, _ = _launch(x, stream)
    with torch.cuda.stream(s):
        onsets = torch.arange(x.shape[0], dtype=torch.int64, device=x.device) * (d.C * d.T)
    return forward_epochs_bank_torch(bank, x, onsets, set_of, row_stride=d.T, stream=s, check=check)


def bank_windows_lists(bank, lengths, sets, hop: int):
    """net_bank_windows_starts / net_bank_windows_lists: the layout and lists of the sliding windows
    (hop ``hop``) of recordings of ``lengths`` samples, recording r under set ``sets[r]`` of ``bank``,
    each starting at a multiple of 16 samples.  Returns (starts, L, blk_set, onsets, first): NumPy
    arrays int64[R], int32[ceil(L / 16)], int64[W] and int64[R + 1], and L as an int."""
    _require_bank(bank)
    lens, ss = [int(v) for v in lengths], [int(v) for v in sets]
    R = len(lens)
    if len(ss) != R:
        raise ValueError(f"{len(ss)} sets for {R} recordings")
    if R == 0 or hop < 1 or min(lens) < 0 or min(ss) < 0 or max(ss) >= bank.n_sets:
        raise ValueError(f"at least one recording, hop at least 1, non-negative lengths and sets in 0 .. {bank.n_sets - 1}")
    if sum(lens) + 16 * R >= 2**63:
        raise ValueError("the recordings must end below 2^63 samples")
    arr = (ctypes.c_size_t * R)(*lens)
    sarr = (ctypes.c_int32 * R)(*ss)
    starts = np.zeros(R, np.int64)
    L = int(load().net_bank_windows_starts(arr, R, starts.ctypes.data))
    nb = (L + 15) // 16
    first = (ctypes.c_size_t * (R + 1))()
    W = int(load().net_bank_windows_lists(bank.handle, arr, sarr, R, hop, None, 0, None, 0, None))
    blk_set, onsets = np.empty(nb, np.int32), np.empty(W, np.int64)
    load().net_bank_windows_lists(bank.handle, arr, sarr, R, hop, blk_set.ctypes.data if nb else None, nb,
                                  onsets.ctypes.data if W else None, W, first)
    return starts, L, blk_set, onsets, np.array(list(first), np.int64)


def forward_windows_bank_torch(bank, x, blk_set, onsets, layout: str = "ct", stream=None, check: bool = True,
                               return_y1: bool = False):
    """net_model_compute_windows_bank / _f32: the windows x[:, onsets[i] : onsets[i] + T] of many
    recordings laid along time in ``x`` at multiples of 16 samples, each classified by the set of
    its recording.  ``x`` is int8 ("ct" = [C][L] or "tc" = [L][C]) or float32 (either layout; needs a
    bank with scales), C and T the bank's; ``blk_set`` a device int32 tensor of ceil(L / 16) entries, the
    set of each 16-sample block (-1: a gap); ``onsets`` an int64 tensor or a sequence
    (bank_windows_lists builds both).  Returns the logits [W][N] int8, row i what forward_ct_torch
    returns for that window with its set loaded; with ``return_y1`` also the workspace
    [16][row_stride].  A window is invalid when its onset lies outside 0 .. L - T, its first block's
    set lies outside the bank or its last block has another entry; such rows are zero, and with
    ``check`` their count is read back (a host sync) and a ValueError names it."""
    net = _Net(_require_bank(bank))
    L, lead = _windows_source(net, x, layout, None, "the recordings' array")
    _check_tensor(blk_set, "blk_set", ("int32",), ((L + 15) // 16,))
    if blk_set.device != x.device:
        raise ValueError("blk_set must be on the array's device")
    ws = _workspace(x, L)
    y = _forward_onsets(net, "net_model_compute_windows_bank", x, lead + (blk_set.data_ptr(),), onsets,
                        (ws.data_ptr(), ws.numel()), stream, check, "recording or the bank")
    return (y, ws) if return_y1 else y


def forward_windows_multi_bank_torch(bank, recordings, sets, hop: int, layout: str = "ct", stream=None,
                                     max_bytes: Optional[int] = None):
    """The sliding windows (hop ``hop``) of many recordings, recording r classified by set
    ``sets[r]`` of ``bank``, in one call per chunk.  ``recordings`` is a list of CUDA/HIP tensors
    ([C][L_r] each, or [L_r][C] for "tc"; int8, or float32 for a bank with scales).  Returns
    (logits [W][N] int8, first): rows first[r] .. first[r + 1] - 1 are what forward_windows_torch
    returns for recording r with set ``sets[r]`` loaded.  The tensors are laid at starts that are
    multiples of 16 samples, zero pads between them, and whole recordings are grouped into chunks
    whose samples times max(16, C * element size) stay below ``max_bytes`` (default: the entries'
    2^31 limit), each chunk one forward_windows_bank_torch call; no host sync."""
    torch = _torch()
    net = _Net(_require_bank(bank))
    d = bank.dims
    tensors, sets = list(recordings), [int(v) for v in sets]
    axis, lengths, f32 = _check_recordings(net, tensors, layout, hop)
    if len(sets) != len(tensors):
        raise ValueError(f"{len(sets)} sets for {len(tensors)} recordings")
    net.float_input(f32, None, "recording")
    # a chunk's pads add at most 15 samples per recording
    per = max(16, d.C * (4 if f32 else 1))
    chunks = _plan_chunks([n + 15 for n in lengths], per, 2**31 if max_bytes is None else int(max_bytes))
    s, _ = _launch(tensors[0], stream)
    out, first = [], [0]
    with torch.cuda.stream(s):  # the chunks' copies precede their launches on the stream
        for a, b in chunks:
            starts, L, blk_set, onsets, f = bank_windows_lists(bank, lengths[a:b], sets[a:b], hop)
            first += [first[a] + int(v) for v in f[1:]]
            parts = []
            for r in range(a, b):
                parts.append(tensors[r])
                pad = (int(starts[r - a + 1]) if r + 1 < b else L) - int(starts[r - a]) - lengths[r]
                if pad:
                    shape = (d.C, pad) if axis == 1 else (pad, d.C)
                    parts.append(torch.zeros(shape, dtype=tensors[r].dtype, device=tensors[r].device))
            xc = parts[0] if len(parts) == 1 else torch.cat(parts, dim=axis)
            # every generated window is valid: no counter, no host sync
            out.append(forward_windows_bank_torch(bank, xc, torch.from_numpy(blk_set).to(xc.device),
                                                  torch.from_numpy(onsets), layout=layout, stream=s, check=False))
        return _stitch(net, tensors[0], out), first


class _StreamGroup(_Handle):
    """What Streams and StreamsEach share: the constructor (``_create`` names the create entry), the
    entries that take either kind of group, and the checks of a push's ``x``.  The subclasses keep
    the docstrings that differ between the two kinds."""

    _destroy, _closed, _create = "net_streams_destroy", "the stream group is closed", None

    def __init__(self, bank, sets, hop: int, max_push: int, device: int = 0):
        self.bank = _require_bank(bank)
        ss = [0] * sets if isinstance(sets, int) else [int(v) for v in sets]
        if hop < 1 or max_push < 1 or not ss:
            raise ValueError("at least one session, hop and max_push at least 1")
        arr = (ctypes.c_int32 * len(ss))(*ss)
        h = ctypes.c_void_p()
        _check(getattr(load(), self._create)(bank.handle, arr, len(ss), hop, max_push, device, ctypes.byref(h)),
               self._create)
        self._h = h.value
        self.S, self.hop, self.max_push, self.device = len(ss), hop, max_push, device
        self.cap = self.info()[3]

    def info(self) -> list:
        """net_streams_info: six int64 values."""
        arr = (ctypes.c_int64 * 6)()
        _check(load().net_streams_info(self.handle, arr), "net_streams_info")
        return list(arr)

    def origin(self, i: int) -> tuple:
        """net_streams_origin: (origin, set) of session ``i``."""
        o, s = ctypes.c_int64(0), ctypes.c_int32(0)
        _check(load().net_streams_origin(self.handle, i, ctypes.byref(o), ctypes.byref(s)), "net_streams_origin")
        return o.value, s.value

    def restart(self, i: int, set: int, stream=None) -> None:
        """net_streams_restart of session ``i`` under ``set``."""
        _check(load().net_streams_restart(self.handle, i, set, _stream_on(self.device, stream).cuda_stream),
               "net_streams_restart")

    def windows_at(self, sessions, onsets, stream=None, out=None, check: bool = True, features: bool = False):
        """net_streams_windows_at: the windows of sessions ``sessions[w]`` that start at samples
        ``onsets[w]``, read from the layer-1 rings as they are.  The lists are device tensors (int32 and
        int64, 1-D) or sequences of ints, through _index_list; their device copies and the zeroed
        counter are made on the launch stream.  ``check`` is forward_windows_at_torch's: the stream is
        synchronised, the count of invalid items read back and a ValueError raised if it is not zero;
        ``check=False`` passes NULL for the counter.  Returns the logits [W][N]; with ``features``
        (net_streams_windows_at_feat) the pair (logits, features [W][16][T64] int8), a zero feature
        row beside every zero logit row."""
        torch = _torch()
        ses = _index_list(sessions, torch.int32, "sessions")
        ons = _index_list(onsets, torch.int64, "onsets")
        d = self.bank.dims
        W, N = int(ses.numel()), d.N
        if int(ons.numel()) != W:
            raise ValueError(f"{W} sessions for {int(ons.numel())} onsets")
        dev = torch.device("cuda", self.device)
        s = _stream_on(self.device, stream)
        with torch.cuda.stream(s):  # the lists' copies and the counter's zeroing precede the launch on its stream
            ses, ons = ses.to(dev).contiguous(), ons.to(dev).contiguous()
            nbad = torch.zeros((1,), dtype=torch.int32, device=dev) if check else None
            if out is None:
                out = torch.empty((W, N), dtype=torch.int8, device=dev)
            feat = torch.empty((W, d.F2, d.T64), dtype=torch.int8, device=dev) if features else None
        _check_tensor(out, "out", ("int8",), (W, N))
        lead = (self.handle, ses.data_ptr() if W else None, ons.data_ptr() if W else None, W, out.data_ptr() if W else None)
        tail = (nbad.data_ptr() if check else None, s.cuda_stream)
        if features:
            _check(load().net_streams_windows_at_feat(*lead, feat.data_ptr() if W else None, *tail),
                   "net_streams_windows_at_feat")
        else:
            _check(load().net_streams_windows_at(*lead, *tail), "net_streams_windows_at")
        if check and W:
            s.synchronize()
            bad = int(nbad.item())
            if bad:
                raise ValueError(f"{bad} of {W} windows are not in the rings (their logit rows are zero)")
        return (out, feat) if features else out

    _set_decimator = None  # the subclass's entry

    def decimate(self, q: int, taps, stream=None) -> None:
        """``_set_decimator`` (net_streams_set_decimator or _each) with the taps as float32[K]."""
        h = np.ascontiguousarray(taps, dtype=np.float32)
        if h.ndim != 1:
            raise ValueError("taps must be a 1-D array")
        s = _stream_on(self.device, stream)
        _check(getattr(load(), self._set_decimator)(self.handle, q, h.ctypes.data, h.size, s.cuda_stream),
               self._set_decimator)

    def raw_info(self) -> list:
        """net_streams_raw_info: four int64 values."""
        arr = (ctypes.c_int64 * 4)()
        _check(load().net_streams_raw_info(self.handle, arr), "net_streams_raw_info")
        return list(arr)

    def prefilter(self, sos, stream=None) -> np.ndarray:
        """net_streams_set_prefilter: once, after the decimator and before the first push.  ``sos`` is
        [M][5] = {b0, b1, b2, a1, a2} (a0 = 1) or scipy's [M][6] = {b0, b1, b2, a0, a1, a2}, which is
        divided by a0 in float64 and then rounded to float32.  From then on every raw frame passes the
        cascade, per session and electrode, ahead of the FIR, bit for bit as decimate.sos_filter
        states it.  Returns the float32 [M][5] that was handed over."""
        c = np.asarray(sos, dtype=np.float64)
        if c.ndim != 2 or c.shape[1] not in (5, 6):
            raise ValueError("sos must be an array [M][5] or [M][6]")
        if c.shape[1] == 6:
            c = np.concatenate([c[:, :3], c[:, 4:]], axis=1) / c[:, 3:4]
        c = np.ascontiguousarray(c, dtype=np.float32)
        s = _stream_on(self.device, stream)
        _check(load().net_streams_set_prefilter(self.handle, c.ctypes.data, c.shape[0], s.cuda_stream),
               "net_streams_set_prefilter")
        return c

    def prefilter_info(self) -> list:
        """net_streams_prefilter_info: [M (0: none), the scratch's frames per session, bytes allocated]."""
        arr = (ctypes.c_int64 * 3)()
        _check(load().net_streams_prefilter_info(self.handle, arr), "net_streams_prefilter_info")
        return list(arr)

    def _push_source(self, x, layout: str, f32: bool) -> tuple:
        """Checks a push's ``x``, int8 or (``f32``) float32, [S][C][n] or [S][n][C] by ``layout``.  Returns
        the entry's suffix ("", "_f32" or "_f32_tm"), the layout code as the entry takes it (the
        float32 entries take none) and n."""
        code = _layout_code(layout)
        if f32 and not self.bank.has_scales:
            raise ValueError("a float32 source needs a bank created with scales")
        C, ct = self.bank.dims.C, layout == "ct"
        _check_tensor(x, "x", ("float32",) if f32 else ("int8",), (self.S, C, "n") if ct else (self.S, "n", C))
        n = int(x.shape[2 if ct else 1])
        return ("_f32" if ct else "_f32_tm", (), n) if f32 else ("", (code,), n)


class Streams(_StreamGroup):
    """net_streams_create: ``len(sets)`` live sessions of ``bank``'s geometry on ``device``, session i
    decoded by set ``sets[i]`` (``sets`` an int: that many sessions under set 0), windows at every
    ``hop``-th sample of the global grid, at most ``max_push`` samples per session and push.  The group
    keeps a device-resident ring of layer-1 outputs per session; ``push`` runs layer 1 on the new
    samples only and returns the windows that end in them.  All pushes and restarts of a group must
    be ordered with respect to one another (one stream, or events).  The bank must outlive the group;
    ``close()`` (or leaving the ``with`` block) synchronises the device and frees it."""

    _create, _set_decimator = "net_streams_create", "net_streams_set_decimator"

    def info(self) -> list:
        """net_streams_info: [S, hop, max_push, cap, position, windows returned per session so far]."""
        return super().info()

    def windows(self, n: int) -> int:
        """net_streams_push_windows: the windows per session the next push of ``n`` samples returns."""
        return int(load().net_streams_push_windows(self.bank.handle, self.hop, self.info()[4], n))

    def _push(self, x, dtype: str, code, n: int, stream, out, k: Optional[int] = None):
        """``dtype``: the entry's suffix, "" (int8), "_f32", "_f32_tm" or "_raw_f32_tm"; ``k``: the windows
        per session, where they are not ``windows(n)``."""
        torch = _torch()
        k, N = self.windows(n) if k is None else k, self.bank.dims.N
        s, _ = _launch(x, stream)
        with torch.cuda.stream(s):  # the counter's zeroing precedes the launch on its stream
            nbad = torch.zeros((1,), dtype=torch.int32, device=x.device)
        if out is None:
            out = torch.empty((self.S, k, N), dtype=torch.int8, device=x.device)
        else:
            _check_tensor(out, "out", ("int8",), (self.S, k, N))
        name = "net_streams_push" + dtype
        _check(getattr(load(), name)(self.handle, x.data_ptr(), *code, n, out.data_ptr() if k else None, nbad.data_ptr(),
                                     s.cuda_stream), name)
        return out, nbad

    def push(self, x, layout: str = "ct", stream=None, out=None):
        """net_streams_push: ``x`` is a CUDA/HIP int8 tensor of every session's new samples, "ct" =
        [S][C][n] or "tc" = [S][n][C], any byte alignment.  Returns (logits [S][k][N] int8, n_bad): row
        (i, j) is the j-th window of the global grid that ends in this push, what forward_ct_torch
        returns for that window of session i's samples with its set loaded; the rows of windows that
        start before a session's origin are zero and counted in ``n_bad``, a device int32 tensor of one
        element (no host sync here).  ``out``: an int8 device tensor [S][k][N] to write instead."""
        return self._push(x, *self._push_source(x, layout, False), stream, out)

    def push_f32(self, x, stream=None, out=None, layout: str = "ct"):
        """net_streams_push_f32 / _f32_tm: ``x`` is a CUDA/HIP float32 tensor, "ct" = [S][C][n] or "tc" =
        [S][n][C] (frames as an amplifier delivers them); session i is quantised with the bank's scale
        of its set.  Returns what push returns."""
        return self._push(x, *self._push_source(x, layout, True), stream, out)

    def decimate(self, q: int, taps, stream=None) -> None:
        """net_streams_set_decimator: once, before the first push.  From then on the group takes raw
        float32 frames at ``q`` times the network's rate through ``push_raw`` and filters them with
        the FIR ``taps`` (K <= 128 finite float32 values, q <= 16; decimate.firwin_taps(q) is a
        default) inside the layer-1 kernel, bit for bit as decimate.fir_decimate states it."""
        super().decimate(q, taps, stream)

    def raw_info(self) -> list:
        """net_streams_raw_info: [q (0: no decimator), K, the raw position, the decimated position]."""
        return super().raw_info()

    def push_raw(self, frames, stream=None, out=None):
        """net_streams_push_raw_f32_tm: ``frames`` is a CUDA/HIP float32 tensor [S][n_raw][C] at q times
        the network's rate, at most q max_push frames.  Returns what push returns for the decimated
        samples these frames complete (possibly none: then the logits are [S][0][N])."""
        if not self.bank.has_scales:
            raise ValueError("a float32 source needs a bank created with scales")
        _check_tensor(frames, "frames", ("float32",), (self.S, "n", self.bank.dims.C))
        q, _, P, D = self.raw_info()
        n_raw = int(frames.shape[1])
        k = int(load().net_streams_push_windows(self.bank.handle, self.hop, D, raw_samples(q, P, n_raw)))
        return self._push(frames, "_raw_f32_tm", (), n_raw, stream, out, k)

    def windows_at(self, sessions, onsets, stream=None, out=None, check: bool = True, features: bool = False):
        """net_streams_windows_at: the windows of sessions ``sessions[w]`` whose first samples are
        ``onsets[w]`` on the group's position axis (the decimated one on a group with a decimator: a
        cue at raw frame a is the onset ceil(a / q)), read from the rings as they are (cue-locked
        trials).  Device tensors (int32, int64) or sequences of ints, any order, duplicates allowed;
        sorted by session the call reloads parameters least.  Returns the logits [W][N] int8, row w
        what forward_ct_torch returns for samples onsets[w] .. + T - 1 of the session with its set
        loaded.  A window that is not complete, no longer in the ring (see ``at_span``), from before
        the session's origin, or of a session outside the group gives a zero row; with ``check``
        their count is read back (a host sync) and a ValueError names it.  ``out``: an int8 device
        tensor [W][N] to write instead.  Ordered like a push; moves nothing.  With ``features``
        returns (logits, features [W][16][T // 64] int8): each window's layer-4 output under its
        session's set (forward_epochs_bank_torch), zeros beside a zero logit row."""
        return super().windows_at(sessions, onsets, stream, out, check, features)

    def at_span(self) -> tuple:
        """net_streams_at_span: (lo, hi), the onsets whose windows are in the rings now, lo =
        max(position - cap, 0) and hi = position - T; hi < lo: none yet.  A session's origin applies
        on top."""
        lo, hi = ctypes.c_int64(0), ctypes.c_int64(0)
        _check(load().net_streams_at_span(self.handle, ctypes.byref(lo), ctypes.byref(hi)), "net_streams_at_span")
        return lo.value, hi.value

    def restart(self, i: int, set: int, stream=None) -> None:
        """net_streams_restart: from the next push session ``i`` is decoded by ``set`` and answers no
        window that starts before the current position.  ``stream``: a torch stream (default: the
        current one of the group's device)."""
        super().restart(i, set, stream)


class StreamsEach(_StreamGroup):
    """net_streams_create_each: a stream group whose sessions advance at their own pace.  Every
    session has its own position in device memory, a push hands session i ``counts[i]`` samples
    (0 .. n_max, 0: it skips the tick) and returns the windows of the session's own grid that end in
    them.  A push reads nothing from the host, so after one eager push it may be captured into a
    graph and replayed with ``x`` and ``counts`` rewritten in place.  A class of its own beside
    Streams: its push takes and returns other things.  The ordering rule (all pushes, restarts and
    position copies of a group ordered with respect to one another), the bank's lifetime and
    ``close()`` are Streams'."""

    _create, _set_decimator = "net_streams_create_each", "net_streams_set_decimator_each"

    def info(self) -> list:
        """net_streams_info: [S, hop, max_push, cap, pushes enqueued so far, -1]."""
        return super().info()

    def origin(self, i: int) -> tuple:
        """net_streams_origin: (-1, the set of session ``i``): an each-group keeps no origin."""
        return super().origin(i)

    def rows(self, n_max: int) -> int:
        """net_streams_each_rows: kmax, the rows per session of a push of at most ``n_max`` samples."""
        return int(load().net_streams_each_rows(self.hop, n_max))

    def _positions(self, name: str, stream):
        torch = _torch()
        s = _stream_on(self.device, stream)
        with torch.cuda.stream(s):
            out = torch.empty((self.S,), dtype=torch.int64, device=f"cuda:{self.device}")
        _check(getattr(load(), name)(self.handle, out.data_ptr(), s.cuda_stream), name)
        return out

    def positions(self, stream=None):
        """net_streams_positions: the sessions' positions, an int64 device tensor [S] (no host sync).
        On a group with a decimator they are the decimated ones, ceil(raw_positions() / q)."""
        return self._positions("net_streams_positions", stream)

    def raw_positions(self, stream=None):
        """net_streams_raw_positions: the raw frames every session of a group with a decimator was
        given since its creation or last restart, an int64 device tensor [S] (no host sync)."""
        return self._positions("net_streams_raw_positions", stream)

    def decimate(self, q: int, taps, stream=None) -> None:
        """net_streams_set_decimator_each: once, before the first push.  From then on the group takes
        raw float32 frames at ``q`` times the network's rate through ``push_raw``, every session at
        its own pace and phase, filtered as Streams.decimate says; ``push`` and ``push_f32`` are
        refused."""
        super().decimate(q, taps, stream)

    def raw_info(self) -> list:
        """net_streams_raw_info: [q (0: no decimator), K, -1, -1] (the positions are on the device:
        ``raw_positions()`` and ``positions()``); without a decimator [0, 0, 0, pushes enqueued]."""
        return super().raw_info()

    def _push(self, x, dtype: str, code, n_max: int, counts, stream, out, kmax: Optional[int] = None):
        """``dtype``: the entry's suffix, "" (int8), "_f32", "_f32_tm" or "_raw_f32_tm"; ``kmax``: the rows
        per session, where they are not ``rows(n_max)``."""
        torch = _torch()
        _check_tensor(counts, "counts", ("int32",), (self.S,))
        if counts.device != x.device:
            raise ValueError("counts must be on x's device")
        kmax, N = self.rows(n_max) if kmax is None else kmax, self.bank.dims.N
        s, _ = _launch(x, stream)
        with torch.cuda.stream(s):  # the counter's zeroing precedes the launch on its stream
            nbad = torch.zeros((1,), dtype=torch.int32, device=x.device)
            cnt_out = torch.empty((self.S,), dtype=torch.int32, device=x.device)
            if out is None:
                out = torch.empty((self.S, kmax, N), dtype=torch.int8, device=x.device)
        _check_tensor(out, "out", ("int8",), (self.S, kmax, N))
        name = "net_streams_push_each" + dtype
        _check(getattr(load(), name)(self.handle, x.data_ptr(), *code, counts.data_ptr(), n_max, out.data_ptr(),
                                     cnt_out.data_ptr(), None, nbad.data_ptr(), s.cuda_stream), name)
        return out, cnt_out, nbad

    def push(self, x, counts, layout: str = "ct", stream=None, out=None):
        """net_streams_push_each: ``x`` is a CUDA/HIP int8 tensor of fixed slots, "ct" = [S][C][n_max]
        or "tc" = [S][n_max][C], any byte alignment; ``counts`` an int32 device tensor [S], the samples
        of each slot that are new.  Returns (logits [S][kmax][N] int8, cnt_out [S] int32, n_bad [1]
        int32), all device tensors, no host sync: rows j < cnt_out[i] of session i are its windows that
        end in this push, what forward_ct_torch returns for them with its set loaded; the other rows
        are not written.  A count outside 0 .. n_max gives cnt_out[i] = -1, moves nothing and is counted
        in n_bad.  ``out``: an int8 device tensor [S][kmax][N] to write instead."""
        return self._push(x, *self._push_source(x, layout, False), counts, stream, out)

    def push_f32(self, x, counts, stream=None, out=None, layout: str = "ct"):
        """net_streams_push_each_f32 / _f32_tm: ``x`` is a CUDA/HIP float32 tensor of fixed slots, "ct" =
        [S][C][n_max] or "tc" = [S][n_max][C]; session i is quantised with the bank's scale of its
        set.  Returns what push returns."""
        return self._push(x, *self._push_source(x, layout, True), counts, stream, out)

    def push_raw(self, frames, counts, stream=None, out=None):
        """net_streams_push_each_raw_f32_tm: ``frames`` is a CUDA/HIP float32 tensor of fixed slots
        [S][n_raw_max][C] at q times the network's rate, n_raw_max at most q max_push; ``counts`` an
        int32 device tensor [S], the frames of each slot that are new (the rest of a slot is never
        used).  Returns what push returns, with kmax = each_raw_rows(hop, q, n_raw_max): the windows
        that end in the decimated samples each session's frames complete (often none)."""
        if not self.bank.has_scales:
            raise ValueError("a float32 source needs a bank created with scales")
        _check_tensor(frames, "frames", ("float32",), (self.S, "n", self.bank.dims.C))
        n_raw_max = int(frames.shape[1])
        kmax = each_raw_rows(self.hop, self.raw_info()[0], n_raw_max)
        return self._push(frames, "_raw_f32_tm", (), n_raw_max, counts, stream, out, kmax)

    def windows_at(self, sessions, onsets, stream=None, out=None, check: bool = True, features: bool = False):
        """net_streams_windows_at on an each-group: Streams.windows_at with every onset in its
        session's own count since its last restart; a session's span is max(pos - cap, 0) ..
        pos - T of its position (``positions()``).  With device tensors and ``check=False`` the call
        reads nothing from the host and, after one eager call, may be captured behind a push.
        ``features``: Streams.windows_at's."""
        return super().windows_at(sessions, onsets, stream, out, check, features)

    def restart(self, i: int, set: int, stream=None) -> None:
        """net_streams_restart on an each-group: session ``i`` starts again at position 0 under
        ``set``; its grid starts at its next sample.  ``stream``: a torch stream (default: the current
        one of the group's device)."""
        super().restart(i, set, stream)


def streams_ring(streams, i: int) -> np.ndarray:
    """Test hook (mibminet_test_streams_ring): the layer-1 ring of session ``i`` of a Streams or
    StreamsEach group, [16][2 cap] int8, read after synchronising its device."""
    out = np.empty((16, 2 * streams.cap), np.int8)
    _check(load().mibminet_test_streams_ring(streams.handle, i, out.ctypes.data), "mibminet_test_streams_ring")
    return out


def streams_seek(streams, pos, origin=None) -> None:
    """Test hook (mibminet_test_streams_seek): places the fresh Streams or StreamsEach group at the
    positions ``pos`` (S ints; raw ones on a group with a decimator), a uniform group's origins at
    ``origin`` (S ints) or, by default, at the new position.  After ``decimate`` and ``prefilter``,
    before the first push or restart."""
    def arr(v):
        return None if v is None else (ctypes.c_int64 * len(v))(*[int(e) for e in v])

    if len(pos) != streams.S or (origin is not None and len(origin) != streams.S):
        raise ValueError(f"one position (and origin) for each of the {streams.S} sessions")
    _check(load().mibminet_test_streams_seek(streams.handle, arr(pos), arr(origin)), "mibminet_test_streams_seek")


def raw_samples(q: int, raw_pos: int, n_raw: int) -> int:
    """net_streams_raw_samples: the decimated samples that ``n_raw`` raw frames at raw position
    ``raw_pos`` complete under factor ``q``, ceil((raw_pos + n_raw) / q) - ceil(raw_pos / q); 0 for
    q == 0 or when the sum passes 2^64 - 1."""
    return int(load().net_streams_raw_samples(q, raw_pos, n_raw))


def each_raw_rows(hop: int, q: int, n_raw_max: int) -> int:
    """net_streams_each_raw_rows: the rows per session of an each-group's raw push of at most
    ``n_raw_max`` frames under factor ``q``, ceil(ceil(n_raw_max / q) / hop); 0 for hop == 0, q outside
    1 .. 16 or ceil(n_raw_max / q) outside 1 .. 65,536."""
    return int(load().net_streams_each_raw_rows(hop, q, n_raw_max))


def fir_decimate_torch(x, hist, taps, q: int, raw_pos: int, stream=None):
    """Test hook (mibminet_test_fir_decimate): the decimator's device function on one session's chunk
    ``x`` [n_raw][R] at raw position ``raw_pos``, with the history ``hist`` [K - 1][R] in slot order
    (frame a at slot a mod (K - 1); ignored for K == 1) and the taps [K], all float32 device
    tensors.  Returns the decimated floats [m][R] before the quantiser."""
    torch = _torch()
    _check_tensor(x, "x", ("float32",), ("n", "R"))
    _check_tensor(taps, "taps", ("float32",), ("K",))
    n_raw, R, K = int(x.shape[0]), int(x.shape[1]), int(taps.shape[0])
    if K > 1:
        _check_tensor(hist, "hist", ("float32",), (K - 1, R))
    s, dev = _launch(x, stream)
    out = torch.empty((raw_samples(q, raw_pos, n_raw), R), dtype=torch.float32, device=x.device)
    _check(load().mibminet_test_fir_decimate(x.data_ptr(), n_raw, R, hist.data_ptr() if K > 1 else None, taps.data_ptr(), K,
                                             q, raw_pos, out.data_ptr(), dev, s.cuda_stream), "mibminet_test_fir_decimate")
    return out


def sos_filter_torch(x, sos, state, stream=None):
    """Test hook (mibminet_test_sos_filter): the prefilter's kernel on one session's chunk ``x`` [n][R]
    with the state ``state`` [M][2][R] before it (float32 device tensors) and the sections ``sos``
    [M][5] (a host array, float32).  Returns (the filtered floats [n][R], the new state [M][2][R])."""
    torch = _torch()
    c = np.ascontiguousarray(sos, dtype=np.float32)
    if c.ndim != 2 or c.shape[1] != 5:
        raise ValueError("sos must be an array [M][5]")
    _check_tensor(x, "x", ("float32",), ("n", "R"))
    n, R, M = int(x.shape[0]), int(x.shape[1]), c.shape[0]
    _check_tensor(state, "state", ("float32",), (M, 2, R))
    s, dev = _launch(x, stream)
    out, new = torch.empty_like(x), torch.empty_like(state)
    _check(load().mibminet_test_sos_filter(x.data_ptr() if n else None, n, R, c.ctypes.data, M, state.data_ptr(),
                                           out.data_ptr() if n else None, new.data_ptr(), dev, s.cuda_stream),
           "mibminet_test_sos_filter")
    return out, new


def quantize_input_torch(x, scale: float, stream=None):
    """Input quantiser (net_quantize_input_f32/_f64): x is a CUDA/HIP float32 or float64 tensor
    [B][C][T] (the reference's input.npz layout); returns the batched int8 layout [B][stride]
    (stride = C*T rounded up to 16, each trial [T][C]) that forward_torch consumes.  Semantics of
    the reference's quantize_to_int (functional.py:308-334) in the input's precision."""
    dt = _check_tensor(x, "x", ("float32", "float64"), ("B", "C", "T"))
    B, C, T = x.shape
    y = _torch().empty((B, _packed_stride(C, T)), dtype=_torch().int8, device=x.device)
    s, dev = _launch(x, stream)
    fn = load().net_quantize_input_f32 if dt == "float32" else load().net_quantize_input_f64
    _check(fn(x.data_ptr(), y.data_ptr(), B, C, T, scale, dev, s.cuda_stream), "net_quantize_input")
    return y


def argmax_torch(logits, stream=None):
    """Class per trial (net_argmax_batch): logits is a CUDA/HIP int8 tensor [B][N]; returns an int32
    tensor [B] holding the first maximal index of each row (torch.max(dim=1)'s rule)."""
    _check_tensor(logits, "logits", ("int8",), ("B", "N"))
    B, N = logits.shape
    out = _torch().empty((B,), dtype=_torch().int32, device=logits.device)
    s, dev = _launch(logits, stream)
    _check(load().net_argmax_batch(logits.data_ptr(), out.data_ptr(), B, N, dev, s.cuda_stream), "net_argmax_batch")
    return out


def pack_trials_torch(x, stream=None):
    """net_pack_trials_i8: x is a CUDA/HIP int8 tensor [B][C][T] (channel-major); returns the
    batched layout [B][stride] (each trial [T][C], pad zero) that forward_torch consumes."""
    _check_tensor(x, "x", ("int8",), ("B", "C", "T"))
    B, C, T = x.shape
    y = _torch().empty((B, _packed_stride(C, T)), dtype=_torch().int8, device=x.device)
    s, dev = _launch(x, stream)
    _check(load().net_pack_trials_i8(x.data_ptr(), y.data_ptr(), B, C, T, dev, s.cuda_stream), "net_pack_trials_i8")
    return y


def check_trials(x, channel_major: bool, require_contiguous: bool = True) -> None:
    """Raises ValueError unless ``x`` (NumPy array or torch tensor) is a C-contiguous int8 batch of
    trials in the chosen layout (check_trial_shape).  The C ABI sees only pointers and counts, so a
    batch of another element type (e.g. int64 from rng.integers) or with strides would otherwise
    run and its bytes be read as int8 trials.  ``require_contiguous=False``: callers that copy the
    batch contiguously themselves before it reaches a pointer (shard.forward_devices)."""
    _check_tensor(x, "trials", ("int8",), device=False, contiguous=require_contiguous)
    check_trial_shape(tuple(x.shape), channel_major)


def check_trial_shape(shape, channel_major: bool) -> None:
    """Raises ValueError unless ``shape`` is a batch of trials in the chosen layout: [B][C][T]
    (channel-major) or [B][trial_stride] (time-major).  The C ABI sees only pointers and counts, so
    a batch in the other layout would otherwise run and return wrong logits."""
    d = _dims()
    want = (d.C, d.T) if channel_major else (trial_stride(),)
    if len(shape) != 1 + len(want) or tuple(shape[1:]) != want:
        kind = f"[B][{d.C}][{d.T}] (channel-major)" if channel_major else f"[B][{want[0]}] (time-major)"
        raise ValueError(f"trials must be {kind}, got {tuple(shape)}")


def model_compute_batch_multi(xs, ys, devices, channel_major: bool = False) -> None:
    """net_model_compute_batch_multi(_ct): xs[i] / ys[i] are device tensors on devices[i]
    ([B_i][trial_stride], or [B_i][C][T] with ``channel_major``, and [B_i][N] int8); one host call
    runs every shard and waits for all."""
    n = len(devices)
    if not (len(xs) == len(ys) == n):
        raise ValueError("xs, ys and devices must have the same length")
    d = _dims()
    for x, y in zip(xs, ys):
        check_trials(x, channel_major)
        if tuple(y.shape) != (x.shape[0], d.N):
            raise ValueError(f"logits must be [B][{d.N}] per shard, got {tuple(y.shape)}")
    dev = (ctypes.c_int * n)(*devices)
    xp = (ctypes.c_void_p * n)(*[x.data_ptr() for x in xs])
    yp = (ctypes.c_void_p * n)(*[y.data_ptr() for y in ys])
    bs = (ctypes.c_size_t * n)(*[x.shape[0] for x in xs])
    fn = load().net_model_compute_batch_multi_ct if channel_major else load().net_model_compute_batch_multi
    _check(fn(n, dev, xp, yp, bs, None), "net_model_compute_batch_multi")
