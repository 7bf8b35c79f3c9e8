"""The FIR decimator of a stream group (net_streams_set_decimator, include/mibminet.h), stated in
NumPy: the arithmetic the layer-1 kernel of a raw push runs, bit for bit, and a default low-pass.

Decimated sample d of a session, electrode r, is

    acc = +0.0f;  for k = 0 .. K-1, ascending:  acc = RN(acc + RN(h[k] * raw[q*d - k][r]))

with raw[a] = 0 for a < 0 and every product and every sum rounded to float32 on its own.  Sample d
exists once raw frame q*d has arrived, so after P frames there are D(P) = ceil(P / q) samples.
"""
from __future__ import annotations

import numpy as np


def raw_decimated(q: int, P: int) -> int:
    """D(P) = ceil(P / q): the decimated samples that P raw frames complete."""
    return -(-P // q)


def fir_decimate(x, taps, q: int, state=None, pos: int = 0):
    """The decimated samples that the raw frames ``x`` [n][R] float32 complete, given at raw position
    ``pos`` after the K - 1 frames ``state`` [K - 1][R] (oldest first; None: zeros).  Returns
    (y [m][R] float32, the new state), m = D(pos + n) - D(pos).  The result does not depend on how
    the frames are split into calls: one float32 product and one float32 sum per tap, in tap order,
    as the kernel does them."""
    x = np.asarray(x)
    h = np.asarray(taps)
    if x.dtype != np.float32 or x.ndim != 2:
        raise ValueError("x must be a float32 array [n][R]")
    if h.dtype != np.float32 or h.ndim != 1 or h.size < 1:
        raise ValueError("taps must be a float32 array [K], K >= 1")
    if q < 1 or pos < 0:
        raise ValueError("q at least 1 and pos at least 0")
    K, (n, R) = h.size, x.shape
    if state is None:
        state = np.zeros((K - 1, R), np.float32)
    state = np.asarray(state)
    if state.dtype != np.float32 or state.shape != (K - 1, R):
        raise ValueError(f"state must be a float32 array [{K - 1}][{R}]")
    ext = np.concatenate([state, x])  # raw frame pos - (K - 1) + i at row i
    d0, d1 = raw_decimated(q, pos), raw_decimated(q, pos + n)
    rows = q * np.arange(d0, d1, dtype=np.int64) - pos + (K - 1)  # frame q d at row q d - pos + K - 1
    acc = np.zeros((d1 - d0, R), np.float32)
    with np.errstate(all="ignore"):
        for k in range(K):
            acc = acc + h[k] * ext[rows - k]  # float32 product, then float32 sum
    return acc, np.ascontiguousarray(ext[len(ext) - (K - 1):])


def firwin_taps(q: int, K: int | None = None) -> np.ndarray:
    """K float32 taps (default 20 q + 1) of a Hamming-windowed sinc low-pass with its cutoff at 1 / q
    of the Nyquist rate, scaled to unit gain at DC: scipy.signal.firwin(K, 1 / q, window="hamming")."""
    if q < 1:
        raise ValueError("q at least 1")
    K = 20 * q + 1 if K is None else K
    if K < 1:
        raise ValueError("K at least 1")
    m = np.arange(K, dtype=np.float64) - (K - 1) / 2.0
    h = np.sinc(m / q) / q
    if K > 1:
        h *= 0.54 - 0.46 * np.cos(2.0 * np.pi * np.arange(K) / (K - 1))
    return (h / h.sum()).astype(np.float32)
