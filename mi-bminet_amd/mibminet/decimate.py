"""The FIR decimator of a stream group (net_streams_set_decimator, include/mibminet.h), stated in
NumPy: the arithmetic the layer-1 kernel of a raw push runs, bit for bit, and a default low-pass.

Decimated sample d of a session, electrode r, is

    acc = +0.0f;  for k = 0 .. K-1, ascending:  acc = RN(acc + RN(h[k] * raw[q*d - k][r]))

with raw[a] = 0 for a < 0 and every product and every sum rounded to float32 on its own.  Sample d
exists once raw frame q*d has arrived, so after P frames there are D(P) = ceil(P / q) samples.

Ahead of it, the IIR prefilter of net_streams_set_prefilter: sos_filter states the biquad cascade the
prefilter kernel runs, bit for bit, and biquad and butter_sos design the usual sections (a notch, a
Butterworth high-pass or low-pass) without scipy.
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


def sos_filter(x, sos, state=None, track_min: bool = False):
    """The prefilter of a stream group (net_streams_set_prefilter) on the raw frames ``x`` [n][R]
    float32, in arrival order: M second-order sections ``sos`` [M][5] = {b0, b1, b2, a1, a2} float32
    (a0 = 1), ascending, transposed direct form II, from the state ``state`` [M][2][R] float32 (z1
    then z2 of a section; None: zeros).  With v a section's input,

        w = RN(RN(b0 v) + z1);  z1' = RN(RN(RN(b1 v) - RN(a1 w)) + z2);  z2' = RN(RN(b2 v) - RN(a2 w))

    every product and every sum or difference a float32 operation of its own, as the kernel does
    them; w is the next section's input and the last one's the output.  Vectorised over R, a loop
    over frames and sections.  Returns (y [n][R] float32, the new state); with ``track_min`` also the
    smallest non-zero magnitude among all intermediates (inf if there is none).  The result does not
    depend on how the frames are split into calls."""
    x = np.asarray(x)
    c = np.asarray(sos)
    if x.dtype != np.float32 or x.ndim != 2:
        raise ValueError("x must be a float32 array [n][R]")
    if c.dtype != np.float32 or c.ndim != 2 or c.shape[1] != 5 or c.shape[0] < 1:
        raise ValueError("sos must be a float32 array [M][5], M >= 1")
    M, (n, R) = c.shape[0], x.shape
    z = np.zeros((M, 2, R), np.float32) if state is None else np.array(state)
    if z.dtype != np.float32 or z.shape != (M, 2, R):
        raise ValueError(f"state must be a float32 array [{M}][2][{R}]")
    y = np.empty_like(x)
    low = np.inf
    with np.errstate(all="ignore"):
        for t in range(n):
            v = x[t]
            for j in range(M):
                b0, b1, b2, a1, a2 = c[j]
                p0 = b0 * v
                w = p0 + z[j, 0]
                p1, q1 = b1 * v, a1 * w
                d1 = p1 - q1
                p2, q2 = b2 * v, a2 * w
                z[j, 0] = d1 + z[j, 1]
                z[j, 1] = p2 - q2
                if track_min:
                    m = np.abs(np.stack([p0, w, p1, q1, d1, p2, q2, z[j, 0], z[j, 1]]))
                    m = m[m > 0]
                    if m.size:
                        low = min(low, float(m.min()))
                v = w
            y[t] = v
    return (y, z, low) if track_min else (y, z)


def biquad64(kind: str, f0: float, fs: float, Q: float) -> np.ndarray:
    """The float64 design behind biquad: {b0, b1, b2, a1, a2} with a0 = 1."""
    if not 0.0 < f0 < fs / 2.0 or Q <= 0.0:
        raise ValueError("0 < f0 < fs / 2 and Q > 0")
    w0 = 2.0 * np.pi * f0 / fs
    cs, alpha = np.cos(w0), np.sin(w0) / (2.0 * Q)
    if kind == "notch":
        b = (1.0, -2.0 * cs, 1.0)
    elif kind == "highpass":
        b = ((1.0 + cs) / 2.0, -(1.0 + cs), (1.0 + cs) / 2.0)
    elif kind == "lowpass":
        b = ((1.0 - cs) / 2.0, 1.0 - cs, (1.0 - cs) / 2.0)
    else:
        raise ValueError('kind must be "notch", "highpass" or "lowpass"')
    return np.array([b[0], b[1], b[2], -2.0 * cs, 1.0 - alpha], np.float64) / (1.0 + alpha)


def biquad(kind: str, f0: float, fs: float, Q: float) -> np.ndarray:
    """One second-order section, float32 [1][5] = {b0, b1, b2, a1, a2}: the analogue notch
    (s^2 + 1) / (s^2 + s/Q + 1), high-pass s^2 / (s^2 + s/Q + 1) or low-pass 1 / (s^2 + s/Q + 1) at
    ``f0`` under sampling rate ``fs``, through the bilinear transform with ``f0`` prewarped, designed
    in float64 and rounded last."""
    return biquad64(kind, f0, fs, Q)[None].astype(np.float32)


def butter_sos64(order: int, fc: float, fs: float, kind: str) -> np.ndarray:
    """The float64 design behind butter_sos, [order / 2][5]."""
    if kind not in ("highpass", "lowpass"):
        raise ValueError('kind must be "highpass" or "lowpass"')
    if order < 2 or order > 16 or order % 2:
        raise ValueError("an even order in 2 .. 16")
    # the pole pairs of the Butterworth prototype, the flattest first: Q = 1 / (2 sin((2 k + 1) pi / (2 order)))
    Qs = sorted(1.0 / (2.0 * np.sin((2 * k + 1) * np.pi / (2.0 * order))) for k in range(order // 2))
    return np.stack([biquad64(kind, fc, fs, Q) for Q in Qs])


def butter_sos(order: int, fc: float, fs: float, kind: str = "highpass") -> np.ndarray:
    """A Butterworth high-pass or low-pass of even ``order`` <= 16 with its -3 dB point at ``fc``, as
    order / 2 sections of biquad: float32 [order / 2][5].  scipy.signal.butter(order, fc, kind,
    fs=fs, output="sos") in exact arithmetic, up to the order of the sections."""
    return butter_sos64(order, fc, fs, kind).astype(np.float32)


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
