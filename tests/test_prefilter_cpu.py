"""The prefilter's statement in NumPy (mibminet/decimate.py: sos_filter, biquad, butter_sos) and the two
conditions that tests/support_prefilter.py promises of every reference the GPU tests use.  No GPU."""
import numpy as np
import pytest

import support_bank as sb
import support_decim as sd
import support_prefilter as pf
from mibminet import decimate, lib

GEOMETRIES = sb.GEOMETRIES[:2]
QK = [(2, 7), (3, 33)]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def scalar_sos(x, sos, state):
    """sos_filter one np.float32 operation at a time."""
    n, R = x.shape
    z, y = np.array(state), np.empty_like(x)
    for r in range(R):
        for t in range(n):
            v = x[t, r]
            for j, (b0, b1, b2, a1, a2) in enumerate(sos):
                w = np.float32(np.float32(b0 * v) + z[j, 0, r])
                z1 = np.float32(np.float32(np.float32(b1 * v) - np.float32(a1 * w)) + z[j, 1, r])
                z[j, 1, r] = np.float32(np.float32(b2 * v) - np.float32(a2 * w))
                z[j, 0, r] = z1
                v = w
            y[t, r] = v
    return y, z


@pytest.mark.parametrize("M", [1, 3, 8])
def test_sos_filter_is_independent_of_the_split(M):
    rng = np.random.default_rng([M, 1])
    x, sos = sd.inputs(rng, (211, 5)), pf.sections(M, 4)
    whole, end = decimate.sos_filter(x, sos)
    for cuts in ([1, 2, 3, 50, 51, 210], [100], list(range(1, 211))):
        state, parts, at = None, [], 0
        for c in cuts + [211]:
            y, state = decimate.sos_filter(x[at:c], sos, state)
            parts.append(y)
            at = c
        assert np.array_equal(bits(np.concatenate(parts)), bits(whole)) and np.array_equal(bits(state), bits(end))
    y0, s0 = decimate.sos_filter(x[:0], sos, end)
    assert y0.shape == (0, 5) and np.array_equal(bits(s0), bits(end))


def test_a_cascade_is_its_sections_one_after_another():
    rng = np.random.default_rng(2)
    x, A, B = sd.inputs(rng, (150, 7)), pf.sections(2, 5), pf.sections(3, 6)
    both, state = decimate.sos_filter(x, np.concatenate([A, B]))
    ya, sa = decimate.sos_filter(x, A)
    yb, sb_ = decimate.sos_filter(ya, B)
    assert np.array_equal(bits(both), bits(yb)) and np.array_equal(bits(state), bits(np.concatenate([sa, sb_])))


def test_sos_filter_against_a_scalar_loop():
    rng = np.random.default_rng(3)
    x, sos = sd.inputs(rng, (40, 3)), pf.sections(3, 7)
    state = sd.inputs(rng, (3, 2, 3)) * np.float32(2.0**-8)
    y, z = decimate.sos_filter(x, sos, state)
    ys, zs = scalar_sos(x, sos, state)
    assert np.array_equal(bits(y), bits(ys)) and np.array_equal(bits(z), bits(zs))
    y2, z2, low = decimate.sos_filter(x, sos, state, track_min=True)
    assert np.array_equal(bits(y2), bits(y)) and np.array_equal(bits(z2), bits(z)) and 0 < low <= np.abs(y[y != 0]).min()


def test_the_identity_section_returns_its_input():
    x = sd.inputs(np.random.default_rng(4), (64, 9))
    y, z = decimate.sos_filter(x, pf.IDENTITY)
    assert np.array_equal(bits(y), bits(x)) and not z.any()


def test_sos_filter_against_float64():
    """In exact arithmetic the statement is the direct-form recursion of scipy.signal.sosfilt."""
    x, sos = sd.inputs(np.random.default_rng(5), (300, 4)), pf.sections(3, 8)
    y = decimate.sos_filter(x, sos)[0]
    v = x.astype(np.float64)
    for b0, b1, b2, a1, a2 in sos.astype(np.float64):
        w = np.zeros_like(v)
        for t in range(len(v)):
            w[t] = b0 * v[t] + (b1 * v[t - 1] - a1 * w[t - 1] if t >= 1 else 0) + (b2 * v[t - 2] - a2 * w[t - 2] if t >= 2 else 0)
        v = w
    assert np.abs(y - v).max() <= 2.0**-18 * np.abs(v).max()


def test_sos_filter_refuses_other_types():
    x, sos = np.zeros((4, 3), np.float32), pf.sections(2, 1)
    for bad in (lambda: decimate.sos_filter(x.astype(np.float64), sos), lambda: decimate.sos_filter(x, sos.astype(np.float64)),
                lambda: decimate.sos_filter(x[0], sos), lambda: decimate.sos_filter(x, sos[:, :4]),
                lambda: decimate.sos_filter(x, sos[:0]), lambda: decimate.sos_filter(x, sos, np.zeros((2, 2, 4), np.float32))):
        with pytest.raises(ValueError):
            bad()


def response(sos64, f, fs):
    z = np.exp(-2j * np.pi * np.asarray(f, np.float64) / fs)
    H = np.ones_like(z)
    for b0, b1, b2, a1, a2 in sos64:
        H = H * (b0 + b1 * z + b2 * z * z) / (1.0 + a1 * z + a2 * z * z)
    return H


@pytest.mark.parametrize("kind", ["highpass", "lowpass"])
@pytest.mark.parametrize("order,fc,fs", [(2, 40.0, 250.0), (4, 0.5, 1000.0), (8, 30.0, 500.0), (16, 60.0, 250.0)])
def test_butterworth_designs(kind, order, fc, fs):
    d = decimate.butter_sos64(order, fc, fs, kind)
    assert d.shape == (order // 2, 5)
    assert abs(abs(response(d, [fc], fs)[0]) ** 2 - 0.5) <= 1e-9
    g = np.abs(response(d, np.linspace(fs / 4000.0, fs / 2.0 * 0.999, 1500), fs))
    step = np.diff(g) if kind == "highpass" else -np.diff(g)
    assert (step >= -1e-12).all() and g.max() <= 1.0 + 1e-9
    s = decimate.butter_sos(order, fc, fs, kind)
    assert s.dtype == np.float32 and np.array_equal(s, d.astype(np.float32))
    for bad in (0, 3, 18):
        with pytest.raises(ValueError):
            decimate.butter_sos(bad, fc, fs, kind)


@pytest.mark.parametrize("f0,fs,Q", [(50.0, 500.0, 30.0), (60.0, 1000.0, 10.0), (50.0, 250.0, 0.7)])
def test_notch_design(f0, fs, Q):
    d = decimate.biquad64("notch", f0, fs, Q)
    assert abs(response([d], [f0], fs)[0]) <= 1e-12 and abs(abs(response([d], [0.0], fs)[0]) - 1.0) <= 1e-12
    s = decimate.biquad("notch", f0, fs, Q)
    assert s.shape == (1, 5) and s.dtype == np.float32 and np.array_equal(s[0], d.astype(np.float32))
    with pytest.raises(ValueError):
        decimate.biquad("bandpass", f0, fs, Q)
    with pytest.raises(ValueError):
        decimate.biquad("notch", fs, fs, Q)


def test_test_sections_are_what_the_issue_asks():
    for m, seed in ((1, 1), (3, pf.SEED), (8, 3)):
        s = pf.sections(m, seed).astype(np.float64)
        rho = np.sqrt(s[:, 4])
        assert ((rho > 0.29) & (rho < 0.91)).all() and (np.abs(s[:, 3]) <= 2 * rho + 1e-6).all()
        assert (np.abs(s[:, :3]).sum(axis=1) <= (1 - rho) ** 2 * (1 + 1e-5)).all()


def test_prototypes_name_the_prefilter():
    for name in ("net_streams_set_prefilter", "net_streams_prefilter_info"):
        assert name in lib.PROTOTYPES and name in lib.EXPORTED_SYMBOLS
    assert "mibminet_test_sos_filter" in lib.PROTOTYPES
    L = lib.load()
    assert L.net_streams_set_prefilter(None, None, 3, None) == lib.NET_ERR_INVALID
    assert L.net_streams_prefilter_info(None, None) == lib.NET_ERR_INVALID


# ---- the two conditions on the references of tests/test_gpu_streams_prefilter.py --------------------------
@pytest.mark.parametrize("C,T,N", GEOMETRIES)
@pytest.mark.parametrize("q,K", QK)
def test_the_schedules_references_are_certified(C, T, N, q, K):
    """The uniform group's cases (the schedule, the restart, windows_at): the whole recordings."""
    _, y, low = pf.filtered_frames(C, T, q, K)
    pf.certify_min(low)
    for i, s in enumerate(pf.SETS):
        pf.certify_spread(sd.decimated(y[i], sd.taps(K, 11), q), pf.SCALES[s], f"session {i}")


def test_the_other_references_are_certified():
    """The hook's cases, the each-group's, the restarted session's and the widened montage's."""
    for M, R, n, x, sos, state in pf.hook_cases():
        pf.certify_min(decimate.sos_filter(x, sos, state, track_min=True)[2])
    for name, case in (("each", pf.each_case()), ("restart", pf.restart_case()), ("montage", pf.montage_case())):
        for i, (x_tc, scale, h, q) in enumerate(case.sessions):
            y, low = pf.filtered(x_tc, case.sos, True)
            pf.certify_min(low)
            pf.certify_spread(sd.decimated(y, h, q), scale, f"{name}, session {i}")
