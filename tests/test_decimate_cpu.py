"""The NumPy statement of a stream group's decimator (mibminet/decimate.py) and the host-only entry
net_streams_raw_samples: no device here."""
import numpy as np
import pytest

from mibminet import decimate, lib

QK = [(1, 1), (2, 7), (3, 33), (2, 2), (5, 4)]
CHUNKINGS = ([103], [1, 5, 16, 47, 2, 1, 1, 30])
R = 5


def _case(q, K):
    rng = np.random.default_rng([q, K, 7])
    x = rng.standard_normal((103, R)).astype(np.float32) * np.float32(37.0)
    h = rng.standard_normal(K).astype(np.float32)
    return x, h


def _chunked(x, h, q, ns):
    state, pos, parts = None, 0, []
    for n in ns:
        y, state = decimate.fir_decimate(x[pos: pos + n], h, q, state, pos)
        assert y.dtype == np.float32 and y.shape == (decimate.raw_decimated(q, pos + n) - decimate.raw_decimated(q, pos), R)
        assert state.shape == (len(h) - 1, R)
        parts.append(y)
        pos += n
    assert pos == len(x)
    return np.concatenate(parts)


@pytest.mark.parametrize("q,K", QK)
def test_fir_decimate_is_independent_of_the_chunking(q, K):
    x, h = _case(q, K)
    assert sum(CHUNKINGS[0]) == sum(CHUNKINGS[1]) == len(x)
    whole, split = (_chunked(x, h, q, ns) for ns in CHUNKINGS)
    assert whole.shape == (-(-len(x) // q), R)
    np.testing.assert_array_equal(whole.view(np.uint32), split.view(np.uint32))


@pytest.mark.parametrize("q,K", QK)
def test_fir_decimate_against_float64_convolution(q, K):
    """Within K 2^-23 sum|h| max|x| of the float64 convolution, decimated: each of the K products and
    K sums rounds once, by at most 2^-24 of a magnitude below sum|h| max|x|."""
    x, h = _case(q, K)
    got = _chunked(x, h, q, CHUNKINGS[1])
    bound = K * 2.0**-23 * np.abs(h.astype(np.float64)).sum() * np.abs(x.astype(np.float64)).max()
    for r in range(R):
        want = np.convolve(x[:, r].astype(np.float64), h.astype(np.float64))[: len(x)][::q]
        assert np.abs(got[:, r] - want).max() <= bound, (q, K, r)


def test_identity_and_stride():
    x, _ = _case(3, 1)
    one = np.ones(1, np.float32)
    np.testing.assert_array_equal(_chunked(x, one, 1, CHUNKINGS[1]).view(np.uint32), x.view(np.uint32))
    np.testing.assert_array_equal(_chunked(x, one, 3, CHUNKINGS[1]).view(np.uint32), x[::3].view(np.uint32))


def test_fir_decimate_refuses_other_types():
    x, h = _case(2, 7)
    for bad in (lambda: decimate.fir_decimate(x.astype(np.float64), h, 2), lambda: decimate.fir_decimate(x, h.astype(np.float64), 2),
                lambda: decimate.fir_decimate(x, h, 0), lambda: decimate.fir_decimate(x, h, 2, np.zeros((5, R), np.float32)),
                lambda: decimate.fir_decimate(x[:, 0], h, 2)):
        with pytest.raises(ValueError):
            bad()


def test_raw_samples_against_python_integers():
    I63, U64 = 2**63 - 1, 2**64 - 1
    for q in (0, 1, 2, 3, 5, 16, 17):
        for P in (0, 1, 2, 15, 16, 17, 2**40 + 3, I63 - 65536, I63 - 1, I63, I63 + 1, U64 - 65536, U64 - 1, U64):
            for n in (0, 1, 2, 15, 16, 47, 65536, 2**20):
                want = 0 if q == 0 or P + n > U64 else -(-(P + n) // q) - -(-P // q)
                assert lib.raw_samples(q, P, n) == want, (q, P, n)


@pytest.mark.parametrize("q", [2, 3, 4, 5])
def test_firwin_taps_against_scipy(q):
    signal = pytest.importorskip("scipy.signal")
    for K in (20 * q + 1, 7, 32):
        want = signal.firwin(K, 1.0 / q, window="hamming")
        got = decimate.firwin_taps(q) if K == 20 * q + 1 else decimate.firwin_taps(q, K)
        assert got.dtype == np.float32 and got.shape == (K,)
        assert np.abs(got - want).max() <= 1e-6, (q, K)
    assert abs(float(decimate.firwin_taps(q).astype(np.float64).sum()) - 1.0) <= 1e-6
