"""An each-group's decimator without a GPU: the restatement of the per-session plan of a raw push
(support_decim_each.plan_each_raw) applied to the ragged schedules the GPU tests run, held against
decimate.raw_decimated, decimate.fir_decimate and support_streams.plan, and the schedules certified to
contain what tests/test_gpu_streams_each_decim.py relies on."""
import numpy as np
import pytest

import support_decim as sd
import support_decim_each as sde
import support_streams as ss
from mibminet import decimate

CASES = [(64, 2, 7), (64, 3, 33), (480, 2, 7), (480, 3, 33), (64, 16, 128)]


@pytest.mark.parametrize("T,q,K", CASES)
def test_schedule_contains_what_the_gpu_tests_rely_on(T, q, K):
    w = sde.certify(T, q, K)
    assert len(w.n_raw_max) < 400  # the GPU test pushes once per tick


@pytest.mark.parametrize("T,q,K", CASES + [(64, 1, 1), (64, 3, 1)])
def test_plan_of_a_ragged_schedule_is_the_uniform_plan_per_session(T, q, K):
    """Per session, the ticks with a count are a uniform group's raw pushes of those counts: the same
    decimated positions, m and windows (support_decim.plan, support_streams.plan), pos = D(P) before
    and after every tick, and the samples a tick completes end inside its count."""
    n_max, counts = sde.schedule(T, q, K)
    w = sde.walk(T, q, K)
    for s in range(sde.S):
        ns = [int(c) for c in counts[:, s]]
        uni = sd.plan(T, q, ns)
        dec = ss.plan(T, sde.HOP, [u[3] for u in uni])
        P = 0
        for t, (Pu, n, d0, m, k, onsets) in enumerate(uni):
            assert (w.P[t, s], w.m[t, s], w.k[t, s]) == (Pu, m, k) == (P, dec[t][1], dec[t][2])
            assert dec[t][0] == d0 == decimate.raw_decimated(q, P) and w.W0[t, s] == dec[t][3]
            assert w.off[t, s] == q * d0 - P and 0 <= w.off[t, s] < q
            assert w.slot0[t, s] == (P % (K - 1) if K > 1 else 0)
            assert m <= -(-n // q) <= -(-n_max[t] // q) and k <= sde.each_raw_rows(sde.HOP, q, n_max[t])
            if m:
                assert q * (m - 1) + w.off[t, s] <= n - 1  # no answered sample reads a frame at or past the count
            P += n
        assert P == w.fed[s]


def test_refused_counts_change_nothing():
    T, q, K, cap = 64, 3, 33, ss.cap(64, 37)
    for P in (0, 7, 301, sde.RAW_LIMIT - 5, sde.RAW_LIMIT):
        for cnt in (-1, 112, -2**31, 2**31 - 1, 6):
            ok, m, n, off, slot0, keep, n_dec, p0, k, at0, W0 = sde.plan_each_raw(T, 3, cap, q, K, P, cnt, 111)
            assert ok == (cnt == 6 and P + 6 <= sde.RAW_LIMIT)
            if not ok:
                assert (m, n, keep, n_dec, k) == (0, 0, 0, 0, 0) and p0 == decimate.raw_decimated(q, P) % cap


@pytest.mark.parametrize("q,K", [(2, 7), (3, 33), (16, 128)])
def test_chunked_fir_decimate_at_each_sessions_pace(q, K):
    """decimate.fir_decimate called chunk by chunk with the state and the position, at the counts of a
    ragged schedule, gives the bits of one call over the concatenation: what the GPU tests' reference
    rests on, and the caller's recipe that the raw push replaces."""
    T, R = 64, 5
    _, counts = sde.schedule(T, q, K)
    h = sd.taps(K, 11)
    for s in (1, 3):
        ns = [int(c) for c in counts[:40, s]]
        x = sd.inputs(np.random.default_rng([q, K, s]), (sum(ns), R))
        whole = decimate.fir_decimate(x, h, q)[0]
        parts, state, P = [], None, 0
        for n in ns:
            y, state = decimate.fir_decimate(x[P: P + n], h, q, state, P)
            parts.append(y)
            P += n
        np.testing.assert_array_equal(np.concatenate(parts).view(np.uint32), whole.view(np.uint32))
