"""What the decimator's GPU tests share (tests/test_gpu_streams_decim.py): inputs and taps whose
non-zero intermediates cannot be subnormal, one raw push schedule per (T, q, K), and, computed once per
case, the reference of every row and ring byte.  The reference is never another stream entry: it is
decimate.fir_decimate on the CPU, then the two-pass quantiser (lib.quantize_input_torch) with the
set's scale, then the C oracle on the materialised sliding windows (support_streams.rows_of)."""
import functools

import numpy as np

import support_bank as sb
import support_streams as ss
import support_windows_bank as swb
from mibminet import decimate, lib

SETS, S, HOP, MAX_PUSH = ss.SETS, ss.S, ss.HOP, ss.MAX_PUSH
# one scale per set of support_bank's five, of the order of the filters' outputs (inputs up to 2^10)
SCALES = (384.0, 900.0, 1500.0, 2600.5, 640.0)


def inputs(rng, shape):
    """float32 with magnitudes uniform in [2^-10, 2^10] and random signs: multiples of 2^-33."""
    mag = rng.uniform(2.0**-10, 2.0**10, size=shape)
    return (mag * rng.choice((-1.0, 1.0), size=shape)).astype(np.float32)


def taps(K, seed):
    """K float32 taps with magnitudes in [2^-10, 1] (multiples of 2^-33) or exactly zero, random signs;
    the first and the last are not zero.  A product of a tap and an input is then a multiple of 2^-66
    of magnitude at least 2^-20, and so is every partial sum that is not zero: nothing is subnormal."""
    rng = np.random.default_rng([K, seed])
    h = (rng.uniform(2.0**-10, 1.0, size=K) * rng.choice((-1.0, 1.0), size=K)).astype(np.float32)
    zero = rng.random(K) < 0.15
    zero[[0, -1]] = False
    h[zero] = 0.0
    return h


@functools.lru_cache(maxsize=None)
def schedule(T, q, K, max_push=MAX_PUSH):
    """The n_raw of a case: pushes of one frame (at q > 1 some complete no sample), pushes below q and,
    several in a row, below K - 1 (the history then spans more than one earlier push), q max_push, and
    a fixed pseudo-random tail until the ring has wrapped twice."""
    head = [1, 1, 1, max(q - 1, 1), 2, 3, 1, 5, q * max_push, 2, 2, 1, 4, q, q + 1, 1, 1]
    rng = np.random.default_rng([T, q, K])
    ns, raw = list(head), sum(head)
    while decimate.raw_decimated(q, raw) < 2 * ss.cap(T, max_push) + 16:
        n = q * max_push if len(ns) % 5 == 0 else int(rng.integers(1, q * max_push + 1))
        ns.append(n)
        raw += n
    return tuple(ns)


def plan(T, q, ns, hop=HOP, raw=0):
    """Per raw push of the list ns from raw position raw: (raw position, n_raw, decimated position, m,
    k, the k onsets)."""
    out, P = [], raw
    for n in ns:
        d0, d1 = decimate.raw_decimated(q, P), decimate.raw_decimated(q, P + n)
        k, W0 = ss.push_windows(T, hop, d0, d1 - d0), ss.windows_count(T, d0, hop)
        out.append((P, n, d0, d1 - d0, k, [(W0 + j) * hop for j in range(k)]))
        P += n
    return out


@functools.lru_cache(maxsize=None)
def frames(C, T, q, K):
    """[S][L][C] float32 raw frames, L the schedule's total.  Read-only."""
    x = inputs(np.random.default_rng([C, T, q, K, 3]), (S, sum(schedule(T, q, K)), C))
    x.setflags(write=False)
    return x


def two_pass(x_tc, scale):
    """The two-pass quantisation (net_quantize_input_f32) of float32 [L][C] -> int8 [C][L]."""
    import torch

    L, C = x_tc.shape
    q = lib.quantize_input_torch(torch.from_numpy(np.ascontiguousarray(x_tc.T)[None]).cuda(), scale)
    return np.ascontiguousarray(q.cpu().numpy()[0, : L * C].reshape(L, C).T)


def decimated(x_tc, h, q):
    """fir_decimate over the whole recording [L][C] from raw position 0, in one call."""
    return decimate.fir_decimate(np.ascontiguousarray(x_tc), h, q)[0]


def session_reference(ps, scale, x_tc, h, q, T, hop=HOP):
    """(int8 [C][Ld]: the quantised decimated samples of one session, rows [W][N]: the oracle's logits
    of every sliding window of them)."""
    qd = two_pass(decimated(x_tc, h, q), scale)
    return qd, ss.rows_of(ps, qd, T, hop)


@functools.lru_cache(maxsize=None)
def reference(C, T, N, q, K):
    """(sets, taps, qd [S] arrays [C][Ld], rows [S] arrays [W][N]) of frames(C, T, q, K), every session
    under its own set and scale."""
    sets, h, x = sb.sets(C, T, N), taps(K, 11), frames(C, T, q, K)
    both = [session_reference(sets[s], SCALES[s], x[i], h, q, T) for i, s in enumerate(SETS)]
    return sets, h, [b[0] for b in both], [b[1] for b in both]


def check_rings(st, sets, qd, set_of=SETS, skip=(), base=0):
    """Every ring (but those of the sessions `skip`) holds, twice, the oracle's layer 1 of the session's
    last cap decimated samples.  base: the position of qd's first sample on the group's axis (an int,
    or one per session), where the group did not start at 0."""
    c = st.cap
    for i, s in enumerate(set_of):
        if i in skip:
            continue
        Ld = qd[i].shape[1]
        t = np.arange(max(0, Ld - c), Ld)
        at = ((base if isinstance(base, int) else int(base[i])) % c + t) % c
        ring = lib.streams_ring(st, i)
        np.testing.assert_array_equal(ring[:, :c], ring[:, c:], err_msg=f"the two copies, session {i}")
        np.testing.assert_array_equal(ring[:, at], swb.layer1_of(sets[s], qd[i][:, t]), err_msg=f"session {i}")
