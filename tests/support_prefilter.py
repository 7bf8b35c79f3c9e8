"""What the prefilter's tests share (tests/test_prefilter_cpu.py, tests/test_gpu_streams_prefilter.py):
seeded second-order sections with their poles well inside the unit circle, scales of the order of
the filtered signals, and, computed once per case, the reference of every row and ring byte.  The
reference is never another stream entry: decimate.sos_filter on the CPU over a session's whole
recording from zero state, then support_decim's chain (decimate.fir_decimate, the two-pass quantiser
with the set's scale, the C oracle on the materialised sliding windows).

Two conditions hold on the reference alone and are asserted without a GPU (test_prefilter_cpu.py) for
every case the GPU tests use: no intermediate of the recursion is below 2^-100 in magnitude unless it
is zero (certify_min), and every session's quantised reference samples take at least 64 distinct int8
values (certify_spread, on params.quantize_to_int, the quantiser's statement in NumPy)."""
import functools

import numpy as np

import support_bank as sb
import support_decim as sd
import support_streams as ss
from mibminet import decimate
from mibminet.params import quantize_to_int

SETS, S, HOP, MAX_PUSH = sd.SETS, sd.S, sd.HOP, sd.MAX_PUSH
M = 3
SEED = 2
# one scale per set of support_bank's five, of the order of the filtered and decimated signals: the
# gain of sections(M, SEED) is a few thousandths (sum |b| = (1 - rho)^2 bounds a section's gain by
# its smallest value over the circle), so inputs up to 2^10 leave the FIRs with a deviation of 3 to 7
SCALES = (20.0, 26.0, 32.0, 40.5, 23.0)
MIN_MAGNITUDE = 2.0**-100
MIN_DISTINCT = 64
MONTAGE_SCALES = (14.0, 17.5, 20.0)  # its taps (support_decim.taps(7, 12)) leave less
IDENTITY = np.array([[1, 0, 0, 0, 0]], np.float32)


def sections(m, seed):
    """m sections [m][5] float32: poles at radius rho in 0.3 .. 0.9 and a random angle theta
    (a1 = -2 rho cos theta, a2 = rho^2), b with random signs and magnitudes in [2^-6, 1], scaled so
    that sum |b| = (1 - rho)^2: 1 / |A| <= (1 - rho)^-2 on the unit circle, so no section's gain
    passes 1 and nothing grows along the cascade."""
    rng = np.random.default_rng([m, seed, 77])
    out = np.empty((m, 5), np.float64)
    for j in range(m):
        rho, theta = rng.uniform(0.3, 0.9), rng.uniform(0.0, np.pi)
        b = rng.uniform(2.0**-6, 1.0, size=3) * rng.choice((-1.0, 1.0), size=3)
        out[j, :3] = b * ((1.0 - rho) ** 2 / np.abs(b).sum())
        out[j, 3:] = -2.0 * rho * np.cos(theta), rho * rho
    out = out.astype(np.float32)
    out.setflags(write=False)
    return out


def filtered(x, sos, track_min=False):
    """decimate.sos_filter over whole recordings x [..][L][C] from zero state, one call: electrodes and
    sessions are independent, so they go side by side as the R of one [L][R] array.  Returns the
    filtered frames in x's shape (with track_min: and the smallest non-zero magnitude)."""
    x = np.asarray(x)
    L, C = x.shape[-2:]
    flat = np.ascontiguousarray(np.moveaxis(x.reshape(-1, L, C), 1, 0).reshape(L, -1))
    res = decimate.sos_filter(flat, sos, None, track_min)
    y = np.ascontiguousarray(np.moveaxis(res[0].reshape(L, -1, C), 0, 1)).reshape(x.shape)
    return (y, res[2]) if track_min else y


@functools.lru_cache(maxsize=None)
def filtered_frames(C, T, q, K):
    """(sos, [S][L][C] float32: support_decim.frames(C, T, q, K) through sections(M, SEED), the smallest
    non-zero magnitude among the intermediates).  Read-only."""
    sos = sections(M, SEED)
    y, low = filtered(sd.frames(C, T, q, K), sos, True)
    y.setflags(write=False)
    return sos, y, low


def quantised_cpu(x_tc, scale):
    """int8 [L][C]: the quantiser's statement in NumPy, for certify_spread (no GPU)."""
    return quantize_to_int(np.asarray(x_tc, np.float32), np.float32(scale)).astype(np.int8)


def certify_min(low):
    assert low >= MIN_MAGNITUDE, f"an intermediate of magnitude {low} is near the subnormals"


def certify_spread(dec_tc, scale, what=""):
    n = len(np.unique(quantised_cpu(dec_tc, scale)))
    assert n >= MIN_DISTINCT, f"{what}: {n} distinct int8 values, the filter flattens the test"


def session_reference(ps, scale, x_tc, sos, h, q, T):
    """(int8 [C][Ld], rows [W][N]) of one session's raw frames [L][C]: filtered from zero state, then
    support_decim.session_reference."""
    return sd.session_reference(ps, scale, filtered(x_tc, sos), h, q, T)


@functools.lru_cache(maxsize=None)
def reference(C, T, N, q, K):
    """(sets, taps, sos, qd [S] arrays [C][Ld], rows [S] arrays [W][N]) of support_decim.frames(C, T,
    q, K), every session under its own set and SCALES."""
    sets, h = sb.sets(C, T, N), sd.taps(K, 11)
    sos, y, _ = filtered_frames(C, T, q, K)
    both = [sd.session_reference(sets[s], SCALES[s], y[i], h, q, T) for i, s in enumerate(SETS)]
    return sets, h, sos, [b[0] for b in both], [b[1] for b in both]


# ---- the other cases of the GPU tests, certified in tests/test_prefilter_cpu.py -------------------------
def hook_cases():
    """(M, R, n, x [n][R], sos, state [M][2][R]) for M in 1, 3, 8, R in 1, 22, 64 and n in 1, 5, 67, from
    a non-zero state of the order of the section's outputs."""
    for m in (1, 3, 8):
        sos = sections(m, 3)
        for R in (1, 22, 64):
            rng = np.random.default_rng([m, R, 9])
            for n in (1, 5, 67):
                yield m, R, n, sd.inputs(rng, (n, R)), sos, sd.inputs(rng, (m, 2, R)) * np.float32(2.0**-6)


class Case:
    """A bag of a case's inputs; sessions: (raw frames [L][C] of one session, its scale, taps, q), what
    the session's reference is made of."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


INT32_MIN = -2**31


@functools.lru_cache(maxsize=None)
def each_case():
    """An each-group at 8 x 64 under (q, K) = (2, 7): support_decim_each's ragged schedule (counts of 0
    and one-frame packets among them), once as it is (the replayed graph's) and once with six counts
    replaced by -1, n_raw_max + 1 and INT32_MIN, which consume nothing."""
    import support_decim_each as sde

    (C, T, N), (q, K) = sb.GEOMETRIES[0], (2, 7)
    n_max, good = sde.schedule(T, q, K)
    counts = np.array(good, np.int64)
    ticks = len(n_max)
    bad = {(3, 1): -1, (7, 3): n_max[7] + 1, (ticks // 3, 0): INT32_MIN, (ticks // 2, 4): -1,
           (ticks // 2 + 1, 4): n_max[ticks // 2 + 1] + 1, (ticks - 2, 2): -1}
    fed_good = counts.sum(axis=0)
    fed = fed_good.copy()
    for (t, s), v in bad.items():
        fed[s] -= counts[t, s]
        counts[t, s] = v
    assert (good == 0).any() and (good == 1).any()
    x, h, sos = sde.frames(C, T, q, K), sd.taps(K, 11), sections(M, SEED)
    sessions = [(x[i][: int(f[i])], SCALES[s], h, q) for f in (fed, fed_good) for i, s in enumerate(SETS)]
    return Case(C=C, T=T, N=N, q=q, K=K, n_max=n_max, good=good, counts=counts, bad=bad, fed=fed, fed_good=fed_good, x=x, h=h,
                sos=sos, sessions=sessions)


@functools.lru_cache(maxsize=None)
def restart_case():
    """The uniform group at 8 x 64 under (3, 33): session RESTART[0] restarts under set RESTART[1] ahead
    of the first push at a raw position off the grid beyond T + 20 decimated samples.  Its reference is
    the session whose frames before the restart were all zero: zero input keeps the states zero."""
    (C, T, N), (q, K) = sb.GEOMETRIES[0], (3, 33)
    ns = sd.schedule(T, q, K)
    pl = sd.plan(T, q, ns)
    i_r, s_r = ss.RESTART
    at = next(i for i, (P, _, d0, *_) in enumerate(pl) if d0 > T + 20 and P % q)
    zeroed = np.array(sd.frames(C, T, q, K)[i_r])
    zeroed[: pl[at][0]] = 0.0
    h, sos = sd.taps(K, 11), sections(M, SEED)
    return Case(C=C, T=T, N=N, q=q, K=K, ns=ns, pl=pl, at=at, i_r=i_r, s_r=s_r, h=h, sos=sos,
                sessions=[(zeroed, SCALES[s_r], h, q)])


@functools.lru_cache(maxsize=None)
def montage_case():
    """Three 19 x 480 sets widened to 64 rows under (2, 7): the unselected electrodes carry NaN and both
    infinities in every chunk; the reference is made of the selected columns alone."""
    T, N, R, q, K = 480, 3, 64, 2, 7
    maps = [[int(c) for c in np.random.default_rng([R, 50 + i]).permutation(R)[:19]] for i in range(3)]
    h, ns, sos = sd.taps(K, 12), sd.schedule(T, q, K), sections(M, SEED)
    rng = np.random.default_rng([R, T, 29])
    x = sd.inputs(rng, (3, sum(ns), R))
    sessions = []
    for i in range(3):
        keep = x[i][:, maps[i]].copy()
        junk = rng.random(x[i].shape)
        x[i][junk < 0.1] = np.nan
        x[i][(junk >= 0.1) & (junk < 0.2)] = -np.inf
        x[i][(junk >= 0.2) & (junk < 0.3)] = np.inf
        x[i][:, maps[i]] = keep
        sessions.append((keep, MONTAGE_SCALES[i], h, q))
    assert all(not np.isfinite(x[i, P: P + n]).all() for i in range(3) for P, n, *_ in sd.plan(T, q, ns))
    return Case(T=T, N=N, R=R, q=q, K=K, maps=maps, h=h, ns=ns, sos=sos, x=x, sessions=sessions)
