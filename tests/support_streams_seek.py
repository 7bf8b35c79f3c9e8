"""What the tests of stream groups far from zero share (tests/test_streams_seek_cpu.py,
tests/test_gpu_streams_seek.py): where the hook mibminet_test_streams_seek (lib.streams_seek) places
each group, and, computed once per case, the reference of every row.

A session seeked to P is the session whose samples before P were all zero.  Its recording x (the
chunks and frames of support_streams, support_decim and support_decim_each as they are) begins at
global sample P, so the window with global onset o >= P is the oracle's on the materialised window
x[:, o - P : o - P + T] (support_streams_at.rows_for).  With a decimator the session's raw frames go
through decimate.sos_filter from zero state and decimate.fir_decimate at phase P mod q (the function
forms q d - pos in int64, so it is handed the phase, not P), and decimated local index j is global
D(P) + j.  The reference is never another stream entry and never built from position 0.

The bases: 2^31 and 2^32, each crossed in the middle of the schedule; a position past 2^53 (what a
double holds), the first at or after 2^53 + 3 * 2^32 + 2^31 + 11 that is no multiple of 4, 16, the
ring or the hop (that number itself is a multiple of the hop, 3); and "top", INT64_MAX - L, from
which the schedule's last push ends exactly at INT64_MAX."""
import functools
from types import SimpleNamespace

import numpy as np

import support_bank as sb
import support_decim as sd
import support_decim_each as sde
import support_features as sf
import support_prefilter as pf
import support_streams as ss
import support_streams_at as sa
import support_streams_each as se
from mibminet import decimate
from support import want, windows_at

SETS, S, HOP, MAX_PUSH = ss.SETS, ss.S, ss.HOP, ss.MAX_PUSH
GEOMETRY, WIDE = sb.GEOMETRIES[0], sb.GEOMETRIES[1]  # 8 x 64 (cap 112) throughout, 19 x 480 once
I63 = 2**63 - 1
BASE = {"2^31": 2**31, "2^32": 2**32, "2^53": 2**53 + 3 * 2**32 + 2**31 + 11, "top": I63}
BASES = tuple(BASE)
CROSSING = ("2^31", "2^32")
DECIM = {"2^32": (3, 33), "2^31": (2, 7)}  # (q, K) of the raw uniform group that crosses the base
EACH_QK = (2, 7)
EACH_53 = 2**53 + 3 * 2**32 + 7            # the third session of an each-group starts at or just after it
LIMIT_AT, CONTROL = 3, 4                   # the session near the limit, and the one that stays at 0
MIN_COMPARED = 20
# the prefilter's sections are support_prefilter.sections(pf.M, SOS_SEED): the first seed of pf.SEED (2),
# 3, ... with which every case here passes tests/test_streams_seek_cpu.py.  2 and 5 leave sessions under
# set 1 of 8 x 64 (two classes) all-zero expected rows, and 2 leaves the session near the raw limit 62
# distinct int8 values; 3, 4, 6, 7 and 8 flatten every session below certify_spread's 64
SOS_SEED = 9


# ---- where a group is placed --------------------------------------------------------------------------
def residues(P, cap, q=0, K=0):
    """{modulus: P mod it} for everything a seek position should be no multiple of: 4 and 16 (the
    kernels' block sizes), the ring and the hop, on the group's own axis; with a decimator these of
    D(P), and of the raw P also q and K - 1 (the phase and the history slot)."""
    d = decimate.raw_decimated(q, P) if q else P
    out = {"4": d % 4, "16": d % 16, "cap": d % cap, "hop": d % HOP}
    if q:
        out.update({"raw 4": P % 4, "raw 16": P % 16, "q": P % q, "K - 1": P % (K - 1)})
    return out


def off_every_grid(P, cap, q=0, K=0, step=1):
    """The first of P, P + step, ... with no zero among residues()."""
    while not all(residues(P, cap, q, K).values()):
        P += step
    return P


def place(base, L, cap, q=0, K=0):
    """(B, P): the base's value and where a group that is fed L samples (raw frames) starts.  A crossing
    base is met about half way, from the nearest position below B - L / 2 that is off every grid; "top"
    has no choice."""
    B = BASE[base]
    if base == "top":
        return B, B - L
    if base in CROSSING:
        return B, off_every_grid(B - L // 2, cap, q, K, -1)
    return B, off_every_grid(B, cap, q, K)


# ---- a. a uniform group ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def uniform_case(base, geometry=GEOMETRY):
    """The group of support_streams' five sessions seeked to P and pushed support_streams.schedule:
    plan is support_streams.plan from P, onsets every onset of the run, first[j] the index of push j's
    first window among them."""
    C, T, N = geometry
    ns, cap = ss.schedule(T), ss.cap(T, MAX_PUSH)
    B, P = place(base, sum(ns), cap)
    plan = ss.plan(T, HOP, ns, pos=P)
    onsets = [o for *_, on in plan for o in on]
    first = np.concatenate([[0], np.cumsum([k for _, _, k, _, _ in plan])]).tolist()
    return SimpleNamespace(base=base, C=C, T=T, N=N, ns=ns, L=sum(ns), cap=cap, B=B, P=P, plan=plan, onsets=onsets,
                           first=first, below=[sum(o < P for o in on) for *_, on in plan])


@functools.lru_cache(maxsize=None)
def uniform_rows(base, geometry=GEOMETRY):
    """(rows [S][W][N], keep [W]): the oracle's rows of every window of the run with onset >= P, each
    session under its own set, and zero rows where keep is False (onset < P: an invalid window)."""
    c = uniform_case(base, geometry)
    keep = np.array([o >= c.P for o in c.onsets])
    rows = np.zeros((S, len(keep), c.N), np.int8)
    for i in range(S):
        rows[i, keep] = sa.rows_for(c.C, c.T, c.N, [(i, SETS[i], o - c.P) for o in c.onsets if o >= c.P])
    rows.setflags(write=False)
    return rows, keep


# ---- b. a restart past 2^32 -------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def restart_case():
    """The 2^32 case of a; session RESTART[0] restarts under set RESTART[1] at R, the first push boundary
    past 2^32 that is no multiple of the hop.  rows: what every push returns; origin [S]."""
    c = uniform_case("2^32")
    i0, new = ss.RESTART
    at = next(j for j, (pos, *_) in enumerate(c.plan) if pos > c.B and pos % HOP)
    R = c.plan[at][0]
    rows, _ = uniform_rows("2^32")
    rows = rows.copy()
    late = [w for w in range(c.first[at], len(c.onsets))]
    for w in late:
        o = c.onsets[w]
        rows[i0, w] = sa.rows_for(c.C, c.T, c.N, [(i0, new, o - c.P)])[0] if o >= R else 0
    origin = [R if i == i0 else c.P for i in range(S)]
    bad = [sum(o < origin[i] for i in range(S) for o in on) for *_, on in c.plan[at:]]
    return SimpleNamespace(case=c, i0=i0, new=new, at=at, R=R, rows=rows, origin=origin, late=late,
                           bad=[S * b for b in c.below[:at]] + bad)


# ---- c. a raw uniform group with a prefilter -----------------------------------------------------------------
def quantised_cpu(dec_tc, scale):
    """int8 [C][Ld]: the quantiser's statement in NumPy (no GPU), as support_decim.two_pass lays it out."""
    return np.ascontiguousarray(pf.quantised_cpu(dec_tc, scale).T)


def rows_from(ps, qd, onsets, D0, T, N):
    """(rows [W][N], keep [W]) of the windows with global onsets `onsets` of the samples qd [C][Ld],
    whose first is global sample D0: the oracle's where the onset is at or past D0, zeros elsewhere."""
    keep = np.array([o >= D0 for o in onsets], bool)
    rows = np.zeros((len(onsets), N), np.int8)
    if keep.any():
        rows[keep] = want(ps, windows_at(qd, [o - D0 for o in onsets if o >= D0], T))
    return rows, keep


@functools.lru_cache(maxsize=None)
def decim_case(base):
    """The uniform group under DECIM[base] with pf.sections(pf.M, SOS_SEED) ahead of the FIR, seeked to
    the raw position P and pushed support_decim.schedule: dec [S] arrays [m][C] float32, the decimated
    samples global D0 .. of every session; low: the smallest non-zero intermediate of the recursion."""
    (C, T, N), (q, K) = GEOMETRY, DECIM[base]
    ns, cap = sd.schedule(T, q, K), ss.cap(T, MAX_PUSH)
    B, P = place(base, sum(ns), cap, q, K)
    plan = sd.plan(T, q, ns, raw=P)
    sos, h = pf.sections(pf.M, SOS_SEED), sd.taps(K, 11)
    y, low = pf.filtered(sd.frames(C, T, q, K), sos, True)
    dec = [decimate.fir_decimate(np.ascontiguousarray(y[i]), h, q, None, P % q)[0] for i in range(S)]
    onsets = [o for *_, on in plan for o in on]
    D0 = decimate.raw_decimated(q, P)
    assert all(len(d) == decimate.raw_decimated(q, P + sum(ns)) - D0 for d in dec)
    return SimpleNamespace(base=base, C=C, T=T, N=N, q=q, K=K, ns=ns, L=sum(ns), cap=cap, B=B, P=P, D0=D0, plan=plan, h=h,
                           sos=sos, low=low, dec=dec, onsets=onsets, below=[sum(o < D0 for o in on) for *_, on in plan])


def decim_rows(c, quantise):
    """(qd [S] arrays [C][Ld], rows [S][W][N], keep [W]) of decim_case c under the quantiser `quantise`
    (float32 [Ld][C], scale) -> int8 [C][Ld]: quantised_cpu here, support_decim.two_pass on the GPU."""
    sets = sb.sets(c.C, c.T, c.N)
    qd = [quantise(c.dec[i], pf.SCALES[s]) for i, s in enumerate(SETS)]
    both = [rows_from(sets[s], qd[i], c.onsets, c.D0, c.T, c.N) for i, s in enumerate(SETS)]
    return qd, np.stack([b[0] for b in both]), both[0][1]


# ---- d, e. each-groups ----------------------------------------------------------------------------------------
def _limit_start(limit, col, n_max, fed_min, cap, q=0, K=0):
    """Where the session near `limit` starts: the highest position from which, fed the counts `col`, it
    takes at least fed_min samples in at least 10 ticks and is then refused in at least 3, a count of 0
    accepted between two of them; off every grid."""
    for c in range(sum(col), fed_min - 1, -1):
        P, pos, ok = limit - c, limit - c, []
        if not all(residues(P, cap, q, K).values()):
            continue
        for m, n in zip(n_max, col):
            ok.append(pos + n <= limit)
            pos += n if ok[-1] else 0
        no = [t for t, v in enumerate(ok) if not v]
        if len(no) >= 3 and no[0] >= 10 and pos - P >= fed_min and any(
                n == 0 and no[0] < t < no[-1] for t, n in enumerate(col)):
            return P
    raise AssertionError("no start near the limit fits the schedule")


def _each_starts(fed, col, n_max, limit, fed_min, cap, q=0, K=0):
    P = [0] * S
    P[0] = off_every_grid(BASE["2^31"] - int(fed[0]) // 2, cap, q, K, -1)
    P[1] = off_every_grid(BASE["2^32"] - int(fed[1]) // 2, cap, q, K, -1)
    P[2] = off_every_grid(EACH_53, cap, q, K)
    P[LIMIT_AT] = _limit_start(limit, col, n_max, fed_min, cap, q, K)
    return P


@functools.lru_cache(maxsize=None)
def each_case():
    """The each-group of support_streams_each.schedule with one count of session LIMIT_AT, three ticks
    before the end, replaced by 0 (the schedule has no 0 for it that late), seeked to 2^31 - a, 2^32 - b
    (each crossed about half way), past 2^53, just below EACH_POS_LIMIT and 0.  walk: the plan of every
    tick from there, refusals recorded."""
    C, T, N = GEOMETRY
    n_max, counts = se.schedule(T)
    counts = np.array(counts)
    counts[len(n_max) - 3, LIMIT_AT] = 0
    counts.setflags(write=False)
    cap = ss.cap(T, MAX_PUSH)
    col = [int(v) for v in counts[:, LIMIT_AT]]
    P = _each_starts(counts.sum(axis=0), col, n_max, se.POS_LIMIT, T + MIN_COMPARED * HOP, cap)
    walk = se.Walk(T, HOP, MAX_PUSH, n_max, counts, start=P, refusals=True)
    return SimpleNamespace(C=C, T=T, N=N, cap=cap, n_max=n_max, counts=counts, P=P, walk=walk, fed=walk.fed)


def each_onsets(T, P, fed):
    """The global onsets of the windows a session at P completes while it is fed `fed` samples."""
    return [w * HOP for w in range(ss.windows_count(T, P, HOP), ss.windows_count(T, P + fed, HOP))]


@functools.lru_cache(maxsize=None)
def each_rows():
    """[S] pairs (rows [W_i][N], keep [W_i]) of each_case: session i's windows in the order its pushes
    return them, the oracle's where the onset is at or past P_i."""
    c = each_case()
    sets, x = sb.sets(c.C, c.T, c.N), ss.chunks(c.C, c.T)
    return [rows_from(sets[s], np.ascontiguousarray(x[i][:, : int(c.fed[i])]), each_onsets(c.T, c.P[i], int(c.fed[i])),
                      c.P[i], c.T, c.N) for i, s in enumerate(SETS)]


@functools.lru_cache(maxsize=None)
def each_raw_case():
    """The each-group under EACH_QK with the prefilter, support_decim_each.schedule as it is, the five
    starts of each_case on the raw axis with EACH_RAW_LIMIT.  dec [S] arrays [m_i][C]: the decimated
    samples global D(P_i) .. of what session i consumes."""
    (C, T, N), (q, K) = GEOMETRY, EACH_QK
    n_max, counts = sde.schedule(T, q, K)
    cap = ss.cap(T, MAX_PUSH)
    col = [int(v) for v in counts[:, LIMIT_AT]]
    P = _each_starts(counts.sum(axis=0), col, n_max, sde.RAW_LIMIT, q * (T + MIN_COMPARED * HOP), cap, q, K)
    walk = sde.Walk(T, q, K, n_max, counts, start=P)
    sos, h, x = pf.sections(pf.M, SOS_SEED), sd.taps(K, 11), sde.frames(C, T, q, K)
    dec, low = [], np.inf
    for i in range(S):
        y, _, lo = decimate.sos_filter(np.ascontiguousarray(x[i][: int(walk.fed[i])]), sos, None, True)
        dec.append(decimate.fir_decimate(y, h, q, None, P[i] % q)[0])
        low = min(low, lo)
    D0 = [decimate.raw_decimated(q, p) for p in P]
    return SimpleNamespace(C=C, T=T, N=N, q=q, K=K, cap=cap, n_max=n_max, counts=counts, P=P, D0=D0, walk=walk, fed=walk.fed,
                           sos=sos, h=h, x=x, dec=dec, low=low)


def each_raw_rows(c, quantise):
    """(qd [S] arrays [C][Ld_i], [S] pairs (rows, keep)) of each_raw_case c under the quantiser."""
    sets = sb.sets(c.C, c.T, c.N)
    qd = [quantise(c.dec[i], pf.SCALES[s]) for i, s in enumerate(SETS)]
    return qd, [rows_from(sets[s], qd[i], each_onsets(c.T, c.D0[i], qd[i].shape[1]), c.D0[i], c.T, c.N)
                for i, s in enumerate(SETS)]


# ---- f. windows at given onsets -------------------------------------------------------------------------------
def at_points(c):
    """The pushes of uniform_case c after which the group is queried: the first that leaves T + 3 samples
    behind P (onsets just below P are still in the ring, and only the origin refuses them), on a crossing
    base the first that takes the position to B + T + 2 or beyond (onsets on both sides of B are in the
    ring), and the last."""
    ends = [pos + n for pos, n, *_ in c.plan]
    out = {next(j for j, e in enumerate(ends) if e >= c.P + c.T + 3), len(ends) - 1}
    if c.base in CROSSING:
        out.add(next(j for j, e in enumerate(ends) if e >= c.B + c.T + 2))
    return sorted(out)


def at_onsets(T, cap, pos, lo):
    """support_streams_at.onsets_at for a session at pos whose samples begin at lo."""
    return sa.onsets_at(T, pos, lo, cap)


def uniform_at_items(c, pos):
    """The valid (session, onset) items asked of uniform_case c at position pos, shuffled."""
    return sa.shuffled([(i, o) for i in range(S) for o in at_onsets(c.T, c.cap, pos, c.P)], [c.T, pos % 2**31])


def far_bad_onsets(T, cap, pos):
    """Invalid onsets, by name, of a session with floor 0 at a position past 2^33 + cap: those of
    support_streams_at.bad_onsets that fit an int64 here, and the newest window's onset 2^32 and 2^33
    lower, which are non-negative and at or below the position, so that only d > cap refuses them."""
    good = pos - T
    out = {"one past the newest": good + 1, "one before the oldest": pos - cap - 1, "-1": -1, "INT64_MIN": -2**63,
           "INT64_MAX": I63, "low 32 bits valid, - 2^32": good - 2**32, "low 32 bits valid, - 2^33": good - 2**33,
           "low 32 bits valid, sign bit": good - 2**63}
    if good + 2**32 <= I63:
        out["low 32 bits valid, + 2^32"] = good + 2**32
    assert all(not sa.valid(o, 0, pos, T, cap) and -2**63 <= o <= I63 for o in out.values())
    assert 0 <= out["low 32 bits valid, - 2^33"] < out["low 32 bits valid, - 2^32"] <= pos
    return out


def each_at_ticks(c):
    """(the ticks of each_case c after which the each-group is queried, the positions [ticks][S] after
    every tick): for each of the two crossing sessions the first tick that takes it to its base + T + 2
    or beyond, then the last tick."""
    w = c.walk
    after = w.pos + np.where(w.ok, w.counts, 0)
    cross = [next(t for t in range(len(c.n_max)) if int(after[t, i]) >= BASE[base] + c.T + 2)
             for i, base in ((0, "2^31"), (1, "2^32"))]
    return cross + [len(c.n_max) - 1], after


def at_reference(C, T, N, items, P, features=False):
    """The oracle's logits [W][N] of the valid (session, global onset) items of sessions that start at
    P[i] (an int: all at the same), each under its own set; with features the pair (logits, feature
    rows [W][16][T64]) of support_features."""
    at = [(i, o - (P if isinstance(P, int) else P[i])) for i, o in items]
    if not features:
        return sa.expected(C, T, N, at)
    sets, x = sb.sets(C, T, N), ss.chunks(C, T)
    both = [sf.features(sets[SETS[i]], windows_at(np.ascontiguousarray(x[i]), [o], T)) for i, o in at]
    return np.concatenate([b[1] for b in both]), np.concatenate([b[0] for b in both])
