"""What tests/support_streams_seek.py promises of every case tests/test_gpu_streams_seek.py uses,
asserted on the reference alone.  No GPU.

Two of the issue's own figures cannot be met as stated and are held to what can be: the position past
2^53 and the each-group's 2^53 + 3 * 2^32 + 7 are both multiples of the hop (3), so each case starts at
the first position at or after its figure that is off every grid; and INT64_MAX - L at 8 x 64 (L = 339)
is a multiple of 4, which a group whose last push must end at INT64_MAX cannot avoid, so the top base
is held to the other residues.  The control session of the plain each-group is support_streams_each's
SLOW, which is fed 90 samples: it has 9 windows, all of them compared."""
import numpy as np
import pytest

import support_decim_each as sde
import support_prefilter as pf
import support_streams as ss
import support_streams_at as sa
import support_streams_each as se
import support_streams_seek as sk

S, HOP, MAX_PUSH = sk.S, sk.HOP, sk.MAX_PUSH
LEFT_OUT = -(-(sk.GEOMETRY[1] - 1) // HOP)  # ceil((T - 1) / hop) at 8 x 64


def off_grids(P, cap, q=0, K=0, but=()):
    zero = [m for m, r in sk.residues(P, cap, q, K).items() if r == 0]
    assert zero == list(but), (P, zero)


def no_zero_row(rows, keep, what):
    assert rows[..., keep, :].any(axis=-1).all(), f"{what}: a compared window's expected row is all zeros"
    assert not rows[..., ~keep, :].any()


CASES = [(b, sk.GEOMETRY) for b in sk.BASES] + [("2^32", sk.WIDE)]


@pytest.mark.parametrize("base,geometry", CASES)
def test_uniform_cases(base, geometry):
    c = sk.uniform_case(base, geometry)
    T = c.T
    assert c.cap == ss.cap(T, MAX_PUSH) and (geometry != sk.GEOMETRY or c.cap == 112)
    off_grids(c.P, c.cap, but=("4",) if base == "top" else ())
    assert c.P + c.L <= sk.I63 and (base != "top" or c.P + c.L == sk.I63 == c.B)
    assert base != "2^53" or (c.B <= c.P <= c.B + 16 and float(c.P) != c.P)
    rows, keep = sk.uniform_rows(base, geometry)
    no_zero_row(rows, keep, base)
    # the windows left out are exactly those that start before the seek: at most ceil((T - 1) / hop)
    assert (~keep).sum() == sum(c.below) == sum(1 for o in c.onsets if o < c.P) <= -(-(T - 1) // HOP)
    assert (~keep).sum() > 0 and keep.sum() >= sk.MIN_COMPARED
    assert c.onsets == sorted(c.onsets) and all(o % HOP == 0 and o + T <= c.P + c.L for o in c.onsets)
    if base in sk.CROSSING:
        assert abs((c.B - c.P) - c.L // 2) <= 16
        assert any(pos < c.B <= pos + n for pos, n, *_ in c.plan)
        assert any(o < c.B < o + T for o, k in zip(c.onsets, keep) if k)
    points = sk.at_points(c)
    ends = [pos + n for pos, n, *_ in c.plan]
    assert len(points) == (3 if base in sk.CROSSING else 2)
    # the early point: onsets just below P are in the ring and complete, so only the origin refuses them
    early = ends[points[0]]
    assert all(sa.valid(o, 0, early, T, c.cap) and not sa.valid(o, c.P, early, T, c.cap) for o in (c.P - 1, c.P - 2))
    for j in points:
        items = sk.uniform_at_items(c, ends[j])
        assert len({i for i, _ in items}) == S and all(sa.valid(o, c.P, ends[j], T, c.cap) for _, o in items)
        assert {o % 4 for _, o in items} == {0, 1, 2, 3}
    if base in sk.CROSSING:
        pos = ends[points[1]]
        on = [o for _, o in sk.uniform_at_items(c, pos)]
        assert any(o < c.B <= pos for o in on) and any(o >= c.B for o in on)
    if geometry == sk.GEOMETRY:
        at = sk.at_reference(c.C, T, c.N, sk.uniform_at_items(c, ends[points[-1]]), c.P)
        no_zero_row(at, np.ones(len(at), bool), "windows_at")


def test_far_bad_onsets():
    for base in ("2^53", "top"):
        c = sk.uniform_case(base)
        bad = sk.far_bad_onsets(c.T, c.cap, c.P + c.L)
        assert len(bad) == (9 if base == "2^53" else 8)
        for name in ("low 32 bits valid, - 2^32", "low 32 bits valid, - 2^33"):
            o, pos = bad[name], c.P + c.L
            assert 0 <= o <= pos and (pos - o) % 2**32 == c.T  # a d cut to 32 bits would read T: valid


def test_restart_case():
    r = sk.restart_case()
    c = r.case
    assert c.P < 2**32 < r.R == c.plan[r.at][0] and r.R % HOP and r.at > 0
    before = [o for o, k in zip(c.onsets[: c.first[r.at]], sk.uniform_rows("2^32")[1][: c.first[r.at]]) if k and o < 2**32]
    assert before and r.R % 2**32 < min(o % 2**32 for o in before)
    zero = [w for w in r.late if c.onsets[w] < r.R]
    live = [w for w in r.late if c.onsets[w] >= r.R]
    assert len(zero) >= 10 and len(live) >= 10 and sum(r.bad[r.at:]) == len(zero)
    assert not r.rows[r.i0, zero].any() and r.rows[r.i0, live].any(axis=1).all()
    own = sk.uniform_rows("2^32")[0]
    assert (r.rows[r.i0, live] != own[r.i0, live]).any(axis=1).mean() >= 0.75  # the new set shows
    others = [i for i in range(S) if i != r.i0]
    assert np.array_equal(r.rows[others], own[others])


@pytest.mark.parametrize("base", list(sk.DECIM))
def test_decim_cases(base):
    c = sk.decim_case(base)
    assert (c.q, c.K) == sk.DECIM[base] and c.D0 == -(-c.P // c.q)
    off_grids(c.P, c.cap, c.q, c.K)
    assert abs((c.B - c.P) - c.L // 2) <= 64 and any(P < c.B <= P + n for P, n, *_ in c.plan)
    pf.certify_min(c.low)
    for i, s in enumerate(sk.SETS):
        pf.certify_spread(c.dec[i], pf.SCALES[s], f"session {i}")
    qd, rows, keep = sk.decim_rows(c, sk.quantised_cpu)
    no_zero_row(rows, keep, base)
    assert (~keep).sum() == sum(c.below) <= LEFT_OUT and (~keep).sum() > 0 and keep.sum() >= sk.MIN_COMPARED
    # a compared window whose raw frames lie on both sides of the base
    assert any(c.q * o < c.B < c.q * (o + c.T) for o, k in zip(c.onsets, keep) if k)


def each_checks(c, rows, limit, q=0, K=0):
    w = c.walk
    for i in range(4):
        off_grids(c.P[i], c.cap, q, K)
    assert c.P[sk.CONTROL] == 0 and sk.EACH_53 <= c.P[2] <= sk.EACH_53 + 16 and float(c.P[2]) != c.P[2]
    for i, base in ((0, "2^31"), (1, "2^32")):  # crossed mid-schedule, in the middle of a tick
        B = sk.BASE[base]
        assert c.P[i] < B < c.P[i] + int(c.fed[i]) and abs((B - c.P[i]) - int(c.fed[i]) // 2) <= 64 * max(q, 1)
        assert any(int(w_pos) < B < int(w_pos) + int(n) for w_pos, n in zip((w.P if q else w.pos)[:, i], c.counts[:, i]))
    # the session near the limit: accepted in ten ticks and more, then refused at least three times
    # with an accepted count of 0 in between; every other count of the schedule is accepted
    ok = w.ok[:, sk.LIMIT_AT].astype(bool)
    no = np.flatnonzero(~ok)
    others = [i for i in range(S) if i != sk.LIMIT_AT]
    assert w.ok[:, others].all() and len(no) >= 3 and no[0] >= 10
    assert any(c.counts[t, sk.LIMIT_AT] == 0 and ok[t] for t in range(no[0] + 1, no[-1]))
    assert c.P[sk.LIMIT_AT] + int(c.fed[sk.LIMIT_AT]) <= limit < c.P[sk.LIMIT_AT] + int(c.counts[no[0], sk.LIMIT_AT]) + int(
        (w.P if q else w.pos)[no[0], sk.LIMIT_AT] - c.P[sk.LIMIT_AT])
    for i, (r, keep) in enumerate(rows):
        no_zero_row(r, keep, f"session {i}")
        assert (~keep).sum() <= LEFT_OUT
        if i == sk.CONTROL:
            assert keep.all() and len(keep) > 0  # today's rows, all of them
        else:
            assert (~keep).sum() > 0 and keep.sum() >= sk.MIN_COMPARED, (i, keep.sum())


def test_each_case():
    c = sk.each_case()
    n_max, counts = se.schedule(c.T)
    changed = np.argwhere(c.counts != counts)
    assert changed.tolist() == [[len(n_max) - 3, sk.LIMIT_AT]] and c.n_max == n_max
    rows = sk.each_rows()
    each_checks(c, rows, se.POS_LIMIT)
    own = se.expected(ss.table(c.C, c.T, c.N), [0, 0, 0, 0, int(c.fed[sk.CONTROL])], c.T)[sk.CONTROL]
    assert np.array_equal(rows[sk.CONTROL][0], own)
    ticks, after = sk.each_at_ticks(c)
    assert len(ticks) == 3 and ticks[2] == len(c.n_max) - 1
    for t, (i, base) in zip(ticks, ((0, "2^31"), (1, "2^32"))):
        pos, B = int(after[t, i]), sk.BASE[base]
        on = sk.at_onsets(c.T, c.cap, pos, c.P[i])
        assert any(o < B <= pos for o in on) and any(o >= B for o in on)
    for i in (2, sk.LIMIT_AT):
        sk.far_bad_onsets(c.T, c.cap, c.P[i] + int(c.fed[i]))


def test_each_raw_case():
    c = sk.each_raw_case()
    assert (c.n_max, c.counts.tolist()) == (sde.schedule(c.T, c.q, c.K)[0], sde.schedule(c.T, c.q, c.K)[1].tolist())
    pf.certify_min(c.low)
    for i, s in enumerate(sk.SETS):
        pf.certify_spread(c.dec[i], pf.SCALES[s], f"session {i}")
    qd, rows = sk.each_raw_rows(c, sk.quantised_cpu)
    each_checks(c, rows, sde.RAW_LIMIT, c.q, c.K)
