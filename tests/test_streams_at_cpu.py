"""net_streams_windows_at without a GPU: the entries' refusal of a NULL group (every other check needs
a group, and a group a device: tests/stream_at_host_main.cpp walks them), the properties the query
points and onset lists of tests/support_streams_at.py must have, the restated arithmetic on them, and
the certification of the GPU suite's inputs on the C oracle alone: zeros mark an invalid item, so no
expected row may be all zeros; a ring read one sample off must show; and so must a window decoded by
a neighbour's set."""
import ctypes

import numpy as np
import pytest

import support_streams as ss
import support_streams_at as sa
from mibminet import lib


def test_a_null_group_is_refused():
    L = lib.load()
    lo, hi = ctypes.c_int64(-7), ctypes.c_int64(-7)
    assert L.net_streams_at_span(None, ctypes.byref(lo), ctypes.byref(hi)) == lib.NET_ERR_INVALID
    assert (lo.value, hi.value) == (-7, -7)
    buf = (ctypes.c_int64 * 4)()
    p = ctypes.addressof(buf)
    assert L.net_streams_windows_at(None, p, p, 1, p, p, None) == lib.NET_ERR_INVALID
    assert L.net_streams_windows_at(None, None, None, 0, None, None, None) == lib.NET_ERR_INVALID  # before W == 0
    for name in ("net_streams_windows_at", "net_streams_at_span"):
        assert name in lib.PROTOTYPES and name in lib.EXPORTED_SYMBOLS
    assert hasattr(lib.Streams, "windows_at") and hasattr(lib.StreamsEach, "windows_at")
    assert hasattr(lib.Streams, "at_span") and not hasattr(lib.StreamsEach, "at_span")


def test_restatement_on_small_rings():
    """valid() against the definition by enumeration: the window's samples o .. o + T - 1 have all
    arrived and none was overwritten, at every position of rings of a few samples."""
    for T, cap in ((3, 16), (16, 16), (5, 32)):
        for pos in range(0, 3 * cap + 2):
            held = set(range(max(pos - cap, 0), pos))  # the samples the ring holds
            for lo in (0, 4, pos):
                for o in range(-3, pos + 3):
                    there = o >= lo and set(range(o, o + T)) <= held
                    assert sa.valid(o, lo, pos, T, cap) == there, (T, cap, pos, lo, o)
                    if there:
                        assert 0 <= sa.ring_at(o, cap) < cap and sa.ring_at(o, cap) + T <= 2 * cap
            a, b = sa.span(T, cap, pos)
            assert [o for o in range(-3, pos + 3) if sa.valid(o, 0, pos, T, cap)] == list(range(a, b + 1))


@pytest.mark.parametrize("C,T,N", ss.GEOMETRIES)
def test_query_points_and_onsets(C, T, N):
    ns, cap = ss.schedule(T), ss.cap(T, ss.MAX_PUSH)
    pts = sa.points(T)
    pos = [sa.position(T, j) for j in pts]
    assert len(pts) in (3, 4) and T + 3 <= pos[0] < cap and pos[-1] == ss.total(T) >= 2 * cap + 16
    # right after a push that crossed the seam while writing: the newest window wraps, the oldest does not
    cross = sa.crossings(T)
    assert len(cross) == 2 and set(cross) <= set(pts)
    for j in cross:
        p = sa.position(T, j)
        assert (p - ns[j]) % cap + ns[j] > cap and 0 < p % cap < ns[j]
        a, b = sa.span(T, cap, p)
        assert sa.wraps(b, T, cap) and not sa.wraps(a, T, cap)
    assert cap < sa.position(T, cross[0]) < sa.position(T, cross[1])
    kinds = set()
    for p in pos:
        items = sa.uniform_items(T, p)
        a, b = sa.span(T, cap, p)
        for i in range(ss.S):
            on = [o for s, o in items if s == i]
            assert a in on and b in on and all(sa.valid(o, 0, p, T, cap) for o in on)
            if p >= cap:
                assert {o % 16 for o in on} == set(range(16))
            else:
                assert a == 0 and {o % 4 for o in on} == {0, 1, 2, 3}
        assert len(items) > len(set(items))  # one session asked for one window several times
        sets = [ss.SETS[i] for i, _ in items]
        steps = {(x, y) for x, y in zip(sets, sets[1:]) if x != y}
        assert any(x < y for x, y in steps) and any(x > y for x, y in steps) and len(steps) >= 4
        kinds |= {sa.wraps(o, T, cap) for _, o in items}
        assert 24 <= len(items) <= 120
    assert kinds == {True, False}
    bad = sa.bad_onsets(T, cap, pos[-1])
    assert len(set(bad.values())) == len(bad) == 8


def _certify(C, T, N):
    """The first failing condition of a geometry's inputs on the onsets queried, or None."""
    L = ss.total(T)
    asked = sorted({(i, o) for j in sa.points(T) for i, o in sa.uniform_items(T, sa.position(T, j))})
    rows = sa.expected(C, T, N, asked)
    if not rows.any(axis=1).all():
        return f"(i) {int((~rows.any(axis=1)).sum())} all-zero rows"
    near = [(i, o) for i, o in asked if o >= 1 and o + 1 + T <= L]
    at = sa.expected(C, T, N, near)
    off = [sa.expected(C, T, N, [(i, o + d) for i, o in near]) for d in (-1, 1)]
    frac = float(((off[0] != at).any(axis=1) & (off[1] != at).any(axis=1)).mean())
    if len(near) < len(asked) // 2 or frac < 0.5:
        return f"(ii) {frac:.3f} of the onsets differ from both neighbours"
    for i in range(ss.S):
        mine = [(s, o) for s, o in asked if s == i]
        own = sa.expected(C, T, N, mine)
        for j in (i - 1, i + 1):
            if 0 <= j < ss.S and ss.SETS[j] != ss.SETS[i]:
                other = sa.rows_for(C, T, N, [(i, ss.SETS[j], o) for _, o in mine])
                frac = float((other != own).any(axis=1).mean())
                if frac < 0.75:
                    return f"(iii) session {i} under set {ss.SETS[j]}: {frac:.3f} of its windows differ"
    return None


def test_inputs_are_certified():
    """support_streams.SEED passes on the onset lists of this suite, so the chunks are shared."""
    assert sa.SEED == ss.SEED
    fails = {g: _certify(*g) for g in ss.GEOMETRIES}
    assert not {g: f for g, f in fails.items() if f}, fails
