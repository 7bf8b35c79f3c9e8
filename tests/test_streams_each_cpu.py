"""Each-groups without a GPU: the count schedules of tests/support_streams_each.py are certified (the
properties below are conditions the inputs of tests/test_gpu_streams_each.py must meet; the reference
alone meets them), and the host arithmetic of csrc/stream_host.hpp (plan_each, the function one
thread of k_stream_plan runs per session and push; each_rows; check_push_each; alloc_each) runs as a
program of its own, tests/stream_each_host_main.cpp, under AddressSanitizer and
UndefinedBehaviorSanitizer: nothing is loaded into Python, and every line it prints is compared with
the restatement in Python's unbounded integers."""
import numpy as np
import pytest

import support_streams as ss
import support_streams_each as se
from mibminet import lib
from support import run_host_program
from test_lib_cpu import test_prototype_table_matches_header as prototype_table_check

FAST = [s for s in range(se.S) if s != se.SLOW]


@pytest.mark.parametrize("C,T,N", ss.GEOMETRIES)
def test_schedule_is_certified(C, T, N):
    n_max, counts = se.schedule(T)
    w = se.walk(T)
    cap, ticks = w.cap, len(n_max)
    assert counts.shape == (ticks, se.S) and cap == ss.cap(T, se.MAX_PUSH)
    assert all(1 <= m <= se.MAX_PUSH for m in n_max)
    assert (counts >= 0).all() and (counts <= np.array(n_max)[:, None]).all()
    # the sessions consume prefixes of the certified chunks
    assert w.fed.max() <= ss.total(T) and (w.fed == counts.sum(axis=0)).all()
    # every session but one wraps its ring at least twice; the slow one never wraps, and has windows
    assert all(w.fed[s] >= 2 * cap for s in FAST)
    assert T + 4 < w.fed[se.SLOW] < cap
    # one session is always at n_max
    assert (counts[:, se.FULL] == np.array(n_max)).all()
    # one session has at least three consecutive zero counts after its first window
    first = int(np.flatnonzero(w.k[:, se.SLOW] > 0)[0])
    z = counts[first + 1:, se.SLOW] == 0
    assert any(z[i: i + 3].all() for i in range(len(z) - 2))
    assert counts[first + 1:, se.SLOW].sum() > 0 and w.k[first + 1:, se.SLOW].sum() > 0  # and goes on
    # counts hit every residue mod 16, write positions every residue mod 4 in every session
    assert set((counts % 16).ravel().tolist()) == set(range(16))
    for s in range(se.S):
        assert set((w.p0[counts[:, s] > 0, s] % 4).tolist()) == {0, 1, 2, 3}, s
    # at least two pushes per fast session cross the seam while writing
    for s in FAST:
        assert int((w.p0[:, s] + counts[:, s] > cap).sum()) >= 2, s
    # in some tick one session gets kmax rows while another gets none
    kmax = np.array([se.each_rows(se.HOP, m) for m in n_max])
    assert ((w.k == kmax[:, None]).any(axis=1) & (w.k == 0).any(axis=1)).any()
    assert (w.k <= kmax[:, None]).all()
    # no two sessions have equal positions after tick 3
    for t in range(4, ticks):
        assert len(set(w.pos[t].tolist())) == se.S, t
    after = w.fed.tolist()
    assert len(set(after)) == se.S
    # the rows add up to each session's windows
    for s in range(se.S):
        assert w.k[:, s].sum() == ss.windows_count(T, int(w.fed[s]), se.HOP)
        on = w.k[:, s] > 0
        assert (w.at0[on, s] == (w.W0[on, s] * se.HOP) % cap).all()


def test_prototype_table_holds_the_new_entries():
    """tests/test_lib_cpu.py's check of lib.PROTOTYPES against both headers, with the each-group
    entries in it."""
    for name in ("net_streams_create_each", "net_streams_each_rows", "net_streams_push_each", "net_streams_push_each_f32",
                 "net_streams_positions"):
        assert name in lib.PROTOTYPES and name in lib.EXPORTED_SYMBOLS
    prototype_table_check()
    assert [int(lib.load().net_streams_each_rows(h, n)) for h, n in ((3, 37), (1, 37), (50, 37), (0, 37), (3, 0), (3, 65537))] \
        == [13, 37, 1, 0, 0, 0]


def _check_push(S, hop, mp, n_max, layout, f32, scales, xoff, coff, yoff, ooff, woff, boff, no):
    """(rc, the geometry or None) as include/mibminet.h documents the checks, in their order."""
    null = [bool(no & b) for b in (1, 2, 4, 8, 16, 32)]
    bad = (not 1 <= n_max <= mp or (not f32 and layout not in (0, 1)) or any(null[:4])
           or (not null[2] and yoff % 4) or (not null[1] and coff % 4) or (not null[3] and ooff % 4)
           or (not null[4] and woff % 8) or (not null[5] and boff % 4) or (f32 and xoff % 4) or (f32 and not scales))
    if bad:
        return lib.NET_ERR_INVALID, None
    kmax, blocks = se.each_rows(hop, n_max), (n_max + 15) // 16
    return lib.NET_OK, [kmax, min(hop, 65536), blocks, S * blocks, S * kmax]


def test_each_host_arithmetic_under_sanitizers(tmp_path):
    out = run_host_program("stream_each_host_main.cpp", [], tmp_path).splitlines()
    assert out[-1].startswith("cases ") and not [l for l in out if l.startswith("FAIL")], out[-5:]
    seen = {"limit": 0, "plan": 0, "rows": 0, "push": 0, "alloc": 0}
    refused = limit = 0
    for line in out[:-1]:
        kind, *rest = line.split()
        seen[kind] += 1
        if kind == "limit":
            assert int(rest[0]) == se.POS_LIMIT
        elif kind == "plan":
            at = rest.index(":")
            (T, hop, mp, pos, cnt, n_max), got = [int(v) for v in rest[:at]], [int(v) for v in rest[at + 1:]]
            want = se.plan_each(T, hop, ss.cap(T, mp), pos, cnt, n_max)
            assert got == [int(v) for v in want], (line, want)
            refused += not want[0]
            limit += 0 <= cnt <= n_max and not want[0]
        elif kind == "rows":
            hop, n, got = (int(v) for v in rest)
            assert got == se.each_rows(hop, n), line
        elif kind == "push":
            at = rest.index(":")
            args, res = [int(v) for v in rest[:at]], [int(v) for v in rest[at + 1:]]
            rc, geom = _check_push(*args[:5], *(bool(v) for v in args[5:7]), *args[7:])
            assert res[0] == rc and res[1:] == (geom or []), (line, rc, geom)
        else:
            at = rest.index(":")
            (S, cap), got = [int(v) for v in rest[:at]], [int(v) for v in rest[at + 1:]]
            ring, origin = 32 * cap, S * 32 * cap
            base = origin + 12 * S
            plan = (base + 15) // 16 * 16
            assert got == [ring, origin, origin + 8 * S, base, plan, plan + 16 * S, plan + 24 * S], line
            assert origin % 8 == 0 and plan % 16 == 0 and (plan + 16 * S) % 8 == 0
    assert int(out[-1].split()[1]) == sum(seen.values()) and min(seen.values()) >= 1, seen
    assert seen["plan"] > 5000 and seen["push"] > 40 and seen["rows"] == 100 and seen["alloc"] == 16
    assert refused > 1000 and limit > 100  # counts outside 0 .. n_max, and counts the position limit refuses
