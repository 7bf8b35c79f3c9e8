"""The host arithmetic of net_streams_windows_at (csrc/stream_host.hpp: at_item, at_ring, at_span,
check_windows_at) under AddressSanitizer and UndefinedBehaviorSanitizer: tests/stream_at_host_main.cpp,
a program of its own (nothing is loaded into Python), walks the validity predicate the kernel runs per
item, the ring position and the span at positions and onsets around 0, T, cap, the seam, INT64_MIN/MAX
and the each-groups' position limit, holds each to a 128-bit restatement of its own and prints every
value; here each line is compared with the restatement of tests/support_streams_at.py in Python's
unbounded integers, and the argument checks with the order include/mibminet.h documents."""
import support_streams as ss
import support_streams_at as sa
import support_streams_each as se
from mibminet import lib
from support import run_host_program

MAX_ITEMS = 2**31 - 1 - 65535


def _check(group, W, soff, ooff, yoff, boff, no):
    """The documented order: the group, W == 0, W past the limit, NULL pointers, alignment."""
    if not group:
        return lib.NET_ERR_INVALID
    if W == 0:
        return lib.NET_OK
    if W > MAX_ITEMS or no & 7:
        return lib.NET_ERR_INVALID
    if soff % 4 or ooff % 8 or yoff % 4 or (not no & 8 and boff % 4):
        return lib.NET_ERR_INVALID
    return lib.NET_OK


def test_stream_at_host_arithmetic_under_sanitizers(tmp_path):
    out = run_host_program("stream_at_host_main.cpp", [], tmp_path).splitlines()
    assert out[-1].startswith("cases ") and not [l for l in out if l.startswith("FAIL")], out[-5:]
    seen = {"limit": 0, "item": 0, "ring": 0, "span": 0, "check": 0}
    n_valid = low32 = 0
    for line in out[:-1]:
        kind, *rest = line.split()
        seen[kind] += 1
        at = rest.index(":") if ":" in rest else len(rest)
        args, res = [int(v) for v in rest[:at]], [int(v) for v in rest[at + 1:]]
        if kind == "limit":
            assert args == [se.POS_LIMIT, MAX_ITEMS], line
        elif kind == "item":
            o, lo, pos, T, cap = args
            ok = pos >= 0 and sa.valid(o, lo, pos, T, cap)
            assert res == ([1, pos - o, sa.ring_at(o, cap)] if ok else [0, 0, -1]), line
            n_valid += ok
            # an invalid onset that a 32-bit comparison would have passed
            low32 += (not ok) and pos >= 0 and lo == 0 and T <= (pos - o) % 2**32 <= cap
        elif kind == "ring":
            assert res == [0], line
        elif kind == "span":
            T, cap, pos = args
            assert tuple(res) == sa.span(T, cap, pos), line
        else:
            assert res == [_check(*args)], line
    assert int(out[-1].split()[1]) == sum(seen.values()), seen
    assert seen["item"] > 5000 and seen["span"] > 100 and seen["check"] > 50 and seen["ring"] == 9
    assert n_valid > 500 and seen["item"] - n_valid > 2000 and low32 > 100
    assert ss.cap(64, 37) == 112  # the rings walked are the groups' own
