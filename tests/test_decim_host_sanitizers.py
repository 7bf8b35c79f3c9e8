"""The host arithmetic of a stream group's decimator (csrc/stream_host.hpp) under AddressSanitizer
and UndefinedBehaviorSanitizer: tests/decim_host_main.cpp, a program of its own (nothing is loaded
into Python), walks raw_samples, check_set_decimator, check_push_raw, the allocation and the
history's slots at the edges where a sum or a product could wrap, and prints every value; here each
line is compared with a restatement in Python's unbounded integers."""
import support_streams as ss
from mibminet import lib
from support import run_host_program

I63, U64 = 2**63 - 1, 2**64 - 1
OK, INV, UNS = lib.NET_OK, lib.NET_ERR_INVALID, lib.NET_ERR_UNSUPPORTED


def _D(q, P):
    return -(-P // q)


def _m(q, P, n):
    return 0 if q == 0 or P + n > U64 else _D(q, P + n) - _D(q, P)


def _set(group, each, scales, have, pushed, q, K, what):
    if not group:
        return INV
    if each:
        return UNS
    bad = have or pushed or not 1 <= q <= 16 or not 1 <= K <= 128 or what != 0 or not scales
    return INV if bad else OK


def _raw(T, S, R, hop, mp, q, K, P, n, scales, xoff, yoff, boff, nox, noy):
    """(rc, the plan or None) as the header documents the checks, in their order."""
    if n == 0:
        return OK, None
    if n > q * mp or nox or xoff % 4 or not scales or P + n > I63:
        return INV, None
    m, d0 = _m(q, P, n), _D(q, P)
    k = ss.push_windows(T, hop, d0, m)
    if (k and (noy or yoff % 4)) or boff % 4:
        return INV, None
    keep = min(n, K - 1)
    plan = [m, d0, q * d0 - P, P % (K - 1) if K > 1 else 0, keep, S * keep * R]
    if m:
        cap, W0 = ss.cap(T, mp), ss.windows_count(T, d0, hop)
        first = W0 * hop if k else 0
        blocks = (m + 15) // 16
        plan += [k, W0, first, first % cap, d0 % cap, blocks, S * blocks, S * k]
    return OK, plan


def test_decimator_host_arithmetic_under_sanitizers(tmp_path):
    out = run_host_program("decim_host_main.cpp", [], tmp_path).splitlines()
    assert out[-1].startswith("cases ") and not [l for l in out if l.startswith("FAIL")], out[-5:]
    seen = {"m": 0, "set": 0, "alloc": 0, "slot": 0, "raw": 0}
    zero_m = at_limit = past_limit = edge = 0
    for line in out[:-1]:
        kind, *rest = line.split()
        seen[kind] += 1
        if kind == "m":
            q, P, n, got = (int(v) for v in rest)
            assert got == _m(q, P, n), line
        elif kind == "set":
            args, got = [int(v) for v in rest[:8]], int(rest[9])
            assert got == _set(*(bool(v) for v in args[:5]), *args[5:]), line
        elif kind == "alloc":
            (S, R, K), got = [int(v) for v in rest[:3]], [int(v) for v in rest[4:]]
            hist, per = (4 * K + 15) // 16 * 16, 4 * (K - 1) * R
            assert got == [0, hist, per, hist + S * per], line
        elif kind == "slot":
            a, K, got = (int(v) for v in rest)
            assert got == a % (K - 1), line
        else:
            at = rest.index(":")
            args, res = [int(v) for v in rest[:at]], [int(v) for v in rest[at + 1:]]
            rc, plan = _raw(*args[:9], bool(args[9]), *args[10:13], *(bool(v) for v in args[13:]))
            assert res[0] == rc and res[1:] == (plan or []), (line, rc, plan)
            mp, q, P, n = args[4], args[5], args[7], args[8]
            zero_m += rc == OK and n > 0 and plan[0] == 0
            at_limit += rc == OK and n == q * mp
            past_limit += n == q * mp + 1 and rc == INV
            edge += rc == OK and n > 0 and P + n == I63
    assert int(out[-1].split()[1]) == sum(seen.values()) and min(seen.values()) > 20, seen
    assert min(zero_m, at_limit, past_limit, edge) > 10, (zero_m, at_limit, past_limit, edge)
