"""The host arithmetic of an each-group's decimator (csrc/stream_host.hpp) under AddressSanitizer and
UndefinedBehaviorSanitizer: tests/decim_each_host_main.cpp, a program of its own (nothing is loaded
into Python), walks plan_each_raw, each_raw_rows, alloc_decim_each and check_push_each_raw at the
edges where a sum, a product or a conversion could wrap, holds each plan to a 128-bit restatement and
prints every value; here each line is compared with a restatement in Python's unbounded integers."""
import support_decim_each as sde
import support_streams as ss
from mibminet import lib
from support import run_host_program

OK, INV = lib.NET_OK, lib.NET_ERR_INVALID
I32 = 2**31
MAX_ITEMS = 2**31 - 1 - 65535


def _push(S, R, hop, mp, q, K, n, scales, xoff, coff, yoff, ooff, woff, boff, no):
    """(rc, the plan or None) as the header documents the checks, in their order."""
    if not 1 <= n <= q * mp:
        return INV, None
    if no & (1 | 2 | 4 | 8):
        return INV, None
    if (yoff % 4 and not no & 4) or coff % 4 or ooff % 4 or (woff % 8 and not no & 16) or (boff % 4 and not no & 32) or xoff % 4:
        return INV, None
    if not scales:
        return INV, None
    n_max = -(-n // q)
    kmax, blocks, keep = sde.each_raw_rows(hop, q, n), (n_max + 15) // 16, min(n, K - 1)
    return OK, [n_max, keep, S * keep * R, kmax, min(hop, 65536), blocks, S * blocks, S * kmax]


def test_each_decimator_host_arithmetic_under_sanitizers(tmp_path):
    out = run_host_program("decim_each_host_main.cpp", [], tmp_path).splitlines()
    assert out[-1].startswith("cases ") and not [l for l in out if l.startswith("FAIL")], out[-5:]
    assert out[0] == f"limit {sde.RAW_LIMIT}"
    seen = {"limit": 0, "plan": 0, "rows": 0, "alloc": 0, "push": 0}
    refused = zero_m = at_limit = off_grid = 0
    for line in out[:-1]:
        kind, *rest = line.split()
        seen[kind] += 1
        if kind == "plan":
            at = rest.index(":")
            (T, hop, mp, q, K, P, cnt, nm), got = [int(v) for v in rest[:at]], [int(v) for v in rest[at + 1:]]
            want = sde.plan_each_raw(T, hop, ss.cap(T, mp), q, K, P, cnt, nm)
            assert got == [int(v) for v in want], (line, want)
            refused += not want[0]
            zero_m += want[0] and cnt > 0 and want[1] == 0
            at_limit += want[0] and cnt > 0 and P + cnt == sde.RAW_LIMIT
            off_grid += want[0] and want[3] > 0 and want[1] > 0
        elif kind == "rows":
            hop, q, n, got = (int(v) for v in rest)
            assert got == sde.each_raw_rows(hop, q, n), line
        elif kind == "alloc":
            (S, R, K), got = [int(v) for v in rest[:3]], [int(v) for v in rest[4:]]
            hist, per = (4 * K + 15) // 16 * 16, 4 * (K - 1) * R
            raw_pos = (hist + S * per + 15) // 16 * 16
            rec = (raw_pos + 8 * S + 15) // 16 * 16
            assert got == [0, hist, per, hist + S * per, raw_pos, rec, rec + 16 * S], line
        elif kind == "push":
            at = rest.index(":")
            args, res = [int(v) for v in rest[:at]], [int(v) for v in rest[at + 1:]]
            rc, plan = _push(*args[:7], bool(args[7]), *args[8:])
            assert res[0] == rc and res[1:] == (plan or []), (line, rc, plan)
    assert int(out[-1].split()[1]) == sum(seen.values()) and min(seen["plan"], seen["rows"], seen["alloc"], seen["push"]) > 40
    assert min(refused, zero_m, at_limit, off_grid) > 10, (refused, zero_m, at_limit, off_grid)
