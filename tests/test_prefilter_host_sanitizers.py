"""The host side of a stream group's prefilter (csrc/stream_host.hpp) under AddressSanitizer and
UndefinedBehaviorSanitizer: tests/prefilter_host_main.cpp, a program of its own (nothing is loaded into
Python), walks check_set_prefilter through every refusal in the documented order and alloc_prefilter
over the corners of S, R, M, q and max_push, holds both to restatements of its own (the allocation's
in 128 bits) and prints every case; here each line is compared with a restatement in Python's
unbounded integers."""
from mibminet import lib
from support import run_host_program

OK, INV = lib.NET_OK, lib.NET_ERR_INVALID
MAX_ITEMS = 2**31 - 1 - 65535


def _set(group, decim, have, pushed, M, what):
    """The documented order: a NULL group; a group without a decimator, with a prefilter or pushed to;
    M outside 1 .. 8; NULL sos; a coefficient that is not finite."""
    if not group:
        return INV
    if not decim or have or pushed:
        return INV
    if not 1 <= M <= 8:
        return INV
    return INV if what else OK


def test_prefilter_host_arithmetic_under_sanitizers(tmp_path):
    out = run_host_program("prefilter_host_main.cpp", [], tmp_path).splitlines()
    assert out[-1].startswith("cases ") and not [l for l in out if l.startswith("FAIL")], out[-5:]
    assert out[0] == "max 8"
    seen = {"max": 0, "set": 0, "alloc": 0}
    accepted = at_limit = 0
    for line in out[:-1]:
        kind, *rest = line.split()
        seen[kind] += 1
        if kind == "set":
            got = int(rest[-1])
            assert got == _set(*[int(v) for v in rest[:6]]), line
            accepted += got == OK
        elif kind == "alloc":
            (S, R, M, q, mp), got = [int(v) for v in rest[:5]], [int(v) for v in rest[6:]]
            per_state, per_scratch = 8 * M * R, 4 * q * mp * R
            scratch = (S * per_state + 255) // 256 * 256
            assert got == [0, per_state, scratch, per_scratch, scratch + S * per_scratch], line
            assert got[4] < 2**64
            at_limit += S * mp > MAX_ITEMS - mp
    assert int(out[-1].split()[1]) == sum(seen.values()) and seen["set"] > 60 and seen["alloc"] > 400
    assert accepted >= 5 and at_limit >= 100
    # the size the header documents: 1,024 sessions of 22 electrodes at q = 4 and max_push = 16
    assert 1024 * 4 * 4 * 16 * 22 == 5_767_168
