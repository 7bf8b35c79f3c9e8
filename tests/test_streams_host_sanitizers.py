"""The host arithmetic of a stream group (csrc/stream_host.hpp) under AddressSanitizer and
UndefinedBehaviorSanitizer: tests/stream_host_main.cpp, a program of its own (nothing is loaded into
Python), walks the ring sizes, the windows of a push and the checks of create and push at the edges
where a sum or a product could wrap, and the checks of the hook that places a group at a position,
and prints every value; here each line is compared with the NumPy-free restatement of
tests/support_streams.py in Python's unbounded integers."""
import support_streams as ss
from mibminet import lib
from support import run_host_program

I63, LIMIT = 2**63 - 1, 2**31 - 1 - 65535


def _push(T, S, hop, mp, pos, n, layout, f32, scales, xoff, yoff, boff, nox, noy):
    """(rc, the geometry or None) as the header documents the checks, in their order."""
    if n == 0:
        return lib.NET_OK, None
    k = ss.push_windows(T, hop, pos, n)
    bad = (n > mp or (not f32 and layout not in (0, 1)) or nox or (f32 and xoff % 4) or (f32 and not scales)
           or pos + n > I63 or (k and (noy or yoff % 4)) or boff % 4)
    if bad:
        return lib.NET_ERR_INVALID, None
    cap, W0 = ss.cap(T, mp), ss.windows_count(T, pos, hop)
    first = W0 * hop if k else 0
    blocks = (n + 15) // 16
    return lib.NET_OK, [k, W0, first, min(hop, I63), first % cap, pos % cap, blocks, S * blocks, S * k]


def _seek(group, each, fresh, q, S, have_pos, have_origin, values):
    """check_seek as include/mibminet_testing.h documents the hook's refusals."""
    pos = values[:S] if have_pos else None
    origin = values[S if have_pos else 0:] if have_origin else None
    if not group or pos is None or not fresh or (each and origin is not None):
        return lib.NET_ERR_INVALID
    limit = I63 if not each else I63 - 2**20 if q else I63 - 65536
    if any(p < 0 or p > limit for p in pos) or (not each and len(set(pos)) != 1):
        return lib.NET_ERR_INVALID
    if origin is not None and any(not 0 <= o <= (-(-p // q) if q else p) for o, p in zip(origin, pos)):
        return lib.NET_ERR_INVALID
    return lib.NET_OK


def test_stream_host_arithmetic_under_sanitizers(tmp_path):
    out = run_host_program("stream_host_main.cpp", [], tmp_path).splitlines()
    assert out[-1].startswith("cases ") and not [l for l in out if l.startswith("FAIL")], out[-5:]
    seen = {"cap": 0, "k": 0, "push": 0, "create": 0, "seek": 0}
    seeks = {lib.NET_OK: 0, lib.NET_ERR_INVALID: 0}
    creates = []
    for line in out[:-1]:
        kind, *rest = line.split()
        seen[kind] += 1
        if kind == "cap":
            T, mp, got = (int(v) for v in rest)
            assert got == ss.cap(T, mp), line
        elif kind == "k":
            T, hop, pos, n, got = (int(v) for v in rest)
            assert got == ss.push_windows(T, hop, pos, n), line
        elif kind == "push":
            at = rest.index(":")
            args, res = [int(v) for v in rest[:at]], [int(v) for v in rest[at + 1:]]
            rc, geom = _push(*args[:7], *(bool(v) for v in args[7:9]), *args[9:12], *(bool(v) for v in args[12:]))
            assert res[0] == rc and res[1:] == (geom or []), (line, rc, geom)
        elif kind == "seek":
            at = rest.index(":")
            a = [int(v) for v in rest[:at]]
            rc = _seek(*(bool(v) for v in a[:3]), a[3], a[4], bool(a[5]), bool(a[6]), a[7:])
            assert int(rest[at + 1]) == rc, (line, rc)
            seeks[rc] += 1
        else:
            creates.append(([int(v) for v in rest[:8]], int(rest[9])))
    assert int(out[-1].split()[1]) == sum(seen.values()) and min(seen.values()) > 20, seen
    assert min(seeks.values()) > 100, seeks
    # create: the lists are the program's own, so the set check is restated on what it printed
    for (bank, n_sets, n_list, S, hop, mp, device, has_out), got in creates:
        base = bank and has_out and S > 0 and hop > 0 and 1 <= mp <= 65536 and S * mp <= LIMIT and 0 <= device < 64
        if not base:
            assert got == lib.NET_ERR_INVALID, (bank, n_sets, n_list, S, hop, mp, device, has_out)
        elif n_list < 0:
            assert got == lib.NET_OK, (S, hop, mp, device)
    # the four lists of five at S 5, hop 3, max_push 37, in the program's order: good, negative, past
    # the bank, INT32_MIN; then the good list on banks of four and of three sets
    five = [got for (bank, n_sets, n_list, S, hop, mp, device, has_out), got in creates
            if bank and has_out and (S, hop, mp, device, n_list) == (5, 3, 37, 0, 5)]
    assert five == [lib.NET_OK] + [lib.NET_ERR_INVALID] * 3 + [lib.NET_OK, lib.NET_ERR_INVALID], five
