"""The loader's host arithmetic under AddressSanitizer and UndefinedBehaviorSanitizer (no GPU, and
nothing loaded into Python): tests/host_arith_main.cpp includes only HIP-free headers
(csrc/requant_host.hpp, csrc/params_host.hpp, csrc/images.hpp), is built here with the host C++
compiler and run as an ordinary child process.  It loads the blobs of the sets
tests/test_images_cpu.py pins, plus one whose layer-1 offset sits at the int32 end, through the
loader's own parse_blob and build_set, normally and on the general path, and prints the verdict and
the digests of both images, held here to the pinned ones; runs the header's dimension cases through
both parsers; sweeps gen::carve_of over every supported geometry; and sweeps choose_reciprocal,
choose_floor_form and xdiv over the factor classes against 64-bit division.
tests/entry_host_main.cpp does the same for the entries' argument arithmetic
(csrc/entry_host.hpp).  Any sanitizer report, failed check or compile error fails the test."""
from mibminet.params import ParamSet, dot_ranges
from support import ROWS, run_host_program

I32_MAX = 2 ** 31 - 1


def _int32_end_set():
    """Layer-1 filter 5 with offset INT32_MAX - dot_range.hi (the numerator reaches INT32_MAX) and a
    factor that keeps the output step 99 -> 100 reachable, so the filter is not folded: exact
    division, first unproven requant (1, 5).  offset + FMAGIC_I would leave int32."""
    ps = ParamSet.synthetic(seed=2)
    lo, hi = dot_ranges(ps)[0][5]
    ps.l1_offset[5] = I32_MAX - hi
    ps.l1_factor[5] = (I32_MAX - (hi - lo) // 2) // 100
    return ps


def test_host_arithmetic_runs_clean_under_sanitizers(tmp_path):
    sets = [row[0]() for row in ROWS] + [_int32_end_set()]
    paths = []
    for i, ps in enumerate(sets):
        paths.append(str(tmp_path / f"set{i}.blob"))
        with open(paths[-1], "wb") as f:
            f.write(ps.to_blob())
    stdout = run_host_program("host_arith_main.cpp", paths, tmp_path)
    lines = [ln.split() for ln in stdout.splitlines() if ln.startswith("set ")]
    assert [(ln[1], ln[2]) for ln in lines] == [(p, mode) for p in paths for mode in ("normal", "general")]
    verdict = lambda ln: tuple(int(v) for v in ln[3:8])  # noqa: E731  rc, xr, layer, filter, folded
    digests = lambda ln: (int(ln[8], 16), int(ln[9], 16))  # noqa: E731  kernels' image, window image
    # the verdict as net_params_info reports it: a filter is named for the compiled geometries only
    for (_, normal, general, _, first, exact, folded), n, g in zip(ROWS, lines[0::2], lines[1::2]):
        assert verdict(n) == (0, int(exact)) + first + (folded,), n
        assert verdict(g) == (0, int(exact), 0, -1, folded), g
        assert digests(n) == (normal, general), n
        assert digests(g) == (general, general), g
    n, g = lines[-2:]  # the int32-end set (no pinned digest): one window image, the general path's own
    assert verdict(n) == (0, 1, 1, 5, 0) and verdict(g) == (0, 1, 0, -1, 0)
    assert digests(g) == (digests(n)[1],) * 2 and digests(n)[0] != digests(n)[1]
    # every header case refused with a code by both parsers; every carve of the supported domain
    # (C 1..64, T 64..4096, N 1..16, four layouts) inside the LDS, the largest filling it exactly
    assert "dims 4" in stdout.splitlines()
    assert f"carve {64 * 4033 * 16 * 4} max {160 * 1024}" in stdout.splitlines()
    assert "sweep 125 factors" in stdout


def test_entry_arithmetic_runs_clean_under_sanitizers(tmp_path):
    """tests/entry_host_main.cpp includes only csrc/entry_host.hpp: check_windows, check_epochs,
    windows_multi and check_scale at the documented edges of include/mibminet.h, each result held to
    the header's rule restated in 128-bit arithmetic, the lists in arrays of exactly their size."""
    assert run_host_program("entry_host_main.cpp", [], tmp_path).splitlines() == ["cases 4730"]
