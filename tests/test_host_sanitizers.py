"""The loader's host arithmetic under AddressSanitizer and UndefinedBehaviorSanitizer (no GPU, and
nothing loaded into Python): tests/host_arith_main.cpp includes only the HIP-free headers
csrc/requant_host.hpp and csrc/params_host.hpp, is built here with the host C++ compiler and run as
an ordinary child process.  It parses the blobs of the sets tests/test_images_cpu.py pins, plus one
whose layer-1 offset sits at the int32 end, runs range check, folding and requant plan on each, and
sweeps choose_reciprocal, choose_floor_form and xdiv over the factor classes against 64-bit
division.  Any sanitizer report, failed check or compile error fails the test."""
import os
import shutil
import subprocess

import pytest

from mibminet.params import ParamSet, dot_ranges
from support import ROWS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mi-bminet_amd", "csrc")
I32_MAX = 2 ** 31 - 1


def _compiler():
    for cxx in (os.environ.get("CXX"), "g++", "c++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        if cxx and shutil.which(cxx):
            return shutil.which(cxx)
    pytest.fail("no host C++ compiler")


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
    exe = str(tmp_path / "host_arith")
    cmd = [_compiler(), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-static-libasan",  # the runtime inside the program: its place in the library list cannot matter
           "-I", CSRC, "-o", exe, os.path.join(ROOT, "tests", "host_arith_main.cpp")]
    cc = subprocess.run(cmd, capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-4000:]
    sets = [row[0]() for row in ROWS] + [_int32_end_set()]
    paths = []
    for i, ps in enumerate(sets):
        paths.append(str(tmp_path / f"set{i}.blob"))
        with open(paths[-1], "wb") as f:
            f.write(ps.to_blob())
    run = subprocess.run([exe] + paths, capture_output=True, text=True)
    assert run.returncode == 0 and not run.stderr.strip(), (run.stdout[-2000:], run.stderr[-4000:])
    lines = [ln.split() for ln in run.stdout.splitlines() if ln.startswith("set ")]
    assert [ln[1] for ln in lines] == paths
    got = [tuple(int(v) for v in ln[2:]) for ln in lines]  # rc, xr, layer, filter, folded
    # the plan's verdict as net_params_info reports it for the compiled geometries (the general
    # path reports no filter)
    want = []
    for _, _, _, path, first, exact, folded in ROWS:
        want.append((0, int(exact)) + (first if path != "general" else got[len(want)][2:4]) + (folded,))
    want.append((0, 1, 1, 5, 0))
    assert got == want
    assert "sweep 125 factors" in run.stdout
