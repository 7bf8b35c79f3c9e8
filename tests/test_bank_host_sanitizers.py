"""The HIP-free part of a parameter bank under AddressSanitizer and UndefinedBehaviorSanitizer (no
GPU, and nothing loaded into Python): tests/bank_host_main.cpp includes only csrc/bank_host.hpp, is
built here with the host C++ compiler and run as an ordinary child process, once per bank.  It calls
bank::build, the function net_bank_create calls, on the bank's blobs: the first set refused and its
code, every set's image held to the window image the blob gets alone (a bank that is not mixed) or
to the exact-division form of its own plan (the promoted sets of a mixed one); then the partition
bank::range_of of E items over G workgroups for E in {0, 1, G - 1, G, G + 1, 2^31 - 65,536} and G in
{1, 3, 512}, whose ranges must tile [0, E) exactly.  Any sanitizer report, failed check or compile
error fails the test."""
import support_bank as sb
from mibminet import lib
from mibminet.params import ParamSet
from support import run_host_program

S, X = ParamSet.synthetic, ParamSet.synthetic_extreme
# (the sets, the first that disagrees with set 0 or -1, which need exact division when loaded alone)
BANKS = [
    (lambda: sb.sets(19, 480, 3), -1, "00000"),
    (lambda: sb.sets(4, 4096, 16), -1, "00000"),
    (lambda: (S(seed=101), X(seed=77, mids=3), S(seed=102), X(seed=78, mids=3)), -1, "0101"),
    (lambda: sb.sets(22, 1125, 4)[:2] + (S(seed=9, C=22, T=1000, N=4),) + sb.sets(22, 1125, 4)[2:], 2, "000000"),
    (lambda: sb.sets(22, 1125, 4)[:4] + (S(seed=9, reorder_bn=False),), 4, "00000"),
    (lambda: (S(seed=9), S(seed=9, clip_balanced=True), S(seed=9, N=3)), 1, "000"),
    (lambda: (S(seed=9),), -1, "0"),
]


def test_bank_host_runs_clean_under_sanitizers(tmp_path):
    for b, (make, mismatch, xr) in enumerate(BANKS):
        paths = []
        for i, ps in enumerate(make()):
            paths.append(str(tmp_path / f"bank{b}_set{i}.blob"))
            with open(paths[-1], "wb") as f:
                f.write(ps.to_blob())
        stdout = run_host_program("bank_host_main.cpp", paths, tmp_path)
        rc = lib.NET_OK if mismatch < 0 else lib.NET_ERR_UNSUPPORTED
        assert stdout.splitlines() == [f"bank {len(paths)} refused {mismatch} rc {rc} xr {xr}", "ranges 18"], (b, stdout)
