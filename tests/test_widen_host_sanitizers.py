"""net_blob_widen's transform under AddressSanitizer and UndefinedBehaviorSanitizer (no GPU, and
nothing loaded into Python): tests/widen_host_main.cpp includes only csrc/params_host.hpp, is built
here with the host C++ compiler and run as an ordinary child process, once per set.  It hands
widen_blob heap blocks of exactly the sizes it names: every truncation of the blob and a handful of
spoilt headers (NET_ERR_BLOB first), R and the channel entries at and past their limits, the size
query, a cap one byte short and an exact one, and holds the output to the input field by field.  Any
sanitizer report, failed check or compile error fails the test."""
from mibminet.params import ParamSet
from support import run_host_program

S, X = ParamSet.synthetic, ParamSet.synthetic_extreme
# (the set, R)
SETS = [
    (lambda: S(seed=31, C=19, T=480, N=3), 64),
    (lambda: S(seed=32, C=8, T=64, N=2), 13),
    (lambda: S(seed=34, C=4, T=64, N=2, weight_bits=4), 5),
    (lambda: S(seed=37, C=1, T=64, N=1, weight_bits=4), 1),
    (lambda: S(seed=33, C=22, T=1125, N=4, reorder_bn=False), 64),
    (lambda: X(seed=79, C=38, T=480, N=2, mids=3, clip_balanced=True), 64),
    (lambda: S(seed=36, C=64, T=480, N=4), 64),
]


def test_widen_host_runs_clean_under_sanitizers(tmp_path):
    for i, (make, R) in enumerate(SETS):
        ps = make()
        path = str(tmp_path / f"set{i}.blob")
        with open(path, "wb") as f:
            f.write(ps.to_blob())
        out = run_host_program("widen_host_main.cpp", [path, str(R), str(100 + i)], tmp_path).split()
        d = ps.dims
        need = len(ps.to_blob()) + d.F2 * ((R + 3) // 4 * 4 - d.C_ALIGN) * ps.weight_bits // 8
        assert out[:10] == ["widen", "C", str(d.C), "R", str(R), "wbits", str(ps.weight_bits), "bytes",
                            str(len(ps.to_blob())), "->"] and out[10] == str(need) and int(out[12]) > 300, (i, out)
