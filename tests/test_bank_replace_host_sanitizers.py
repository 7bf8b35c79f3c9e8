"""The decision part of net_bank_replace under AddressSanitizer and UndefinedBehaviorSanitizer (no
GPU, and nothing loaded into Python): tests/bank_replace_host_main.cpp includes only
csrc/bank_host.hpp, is built here with the host C++ compiler and run as an ordinary child process,
once per bank.  It builds the bank with bank::build, then decides every replacement with
bank::replace_set, the function net_bank_replace calls: refusals (a truncated blob, another N, another
build variant, exact division into a float bank, a bad scale, a bad slot) must leave the bank as it
was, and after every accepted one the whole bank must be, byte for byte, the bank freshly built from
the list as it then stands.  Any sanitizer report, failed check or compile error fails the test."""
import support_bank as sb
import support_features as sf
from mibminet import lib
from mibminet.params import ParamSet
from support import run_host_program

C, T, N = 19, 480, 3
S, X = ParamSet.synthetic, ParamSet.synthetic_extreme
OK, INV, RNG, UNS, BLOB = lib.NET_OK, lib.NET_ERR_INVALID, lib.NET_ERR_RANGE, lib.NET_ERR_UNSUPPORTED, lib.NET_ERR_BLOB


def _run(tmp_path, tag, scales, bank, steps):
    """steps: (slot, ParamSet or bytes, scale, the code expected)."""
    def put(name, v):
        p = str(tmp_path / name)
        with open(p, "wb") as f:
            f.write(v.to_blob() if isinstance(v, ParamSet) else v)
        return p

    args = [str(int(scales)), str(len(bank))] + [put(f"{tag}_set{i}.blob", ps) for i, ps in enumerate(bank)]
    for k, (slot, new, scale, _) in enumerate(steps):
        args += [str(slot), put(f"{tag}_new{k}.blob", new), repr(float(scale))]
    out = run_host_program("bank_replace_host_main.cpp", args, tmp_path).splitlines()
    return out[0], out[1:]


def test_bank_replace_host_runs_clean_under_sanitizers(tmp_path):
    sets = list(sb.sets(C, T, N))
    new, head = sf.new_set(C, T, N), sf.head_set(C, T, N)
    blob = new.to_blob()
    steps = [
        (2, new, 3.0, OK), (2, head, 0.5, OK), (2, head, 0.5, OK), (0, new, 2.0**-60, OK), (4, sets[0], 2.0**60, OK),
        (2, blob[:-4], 1.0, BLOB), (2, blob[:100], 1.0, BLOB), (2, b"", 1.0, BLOB),
        (2, S(seed=9, C=C, T=T, N=N + 1), 1.0, UNS), (2, S(seed=9, C=C, T=T, N=N, reorder_bn=False), 1.0, UNS),
        (2, S(seed=9, C=C, T=T, N=N, clip_balanced=True), 1.0, UNS), (2, S(seed=9, C=C + 1, T=T, N=N), 1.0, UNS),
        (2, X(seed=77, C=C, T=T, N=N, mids=3), 1.0, UNS),
        (2, new, 0.0, INV), (2, new, -1.0, INV), (2, new, 1e-30, RNG), (2, new, 2.0**61, RNG),
        (5, new, 1.0, INV),
        (1, sets[3], 1.0, OK),
    ]
    head_line, lines = _run(tmp_path, "float", True, sets, steps)
    assert head_line == f"bank 5 rc {OK} xr 0"
    assert lines == [f"replace {slot} rc {code}" for slot, _, _, code in steps], lines
    # without scales the scale is ignored
    head_line, lines = _run(tmp_path, "noscale", False, sets[:2], [(1, new, 0.0, OK), (0, new, -1.0, OK)])
    assert (head_line, lines) == (f"bank 2 rc {OK} xr 0", [f"replace 1 rc {OK}", f"replace 0 rc {OK}"])
    # an exact bank takes float sets in the exact form (the fresh bank is then mixed) and exact ones as they are
    ex = list(sb.VARIANTS["all-exact"](C, T, N))
    steps = [(3, sets[1], 1.0, OK), (0, sets[0], 1.0, OK), (3, ex[0], 1.0, OK),
             (1, S(seed=9, C=C, T=T, N=N, reorder_bn=False), 1.0, UNS)]
    head_line, lines = _run(tmp_path, "exact", True, ex, steps)
    assert head_line == f"bank 5 rc {OK} xr 1"
    assert lines == [f"replace {slot} rc {code}" for slot, _, _, code in steps], lines
