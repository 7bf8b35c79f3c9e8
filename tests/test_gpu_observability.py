"""Every kernel family on inputs whose logits see every intermediate element.

The other GPU parity tests prove a fused kernel by ``logits == oracle`` on calibrated
ParamSet.synthetic sets, whose logits depend weakly on most intermediate elements (DESIGN.md §3,
"Observability of the parity tests").  The entries of observability.CASES are certified on the CPU
(tests/test_observability_cpu.py): a one-LSB error in any audited live element of y1..y4 changes
some logit of some trial of the batch.  Here each batch runs through every entry that computes
the forward pass, against the C oracle, byte for byte.
"""
import pytest

import observability as ob
from mibminet import lib
from support import run_entries

pytestmark = pytest.mark.gpu
NAMES = [c.name for c in ob.CASES]
_COMPILED = {(C, T) for C, T, _ in ob.COMPILED}


@pytest.mark.parametrize("name", NAMES)
def test_certified_case(name, gpu):
    """Every forward entry on the certified batch: time-major, channel-major 1-3 bytes into its
    allocation, float32, sliding windows in both layouts (the trials end to end at hop T, and with
    three junk samples between them at hop T + 3) and from float32, the windows at given onsets of
    the latter recording in shuffled order (both layouts and float32), epochs out of a wider source
    with a permuted channel map and unsorted onsets (int8 and float32), and the single-trial entry.
    The compiled geometries run their compiled kernels here."""
    case = ob.CASES[NAMES.index(name)]
    try:
        compiled = case.dims[:2] in _COMPILED and case.dims[2] == 4
        run_entries(case, ("exact" if case.exact else "float") if compiled else "general")
    finally:
        case.drop()


@pytest.mark.parametrize("name", [c.name for c in ob.CASES if c.dims[:2] in _COMPILED])
def test_certified_case_forced_general(name, gpu):
    """The compiled geometries' certified batches on the general kernels."""
    case = ob.CASES[NAMES.index(name)]
    try:
        lib.force_general(True)
        run_entries(case, "general")
    finally:
        lib.force_general(False)
        case.drop()
