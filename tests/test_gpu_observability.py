"""Every kernel family on inputs whose logits see every intermediate element.

The other GPU parity tests prove a fused kernel by ``logits == oracle`` on calibrated
ParamSet.synthetic sets, whose logits depend weakly on most intermediate elements (DESIGN.md §3,
"Observability of the parity tests").  The entries of observability.CASES are certified on the CPU
(tests/test_observability_cpu.py): a one-LSB error in any audited live element of y1..y4 changes
some logit of some trial of the batch.  Here each batch runs through every entry that computes
the forward pass, against the C oracle, byte for byte.
"""
import os

import numpy as np
import pytest

import observability as ob
import oracle
from mibminet import lib
from mibminet.params import pack_trials
from oracle import golden_np as G
from test_gpu_general import _ct
from test_gpu_windows import _at_offset

pytestmark = pytest.mark.gpu
NTH = min(16, os.cpu_count() or 1)
SCALE = 3.0
NAMES = [c.name for c in ob.CASES]
_COMPILED = {(C, T) for C, T, _ in ob.COMPILED}


def _dequant(q):
    """float32 samples that the input quantiser (scale SCALE) maps back to the int8 array q: the
    middle of each value's interval, (q + 0.5 sgn q) SCALE / 127; checked with the NumPy quantiser."""
    v = np.arange(-127, 128)
    lut = ((v + 0.5 * np.sign(v)) * (SCALE / 127.0)).astype(np.float32)
    assert np.array_equal(G.quantize_to_int(lut, SCALE), v)  # the quantiser works sample by sample
    q = np.asarray(q, np.int8)
    assert q.min() >= -127
    return lut[q.astype(np.int16) + 127]


def _recording(x, gap, junk):
    """The trials [B][C][T] end to end as one recording [C][B (T + gap)], `gap` junk samples after
    each: window w at hop T + gap is trial w."""
    B, C, T = x.shape
    rec = junk.integers(-127, 128, size=(C, B, T + gap), dtype=np.int8)
    rec[:, :, :T] = x.transpose(1, 0, 2)
    return np.ascontiguousarray(rec.reshape(C, B * (T + gap)))


def _scattered(x, junk):
    """The trials scattered into a wider source [R][L]: a permuted channel map over R = C + 3 rows,
    unsorted onsets.  Returns (src, onsets, channels); the epochs materialise to x (checked)."""
    B, C, T = x.shape
    R, pitch = C + 3, T + 5
    L = B * pitch + 7
    src = junk.integers(-127, 128, size=(R, L), dtype=np.int8)
    channels = junk.permutation(R)[:C].astype(np.int64)
    onsets = junk.permutation(B).astype(np.int64) * pitch + 2
    idx = onsets[:, None, None] + channels[None, :, None] * L + np.arange(T, dtype=np.int64)[None, None, :]
    src.reshape(-1)[idx] = x
    assert np.array_equal(src.reshape(-1)[idx], x)  # no two epochs overlap
    return src, [int(o) for o in onsets], [int(c) for c in channels]


def _run_entries(case, path):
    import torch

    name, ps, x = case
    d = ps.dims
    B = len(x)
    lib.params_load(ps)
    info = lib.params_info()
    assert info["path"] == path, info
    assert info["exact_division"] == case.exact
    xp = pack_trials(x)
    want = oracle.COracle(ps).batch(xp, nthreads=NTH)
    junk = np.random.default_rng(B + d.T)

    def check(got, what, rows=None):
        got = got.cpu().numpy()
        bad = np.flatnonzero((got != (want if rows is None else want[rows])).any(1))
        assert bad.size == 0, f"{name} {what}: {bad.size} of {B} trials differ, first {bad[:5]}"

    check(lib.forward_torch(torch.from_numpy(xp).cuda()), "time-major")
    check(lib.forward_ct_torch(_ct(torch, x, 1 + B % 3)), "channel-major")
    check(lib.forward_f32_torch(torch.from_numpy(_dequant(x)).cuda(), SCALE), "float32")
    for gap in (0, 3):
        rec = _recording(x, gap, junk)
        for layout in ("ct", "tc"):
            r = _at_offset(torch, rec if layout == "ct" else rec.T, 1 + gap % 2)
            check(lib.forward_windows_torch(r, d.T + gap, layout=layout), f"windows {layout} gap {gap}")
        if gap == 3:
            recf = torch.from_numpy(_dequant(rec)).cuda()
            check(lib.forward_windows_f32_torch(recf, d.T + gap, SCALE), "windows float32")
            # the windows at given onsets: the same trials in shuffled order (a generator of its own, so
            # the inputs of the entries below stay what they were)
            order = np.random.default_rng(B + d.T + 1).permutation(B)
            onsets = [int(w) * (d.T + gap) for w in order]
            for layout in ("ct", "tc"):
                r = _at_offset(torch, rec if layout == "ct" else rec.T, 2)
                check(lib.forward_windows_at_torch(r, onsets, layout=layout), f"windows at {layout}", order)
            check(lib.forward_windows_at_torch(recf, onsets, scale=SCALE), "windows at float32", order)
    src, onsets, channels = _scattered(x, junk)
    check(lib.forward_epochs_torch(_at_offset(torch, src, 3), onsets, channels=channels), "epochs")
    check(lib.forward_epochs_torch(torch.from_numpy(_dequant(src)).cuda(), onsets, channels=channels, scale=SCALE),
          "epochs float32")
    np.testing.assert_array_equal(lib.net_model_compute(oracle.to_tc_align(x[0], d.C_ALIGN)), want[0])


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
        _run_entries(case, ("exact" if case.exact else "float") if compiled else "general")
    finally:
        case.drop()


@pytest.mark.parametrize("name", [c.name for c in ob.CASES if c.dims[:2] in _COMPILED])
def test_certified_case_forced_general(name, gpu):
    """The compiled geometries' certified batches on the general kernels."""
    case = ob.CASES[NAMES.index(name)]
    try:
        lib.force_general(True)
        _run_entries(case, "general")
    finally:
        lib.force_general(False)
        case.drop()
