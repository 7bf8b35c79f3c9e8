"""What more than one test module uses: the oracle's thread count, device placement at a byte
offset, the materialisers and recordings of the window and epoch suites, the geometry sweep, the
observability suites' entry runner, the pinned parameter images' table, the argument-check
suites' fixture and the runner of the stand-alone host programs.  A plain module, imported as ``observability`` is; no test module imports another.
A helper with one user stays in that user's file."""
import os
import shutil
import subprocess

import numpy as np
import pytest
from numpy.lib.stride_tricks import sliding_window_view

import oracle
from mibminet import lib
from mibminet.params import ParamSet, pack_trials
from oracle import golden_np as G

NTH = min(16, os.cpu_count() or 1)


# ---- inputs and references ------------------------------------------------------------------------
def at_offset(torch, arr, offset):
    """`arr` (int8 or float32, any shape) on the device, its first byte `offset` bytes into a
    zero-filled allocation with 64 spare bytes."""
    a = np.ascontiguousarray(arr)
    raw = torch.from_numpy(a.view(np.uint8).ravel()).cuda()
    flat = torch.zeros(offset + raw.numel() + 64, dtype=torch.uint8, device="cuda")
    flat[offset: offset + raw.numel()] = raw
    dt = {np.dtype(np.int8): torch.int8, np.dtype(np.float32): torch.float32}[a.dtype]
    return flat[offset: offset + raw.numel()].view(dt).view(*a.shape)


def sliding_windows(x_ct, T, hop):
    """[C][L] -> the windows [W][C][T], window w = x[:, w hop : w hop + T]."""
    v = sliding_window_view(x_ct, T, axis=1)[:, ::hop]
    return np.ascontiguousarray(v.transpose(1, 0, 2))


def windows_at(x_ct, onsets, T):
    """[C][L] -> the windows [W][C][T], window i = x[:, onsets[i] : onsets[i] + T]."""
    idx = np.asarray(onsets, np.int64)[:, None] + np.arange(T, dtype=np.int64)[None, :]
    return np.ascontiguousarray(x_ct[:, idx].transpose(1, 0, 2))


def epochs_of(src, onsets, channels, row_stride, T):
    """The epochs [E][C][T] of the flat view of `src`."""
    on = np.asarray(onsets, np.int64)
    ch = np.asarray(channels, np.int64)
    idx = on[:, None, None] + ch[None, :, None] * row_stride + np.arange(T, dtype=np.int64)[None, None, :]
    return np.ascontiguousarray(src.reshape(-1)[idx])


def want(ps, trials_ct):
    """The C oracle's logits of the trials [B][C][T]."""
    return oracle.COracle(ps).batch(pack_trials(trials_ct), nthreads=NTH)


def recording(ps, L, seed):
    return np.random.default_rng(seed).integers(-128, 128, size=(ps.dims.C, L)).astype(np.int8)


def source(shape, seed):
    return np.random.default_rng(seed).integers(-128, 128, size=shape).astype(np.int8)


def length(T, hop, residue, wmin=40):
    """The shortest L with at least wmin windows and L % 16 == residue."""
    L = T + (wmin - 1) * hop
    while L % 16 != residue:
        L += 1
    return L


def float_recording(torch, C, L, offset, seed):
    """A float32 recording [C][L] with non-finite samples planted, and its two-pass quantisation
    (scale 3) as an int8 [C][L] array."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    xf = at_offset(torch, np.zeros((C, L), np.float32), offset)
    xf.copy_(torch.randn((C, L), dtype=torch.float32, device="cuda", generator=g) * 1.3)
    xf[0, :7] = torch.tensor([float("nan"), float("inf"), -float("inf"), 3.0, -3.0, 0.0, -0.0])
    xf[C - 1, L - 3:] = torch.tensor([float("nan"), -float("inf"), float("inf")])
    q = lib.quantize_input_torch(xf[None].contiguous(), 3.0)  # [1][stride], the trial [L][C]
    return xf, np.ascontiguousarray(q.cpu().numpy()[0, : L * C].reshape(L, C).T)


def tile_sweep():
    """32 geometries, one per residue of layer 2's column blocks mod 32 (NB2 = ceil(T8 / 4): rest
    0 = whole 32x32 tiles, 1-16 = one or two 16x16x64 tail tiles, 17-31 = one more full tile),
    each with 0-4 full tiles, C over 1..64, N over 1..16, T mod 16 and T mod 64 varied, the
    largest trials past the LDS staging limit (unstaged fragments), and both build variants on
    some of them."""
    out = []
    for rest in range(32):
        m = max(rest % 4, 1 if rest < 2 else 0)
        T8 = 4 * (32 * m + rest) - rest % 4
        T = 8 * T8 + (3 * rest) % 8
        kw = {}
        if rest % 5 == 1:
            kw["reorder_bn"] = False
        if rest % 7 == 3:
            kw["clip_balanced"] = True
        out.append((1 + (7 * rest) % 64, T, 1 + rest % 16, kw))
    return out


# the invalid onsets of the persistent-loop tests, among them values whose low 32 bits would be valid
_BAD = [-1, None, 2**31, 2**32, 2**32 + 5, -(2**63), 2**63 - 1]  # None: one past the last valid onset


# ---- the observability suites: every forward entry on one certified batch ---------------------------
SCALE = 3.0


def dequant(q):
    """float32 samples that the input quantiser (scale SCALE) maps back to the int8 array q: the
    middle of each value's interval, (q + 0.5 sgn q) SCALE / 127; checked with the NumPy quantiser."""
    v = np.arange(-127, 128)
    lut = ((v + 0.5 * np.sign(v)) * (SCALE / 127.0)).astype(np.float32)
    assert np.array_equal(G.quantize_to_int(lut, SCALE), v)  # the quantiser works sample by sample
    q = np.asarray(q, np.int8)
    assert q.min() >= -127
    return lut[q.astype(np.int16) + 127]


def trials_as_recording(x, gap, junk):
    """The trials [B][C][T] end to end as one recording [C][B (T + gap)], `gap` junk samples after
    each: window w at hop T + gap is trial w."""
    B, C, T = x.shape
    rec = junk.integers(-127, 128, size=(C, B, T + gap), dtype=np.int8)
    rec[:, :, :T] = x.transpose(1, 0, 2)
    return np.ascontiguousarray(rec.reshape(C, B * (T + gap)))


def scattered(x, junk):
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


def run_entries(case, path):
    """Every forward entry on a certified case (observability.CASES, param_faults.PCASES), which
    must run the kernels `path` names."""
    name, ps, x = case
    lib.params_load(ps)
    info = lib.params_info()
    assert info["path"] == path, info
    assert info["exact_division"] == case.exact
    run_entries_on(name, ps, x, oracle.COracle(ps).batch(pack_trials(x), nthreads=NTH))


def run_entries_on(name, ps, x, want, again=None):
    """Every forward entry on the trials x [B][C][T] (int8 in [-127, 127]) of the loaded set ps:
    each must give `want` [B][N], byte for byte, in every row.  `again`: a context manager under
    which each batched entry runs a second time on the same input, to the same bytes."""
    import torch

    d = ps.dims
    B = len(x)
    xp = pack_trials(x)
    junk = np.random.default_rng(B + d.T)

    def check(got, what, rows=None):
        got = got.cpu().numpy()
        assert got.shape == (B, d.N), f"{name} {what}: {got.shape}"
        bad = np.flatnonzero((got != (want if rows is None else want[rows])).any(1))
        assert bad.size == 0, f"{name} {what}: {bad.size} of {B} trials differ, first {bad[:5]}"

    for what, run in (("time-major", lambda v=torch.from_numpy(xp).cuda(): lib.forward_torch(v)),
                      ("channel-major", lambda v=at_offset(torch, x, 1 + B % 3): lib.forward_ct_torch(v)),
                      ("float32", lambda v=torch.from_numpy(dequant(x)).cuda(): lib.forward_f32_torch(v, SCALE))):
        got = run()
        check(got, what)
        if again is not None:
            with again():
                assert torch.equal(run(), got), f"{name} {what}: the second run differs"
    for gap in (0, 3):
        rec = trials_as_recording(x, gap, junk)
        for layout in ("ct", "tc"):
            r = at_offset(torch, rec if layout == "ct" else rec.T, 1 + gap % 2)
            check(lib.forward_windows_torch(r, d.T + gap, layout=layout), f"windows {layout} gap {gap}")
        if gap == 3:
            recf = torch.from_numpy(dequant(rec)).cuda()
            check(lib.forward_windows_f32_torch(recf, d.T + gap, SCALE), "windows float32")
            # the windows at given onsets: the same trials in shuffled order (a generator of its own, so
            # the inputs of the entries below stay what they were)
            order = np.random.default_rng(B + d.T + 1).permutation(B)
            onsets = [int(w) * (d.T + gap) for w in order]
            for layout in ("ct", "tc"):
                r = at_offset(torch, rec if layout == "ct" else rec.T, 2)
                check(lib.forward_windows_at_torch(r, onsets, layout=layout), f"windows at {layout}", order)
            check(lib.forward_windows_at_torch(recf, onsets, scale=SCALE), "windows at float32", order)
    src, onsets, channels = scattered(x, junk)
    check(lib.forward_epochs_torch(at_offset(torch, src, 3), onsets, channels=channels), "epochs")
    check(lib.forward_epochs_torch(torch.from_numpy(dequant(src)).cuda(), onsets, channels=channels, scale=SCALE),
          "epochs float32")
    np.testing.assert_array_equal(lib.net_model_compute(oracle.to_tc_align(x[0], d.C_ALIGN)), want[0])


# ---- the pinned parameter images (tests/test_images_cpu.py; tests/test_host_sanitizers.py parses the same sets)
S, X = ParamSet.synthetic, ParamSet.synthetic_extreme

# (set, digest of a normal load, digest under force_general, path, (layer, filter) of the first
# unproven requant, exact division, folded filters).  The digests were taken before the host library
# was split into headers, except the three force_general digests marked "plan": those are
# gen::GenParams images on the exact-division path, which used to carry whatever float constants
# were proven before the first unproven requant.  The exact-division kernels read none of them, and
# the requant plan leaves them zero (l1_r, l1_c, l2_r, l2_c, l3_r, l3_c, sg.l4_r, sg.l4_c, sg.l4_ci);
# every other byte of those images is what it was (0x9ac8cb6cbfd30bfc, 0x3d9d268dc4fc7608 and
# 0xc536a2f9bb5612a8 before).
ROWS = [
    (lambda: S(seed=42), 0x4CB99661AE2E985F, 0x62C068192A10D240, "float", (0, -1), False, 0),
    (lambda: S(seed=11, C=64, T=480, reorder_bn=False, clip_balanced=True), 0x26BE86B5FF09FE11, 0xA16C3DCD74DBE89C,
     "float", (0, -1), False, 0),
    (lambda: S(seed=5, weight_bits=4), 0xF07E14F27F874034, 0x95498DF6658C7CD3, "float", (0, -1), False, 0),
    (lambda: X(seed=77, mids=0), 0xDCBEF0D736030AC9, 0x34FFA648D22236AC, "float", (0, -1), False, 15),
    (lambda: X(seed=77, mids=3), 0x34B6676BA8094F89, 0xD1B7969D33B1A627, "exact", (1, 1), True, 14),  # plan
    (lambda: X(seed=78, mids=3, reorder_bn=False), 0x983A5A7FBC4895E1, 0x44003711BD83F9D8, "exact", (1, 0), True,
     15),  # plan
    (lambda: S(seed=3, C=3, T=64, N=1), 0x1D5848C8AD998815, 0x1D5848C8AD998815, "general", (0, -1), False, 0),
    (lambda: S(seed=4, C=19, T=1125, N=3), 0xC434B9F175686C68, 0xC434B9F175686C68, "general", (0, -1), False, 0),
    (lambda: S(seed=6, C=64, T=4096, N=16), 0xC44B5C39C8356693, 0xC44B5C39C8356693, "general", (0, -1), False, 0),
    (lambda: X(seed=79, C=38, T=480, N=2, mids=3), 0x8FF2E4FC03D11552, 0x8FF2E4FC03D11552, "general", (0, -1), True,
     14),  # plan
]


# ---- the CPU argument-check suites ------------------------------------------------------------------
@pytest.fixture
def loaded():
    ps = ParamSet.synthetic(seed=5)  # 22 x 1125, N = 4
    lib.params_load(ps)
    yield ps
    lib.params_unload()


# ---- the GPU suites of the bank and stream entries --------------------------------------------------
CAPS = (1, 3, 0)  # lib.grid_cap: one workgroup, three, and the normal grid
GUARD = 0x5A      # the byte around and under what a call writes


@pytest.fixture
def capped(gpu):
    """lib.grid_cap for the test; the cap is 0 again afterwards whatever happens."""
    try:
        yield lib.grid_cap
    finally:
        lib.grid_cap(0)


def dev(torch, a):
    """`a` on the device, 4 bytes off a 16-byte boundary (a copy: the shared arrays are read-only)."""
    return at_offset(torch, np.array(a), 4)


def same(rows, expect, what=""):
    """Two arrays of rows, [n][N] or [n][...] (a row is everything under its first index)."""
    assert rows.shape == expect.shape, (what, rows.shape, expect.shape)
    bad = np.flatnonzero((rows != expect).any(axis=tuple(range(1, rows.ndim))))
    assert bad.size == 0, f"{what}: {bad.size} of {len(expect)} rows differ, first {bad[:5]}"


def same_each(rows, expect, what=""):
    """Two lists of per-session arrays [k_i][N]."""
    assert len(rows) == len(expect)
    for i, (r, e) in enumerate(zip(rows, expect)):
        assert r.shape == e.shape, (what, i, r.shape, e.shape)
        bad = np.flatnonzero((r != e).any(axis=1))
        assert bad.size == 0, f"{what} session {i}: {bad.size} of {len(e)} windows differ, first {bad[:5]}"


def same_rows(got, expect, what=""):
    """Two arrays [...][N] (a row is the last axis); `got` may be a list of arrays."""
    got = np.asarray(got)
    assert got.shape == expect.shape, (what, got.shape, expect.shape)
    bad = np.flatnonzero((got != expect).any(axis=-1).reshape(-1))
    assert bad.size == 0, f"{what}: {bad.size} of {expect[..., 0].size} rows differ, first {bad[:5]}"


# ---- the stand-alone host programs under the sanitizers ---------------------------------------------
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mi-bminet_amd", "csrc")


def run_host_program(main_cpp, args, tmp_path):
    """Builds tests/`main_cpp` (it includes HIP-free headers of csrc/ only) with the host C++ compiler
    under AddressSanitizer and UndefinedBehaviorSanitizer (once per `tmp_path`), runs it on `args` as
    an ordinary child process, nothing loaded into Python, and returns its stdout.  A compile error,
    a non-zero exit or anything on stderr (a sanitizer report) fails the test."""
    exe = str(tmp_path / os.path.splitext(main_cpp)[0])
    if not os.path.exists(exe):
        cxx = next((shutil.which(c) for c in (os.environ.get("CXX"), "g++", "c++", "clang++", "/opt/rocm/llvm/bin/clang++")
                    if c and shutil.which(c)), None)
        assert cxx, "no host C++ compiler"
        cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
               "-static-libasan",  # the runtime inside the program: its place in the library list cannot matter
               "-I", CSRC, "-o", exe, os.path.join(ROOT, "tests", main_cpp)]
        cc = subprocess.run(cmd, capture_output=True, text=True)
        assert cc.returncode == 0, cc.stderr[-4000:]
    run = subprocess.run([exe] + list(args), capture_output=True, text=True)
    assert run.returncode == 0 and not run.stderr.strip(), (args, run.stdout[-2000:], run.stderr[-4000:])
    return run.stdout


def aligned(nbytes, align=16):
    """A host buffer and an `align`-aligned address inside it."""
    buf = np.zeros(nbytes + align, np.uint8)
    a = buf.ctypes.data
    return buf, (a + align - 1) // align * align
