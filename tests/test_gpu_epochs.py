"""Epochs read straight out of a wider array (net_model_compute_epochs, forward_ep.hpp): logit row
e must be byte-identical to the forward of the materialised trial
src.flat[onsets[e] + channels[c] row_stride + t].

The reference is always the C oracle on epochs materialised with NumPy indexing from the host
copy of the source (-> [E][C][T] -> pack_trials -> COracle.batch); the existing channel-major
batched entry (forward_ct_torch) on the same materialised epochs is a second witness.  Inputs are
uniform int8 from seeded generators.
"""
import ctypes

import numpy as np
import pytest

import oracle
from mibminet import lib
from mibminet.params import ParamSet, pack_trials
from support import _BAD, NTH, at_offset, epochs_of, source, tile_sweep
from support import want as _want

pytestmark = pytest.mark.gpu


def _check_epochs(ps, src, onsets, channels, offset=0, witness=True, row_stride=None):
    """The int8 source `src` (placed `offset` bytes into its allocation) through
    forward_epochs_torch against the oracle (and forward_ct_torch) on the materialised epochs.
    The set must be loaded.  Returns the expected logits."""
    import torch

    d = ps.dims
    rs = src.shape[-1] if row_stride is None else row_stride
    ch = list(range(d.C)) if channels is None else channels
    epochs = epochs_of(src, onsets, ch, rs, d.T)
    want = _want(ps, epochs)
    x = at_offset(torch, src, offset)
    got = lib.forward_epochs_torch(x, onsets, channels=channels, row_stride=row_stride).cpu().numpy()
    assert got.shape == (len(onsets), d.N)
    np.testing.assert_array_equal(got, want, err_msg=f"epochs vs oracle, offset {offset}")
    if witness:
        full = lib.forward_ct_torch(torch.from_numpy(epochs).cuda()).cpu().numpy()
        np.testing.assert_array_equal(full, want, err_msg="forward_ct_torch vs oracle")
    return want


_CH19 = [23, 0, 7, 22, 3, 3, 15, 1, 19, 11, 5, 21, 2, 9, 14, 8, 0, 17, 12]  # non-monotonic, duplicates, rows 0 and 23


@pytest.mark.parametrize("L", [580, 581, 583])
def test_alignment(L, gpu):
    """Every byte alignment of the epoch rows: the x pointer 0-3 bytes into its allocation, row
    lengths L % 4 in {0, 1, 3}, onsets over every residue mod 16 (0 and the last valid one,
    duplicates, unsorted), a non-monotonic channel list with duplicates."""
    ps = ParamSet.synthetic(seed=19, C=19, T=480, N=3)
    lib.params_load(ps)
    assert lib.params_info()["path"] == "general"
    assert len(_CH19) == 19 and L % 4 in (0, 1, 3)
    src = source((24, L), L)
    last = L - 480  # n_elems - span = 24 L - (23 L + 480)
    rng = np.random.default_rng(L + 1)
    onsets = [0, last, last, 0] + [int(v) for v in rng.permutation(np.arange(1, 45))]  # 44 consecutive: every residue
    assert {o % 16 for o in onsets} == set(range(16)) and max(onsets) == last
    for offset in range(4):
        _check_epochs(ps, src, onsets, _CH19, offset=offset, witness=offset == 0)


@pytest.mark.parametrize("C,T", [(22, 1125), (19, 481)])
def test_partial_last_block(C, T, gpu):
    """T % 16 != 0: the last layer-1 block reads past the epoch.  One epoch ends at the source's
    very last element (zeros past the view); the others are followed in their rows by extreme
    bytes (-128 / 127), or by NaN and infinities in the float32 source, none of which may reach a
    stored sample."""
    import torch

    assert T % 16 != 0
    ps = ParamSet.synthetic(seed=C + T, C=C, T=T, N=4)
    lib.params_load(ps)
    R, gap = C + 2, 16
    L = 3 * (T + gap) + T
    onsets = [2 * (T + gap), 0, L - T, T + gap]
    channels = [R - 1] + list(range(C - 1))  # the last row: epoch L - T ends at the last element
    src = source((R, L), T)
    for o in onsets[:2] + onsets[3:]:
        src[:, o + T: o + T + gap] = np.where(np.arange(gap) % 2 == 0, -128, 127).astype(np.int8)
    for offset in (0, 3):
        _check_epochs(ps, src, onsets, channels, offset=offset, witness=offset == 0)
    # float32: the same layout with non-finite values after the epochs
    g = torch.Generator(device="cuda").manual_seed(T)
    xf = at_offset(torch, np.zeros((R, L), np.float32), 4)
    xf.copy_(torch.randn((R, L), dtype=torch.float32, device="cuda", generator=g) * 1.3)
    junk = torch.tensor([float("nan"), float("inf"), -float("inf"), float("nan")] * (gap // 4), device="cuda")
    for o in onsets[:2] + onsets[3:]:
        xf[:, o + T: o + T + gap] = junk
    q = lib.quantize_input_torch(xf[None].contiguous(), 3.0)  # [1][stride], the trial [L][R]
    q_rl = np.ascontiguousarray(q.cpu().numpy()[0, : L * R].reshape(L, R).T)
    want = _want(ps, epochs_of(q_rl, onsets, channels, L, T))
    got = lib.forward_epochs_torch(xf, onsets, channels=channels, scale=3.0).cpu().numpy()
    np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("offset", [0, 4])
def test_float32(offset, gpu):
    """The in-kernel input quantiser per sample against the two-pass quantiser on the whole
    source, with non-finite and +-3 scale samples planted inside epochs."""
    import torch

    ps = ParamSet.synthetic(seed=20, C=19, T=480, N=3)
    lib.params_load(ps)
    L = 611
    g = torch.Generator(device="cuda").manual_seed(offset + 7)
    xf = at_offset(torch, np.zeros((24, L), np.float32), offset)
    assert xf.data_ptr() % 8 == offset
    xf.copy_(torch.randn((24, L), dtype=torch.float32, device="cuda", generator=g) * 1.3)
    plant = torch.tensor([float("nan"), float("inf"), -float("inf"), 9.0, -9.0, 0.0, -0.0, 3.0, -3.0], device="cuda")
    xf[0, 5:14] = plant
    xf[23, L - 9:] = plant
    xf[7, 300:309] = plant
    q = lib.quantize_input_torch(xf[None].contiguous(), 3.0)
    q_rl = np.ascontiguousarray(q.cpu().numpy()[0, : L * 24].reshape(L, 24).T)
    onsets = [0, L - 480, 5, 77, 5, 130, 16, 1]
    want = _want(ps, epochs_of(q_rl, onsets, _CH19, L, 480))
    got = lib.forward_epochs_torch(xf, onsets, channels=_CH19, scale=3.0).cpu().numpy()
    np.testing.assert_array_equal(got, want)
    full = lib.forward_ct_torch(torch.from_numpy(epochs_of(q_rl, onsets, _CH19, L, 480)).cuda()).cpu().numpy()
    np.testing.assert_array_equal(full, want)


def _geometries():
    sweep = tile_sweep()
    Ts = [64, 65] + [sweep[r][1] for r in (0, 1, 16, 17, 5, 9, 20, 31)] + [64, 65]
    Cs = [1, 16, 17, 33, 64, 1, 16, 17, 33, 64, 64, 33]
    kws = [{}, {}] + [sweep[r][3] for r in (0, 1, 16, 17, 5, 9, 20, 31)] + [{}, {}]
    return [(C, T, 1 if i % 2 == 0 else 16, kw) for i, (C, T, kw) in enumerate(zip(Cs, Ts, kws))]


def _channels(C, R, seed):
    """C rows out of R in random order, the last row among them, one duplicate when C > 2."""
    ch = [int(v) for v in np.random.default_rng(seed).permutation(R)[:C]]
    ch[0] = R - 1
    if C > 2:
        ch[C // 2] = ch[1]
    return ch


@pytest.mark.parametrize("C,T,N,kw", _geometries())
def test_geometries(C, T, N, kw, gpu):
    """One to 64 channels, one and sixteen classes, the shortest T, T = 1 mod 16 and layer 2's
    tile residues, each with a channel subset of a wider source and unsorted onsets that include 0
    and the last valid one."""
    assert 64 <= T <= 4096
    ps = ParamSet.synthetic(seed=C * T + N, C=C, T=T, N=N, **kw)
    lib.params_load(ps)
    R, L = C + 3, T + 37
    _check_epochs(ps, source((R, L), C + T), [37, 0, 13, 13, 7], _channels(C, R, T), offset=1)


def test_longest_trial(gpu):
    ps = ParamSet.synthetic(seed=4096, C=64, T=4096, N=5)
    lib.params_load(ps)
    R, L = 66, 4096 + 50
    _check_epochs(ps, source((R, L), 4096), [50, 0, 3, 17, 17, 32, 49, 1], _channels(64, R, 1), offset=3)


_VARIANTS = [dict(reorder_bn=False), dict(clip_balanced=True), dict(weight_bits=4), dict(extreme=3)]


@pytest.mark.parametrize("kw", _VARIANTS, ids=lambda kw: "-".join(f"{k}={v}" for k, v in kw.items()))
def test_variants(kw, gpu):
    """Plain BN, balanced clip, int4 weights and an exact-division set on a general geometry."""
    C, T, N = 38, 480, 2
    if "extreme" in kw:
        ps = ParamSet.synthetic_extreme(seed=C + T, C=C, T=T, N=N, mids=kw["extreme"])
    else:
        ps = ParamSet.synthetic(seed=C + T, C=C, T=T, N=N, **kw)
    lib.params_load(ps)
    if "extreme" in kw:
        assert lib.params_info()["exact_division"]
    R, L = 64, 640
    onsets = [160, 0, 1, 159, 80, 80, 33, 15, 16, 17, 31]
    _check_epochs(ps, source((R, L), C + len(kw)), onsets, _channels(C, R, 5), offset=2)


@pytest.mark.parametrize("C,T", [(22, 1125), (64, 1000), (64, 480)])
def test_compiled_geometries(C, T, gpu):
    """The compiled geometries run the epoch kernels through the window kernels' parameter image;
    the compiled kernels and what net_params_info reports stay as they were."""
    import torch

    ps = ParamSet.synthetic(seed=C + T, C=C, T=T)
    lib.params_load(ps)
    info = lib.params_info()
    assert info["path"] == "float"
    R, L = C + 2, T + 99
    _check_epochs(ps, source((R, L), C * T), [99, 0, 50, 7, 7, 98], _channels(C, R, 3), offset=1)
    assert lib.params_info() == info
    xp = pack_trials(np.random.default_rng(T).integers(-128, 128, size=(41, C, T)))
    got = lib.forward_torch(torch.from_numpy(xp).cuda()).cpu().numpy()
    np.testing.assert_array_equal(got, oracle.COracle(ps).batch(xp, nthreads=NTH))


def test_identity(gpu):
    """channels = None, row_stride = T and onsets = b C T on a [B][C][T] batch: the batch itself."""
    import torch

    ps = ParamSet.synthetic(seed=31, C=19, T=480, N=3)
    lib.params_load(ps)
    B = 41
    xb = source((B, 19, 480), 31)
    x = at_offset(torch, xb, 1)
    want = lib.forward_ct_torch(x)
    got = lib.forward_epochs_torch(x, torch.arange(B, dtype=torch.int64) * (19 * 480), row_stride=480)
    assert bool((got == want).all())
    np.testing.assert_array_equal(want.cpu().numpy(), _want(ps, xb))


@pytest.mark.parametrize("t0", [0, 1, 160])
def test_forward_crop(t0, gpu):
    import torch

    ps = ParamSet.synthetic(seed=33, C=19, T=480, N=3)
    lib.params_load(ps)
    ch = [63, 0, 31, 8, 9, 10, 40, 41, 42, 20, 21, 22, 50, 51, 52, 60, 61, 62, 5]
    xb = source((37, 64, 640), 33)
    want = _want(ps, np.ascontiguousarray(xb[:, ch, t0: t0 + 480]))
    got = lib.forward_crop_torch(torch.from_numpy(xb).cuda(), t0, channels=ch).cpu().numpy()
    np.testing.assert_array_equal(got, want)
    if t0 == 1:  # float32 batch through the same entry
        xf = torch.from_numpy(xb).cuda().to(torch.float32) * (3.0 / 127.0)
        q = lib.quantize_input_torch(xf, 3.0).cpu().numpy()[:, : 64 * 640].reshape(37, 640, 64).transpose(0, 2, 1)
        want_f = _want(ps, np.ascontiguousarray(q[:, ch, t0: t0 + 480]))
        np.testing.assert_array_equal(lib.forward_crop_torch(xf, t0, channels=ch, scale=3.0).cpu().numpy(), want_f)
    with pytest.raises(ValueError):
        lib.forward_crop_torch(torch.from_numpy(xb).cuda(), 161, channels=ch)


def test_persistent_loop(gpu):
    """More epochs than resident workgroups: E = 3 grid + 1, so every workgroup loops and one
    runs a fourth epoch."""
    import torch

    ps = ParamSet.synthetic(seed=41, C=4, T=64, N=4)
    lib.params_load(ps)
    grid = 2 * torch.cuda.get_device_properties(0).multi_processor_count  # two workgroups per CU
    E = 3 * grid + 1
    src = source((6, 64 + E), 41)
    onsets = [int(v) for v in np.random.default_rng(41).permutation(E)]
    _check_epochs(ps, src, onsets, [5, 0, 3, 3], offset=3, witness=False)


def test_persistent_loop_with_invalid_onsets(gpu):
    """test_persistent_loop's epochs with every seventh onset invalid (test_gpu_windows_at's values,
    among them ones whose low 32 bits would be valid), so that a workgroup meets invalid epochs on
    its first pass, on its last and in between: their rows are zero, n_bad counts them exactly,
    every other row matches the oracle and nothing is written past y.  Then the same source as
    float32 through the in-kernel quantiser, against the oracle on the two-pass quantiser's
    samples."""
    import torch

    ps = ParamSet.synthetic(seed=41, C=4, T=64, N=4)
    lib.params_load(ps)
    T, N, ch = 64, 4, [5, 0, 3, 3]
    grid = 2 * torch.cuda.get_device_properties(0).multi_processor_count  # two workgroups per CU
    E = 3 * grid + 1
    L = 64 + E
    src = source((6, L), 41)
    last = 6 * L - (5 * L + T)  # n_elems - span
    assert last == E
    onsets = [int(v) for v in np.random.default_rng(41).permutation(E)]
    bad = list(range(0, E, 7))
    for j, i in enumerate(bad):
        v = _BAD[j % 7]
        onsets[i] = last + 1 if v is None else v
    # the low 32 bits of 2^32, 2^32 + 5 and INT64_MIN are valid onsets: the check must see 64 bits
    assert all(0 <= (v & 0xFFFFFFFF) <= last for v in (2**32, 2**32 + 5, -(2**63)))
    # invalid entries on a workgroup's first pass, on its last (the pass before the one that only
    # finishes) and on one in between
    assert bad[0] < grid and bad[-1] + grid >= E and any(grid <= i < E - grid for i in bad)
    ok = [i for i in range(E) if i % 7]
    want = _want(ps, epochs_of(src, [onsets[i] for i in ok], ch, L, T))
    assert want.any(axis=1).all()  # no valid row is zero itself
    on = torch.tensor(onsets, dtype=torch.int64, device="cuda")
    tab = (ctypes.c_int32 * 4)(*ch)

    def run(x, *scale):
        y = torch.full((E * N + 64,), 0x5A, dtype=torch.int8, device="cuda")
        nb = torch.zeros((3,), dtype=torch.int32, device="cuda")
        entry = lib.load().net_model_compute_epochs_f32 if scale else lib.load().net_model_compute_epochs
        rc = entry(x.data_ptr(), x.numel(), L, tab, on.data_ptr(), E, *scale, y.data_ptr(), nb.data_ptr() + 4, 0, None)
        assert rc == lib.NET_OK
        torch.cuda.synchronize()
        assert nb.cpu().tolist() == [0, len(bad), 0]
        assert bool((y[E * N:] == 0x5A).all())
        rows = y[: E * N].view(E, N).cpu().numpy()
        assert not rows[bad].any()
        return rows[ok]

    np.testing.assert_array_equal(run(at_offset(torch, src, 3)), want)
    # float32, scale 3: the samples the two-pass quantiser makes of it (-128 becomes -127)
    xf = at_offset(torch, src.astype(np.float32) * np.float32(3.0 / 127.0), 4)
    q = lib.quantize_input_torch(xf[None].contiguous(), 3.0)  # [1][stride], the trial [L][6]
    q_rl = np.ascontiguousarray(q.cpu().numpy()[0, : L * 6].reshape(L, 6).T)
    assert (np.abs(q_rl.astype(int) - src) <= 1).all()
    want_f = _want(ps, epochs_of(q_rl, [onsets[i] for i in ok], ch, L, T))
    np.testing.assert_array_equal(run(xf, 3.0), want_f)


def test_invalid_onsets(gpu):
    """Onsets outside the source form no address: their rows are zero, n_bad counts them and
    every valid row still matches the oracle."""
    import torch

    ps = ParamSet.synthetic(seed=19, C=19, T=480, N=3)
    lib.params_load(ps)
    L = 583
    src = source((24, L), 77)
    last = L - 480
    bad = {1: -1, 4: last + 1, 5: 2**40, 9: -(2**40), 10: -(2**63), 14: 2**63 - 1, 15: 24 * L}
    onsets = [int(v) for v in np.random.default_rng(5).integers(0, last + 1, size=17)]
    onsets[0], onsets[16] = last, 0
    for i, o in bad.items():
        onsets[i] = o
    ok = [i for i in range(17) if i not in bad]
    want = _want(ps, epochs_of(src, [onsets[i] for i in ok], _CH19, L, 480))
    x = at_offset(torch, src, 2)
    on = torch.tensor(onsets, dtype=torch.int64, device="cuda")
    y = torch.full((17 * 3 + 64,), 0x5A, dtype=torch.int8, device="cuda")
    nb = torch.zeros((3,), dtype=torch.int32, device="cuda")
    tab = (ctypes.c_int32 * 19)(*_CH19)
    rc = lib.load().net_model_compute_epochs(x.data_ptr(), x.numel(), L, tab, on.data_ptr(), 17, y.data_ptr(),
                                             nb.data_ptr() + 4, 0, None)
    assert rc == lib.NET_OK
    torch.cuda.synchronize()
    assert nb.cpu().tolist() == [0, len(bad), 0]
    rows = y[: 17 * 3].view(17, 3).cpu().numpy()
    assert bool((y[17 * 3:] == 0x5A).all())
    np.testing.assert_array_equal(rows[ok], want)
    assert not rows[sorted(bad)].any()
    # n_bad == NULL: the same rows, nothing counted
    got = lib.forward_epochs_torch(x, on, channels=_CH19, check=False).cpu().numpy()
    np.testing.assert_array_equal(got, rows)
    with pytest.raises(ValueError, match=f"{len(bad)} of 17"):
        lib.forward_epochs_torch(x, on, channels=_CH19)
    # no epoch: nothing is written
    assert lib.forward_epochs_torch(x, [], channels=_CH19).shape == (0, 3)


def test_graph_capture_and_replay(gpu):
    """One eager call uploads the parameters; a captured net_model_compute_epochs launch then
    replays on changed source contents."""
    import torch

    ps = ParamSet.synthetic(seed=19, C=19, T=480, N=3)
    lib.params_load(ps)
    L = 700
    rng = np.random.default_rng(3)
    srcs = [source((24, L), 100 + i) for i in range(3)]
    onsets = [int(v) for v in rng.integers(0, L - 480 + 1, size=300)]
    x = at_offset(torch, srcs[0], 1)
    on = torch.tensor(onsets, dtype=torch.int64, device="cuda")
    lib.forward_epochs_torch(x, on, channels=_CH19)  # eager: uploads the parameters
    y = torch.zeros((300, 3), dtype=torch.int8, device="cuda")
    nb = torch.zeros((1,), dtype=torch.int32, device="cuda")
    tab = (ctypes.c_int32 * 19)(*_CH19)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            rc = lib.load().net_model_compute_epochs(x.data_ptr(), x.numel(), L, tab, on.data_ptr(), 300, y.data_ptr(),
                                                     nb.data_ptr(), 0, s.cuda_stream)
    assert rc == lib.NET_OK
    for src in srcs:
        x.copy_(torch.from_numpy(src))
        y.zero_()
        g.replay()
        torch.cuda.synchronize()
        np.testing.assert_array_equal(y.cpu().numpy(), _want(ps, epochs_of(src, onsets, _CH19, L, 480)))
    assert int(nb.item()) == 0
    del g
