"""Sliding-window classification of a continuous recording (net_model_compute_windows,
forward_win.hpp): logit row w must be byte-identical to the forward of the materialised trial
x[:, w hop : w hop + T].

The reference is always the C oracle on materialised windows (sliding_window_view -> [W][C][T] ->
pack_trials -> COracle.batch); the existing channel-major batched entry (forward_ct_torch) on the
same windows is a second witness.  Inputs are uniform int8 from seeded generators.
"""
import numpy as np
import pytest

import oracle
from mibminet import lib
from mibminet.params import ParamSet, pack_trials
from support import NTH, at_offset, float_recording, length, recording, sliding_windows, tile_sweep

pytestmark = pytest.mark.gpu


def _check_windows(ps, x_ct, hop, offset=0, layouts=("ct", "tc"), witness=True, oracle_every=1):
    """Both int8 layouts of recording x_ct against the oracle (and forward_ct_torch) on the
    materialised windows.  The set must be loaded.  Returns the expected logits."""
    import torch

    d = ps.dims
    wins = sliding_windows(x_ct, d.T, hop)
    W = wins.shape[0]
    assert W == lib.windows_count(x_ct.shape[1], hop)
    idx = np.arange(0, W, oracle_every)
    want = oracle.COracle(ps).batch(pack_trials(wins[idx]), nthreads=NTH)
    full = None
    if witness:
        full = lib.forward_ct_torch(torch.from_numpy(wins).cuda()).cpu().numpy()
        np.testing.assert_array_equal(full[idx], want, err_msg="forward_ct_torch vs oracle")
    for layout in layouts:
        x = at_offset(torch, x_ct if layout == "ct" else x_ct.T, offset)
        got = lib.forward_windows_torch(x, hop, layout=layout).cpu().numpy()
        assert got.shape == (W, d.N)
        np.testing.assert_array_equal(got[idx], want, err_msg=f"{layout} hop {hop} offset {offset}")
        if full is not None:
            np.testing.assert_array_equal(got, full, err_msg=f"{layout} hop {hop} vs forward_ct_torch")
    return want


@pytest.mark.parametrize("hop", [1, 2, 3, 5, 8, 16, 480, 485])
def test_alignment(hop, gpu):
    """Every byte alignment of the window rows (hop is arbitrary) and of the recording (the x
    pointer 0-3 bytes into its allocation), whole and partial last layer-1 blocks of the recording
    (L % 16 in {0, 1, 15}), hops with gaps (hop > T), in both int8 layouts and float32 with
    non-finite samples planted."""
    import torch

    ps = ParamSet.synthetic(seed=19, C=19, T=480, N=3)
    lib.params_load(ps)
    assert lib.params_info()["path"] == "general"
    d = ps.dims
    for i, residue in enumerate((0, 1, 15)):
        L = length(d.T, hop, residue)
        x_ct = recording(ps, L, 1000 * hop + residue)
        _check_windows(ps, x_ct, hop, offset=(hop + i) % 4, witness=residue == 1)
        _check_windows(ps, x_ct, hop, offset=(hop + i + 2) % 4, witness=False)
        # float32 recording: the in-kernel quantiser per sample, against the two-pass quantiser
        xf, q_ct = float_recording(torch, d.C, L, 4 * (i % 2), L)
        want = oracle.COracle(ps).batch(pack_trials(sliding_windows(q_ct, d.T, hop)), nthreads=NTH)
        got = lib.forward_windows_f32_torch(xf, hop, 3.0).cpu().numpy()
        np.testing.assert_array_equal(got, want, err_msg=f"f32 hop {hop} L {L}")


@pytest.mark.parametrize("C,T", [(22, 1125), (64, 1000), (64, 480)])
def test_compiled_geometries(C, T, gpu):
    """The compiled geometries run the window kernels through their extra parameter image; the
    compiled kernels and what net_params_info reports stay as they were."""
    import torch

    ps = ParamSet.synthetic(seed=C + T, C=C, T=T)
    lib.params_load(ps)
    info = lib.params_info()
    assert info["path"] == "float"
    hop, W = 7, 33
    x_ct = recording(ps, T + (W - 1) * hop, C * T)
    _check_windows(ps, x_ct, hop, offset=1)
    assert lib.params_info() == info
    xp = pack_trials(np.random.default_rng(T).integers(-128, 128, size=(41, C, T)))
    got = lib.forward_torch(torch.from_numpy(xp).cuda()).cpu().numpy()
    np.testing.assert_array_equal(got, oracle.COracle(ps).batch(xp, nthreads=NTH))


def test_persistent_loop(gpu):
    """More windows than resident workgroups (several windows per workgroup), at hop 1."""
    ps = ParamSet.synthetic(seed=23)
    lib.params_load(ps)
    x_ct = recording(ps, 1125 + 1536, 23)
    want = _check_windows(ps, x_ct, 1, offset=3, oracle_every=7)
    assert want.shape == (220, 4)


_EDGES = [(1, 64, 1, {}), (5, 100, 16, {}), (64, 4096, 5, {}), (64, 513, 2, {})] + [tile_sweep()[r] for r in (0, 1, 16, 17)]


@pytest.mark.parametrize("C,T,N,kw", _EDGES)
def test_edges(C, T, N, kw, gpu):
    """One channel, one and sixteen classes, the shortest and longest T, T = 1 mod 16, layer 2's
    tile residues 0, 1, 16 and 17; three windows at hop 37, one window (L == T), and none
    (L == T - 1: nothing is written)."""
    import torch

    ps = ParamSet.synthetic(seed=C * T + N, C=C, T=T, N=N, **kw)
    lib.params_load(ps)
    x_ct = recording(ps, T + 2 * 37 + 5, C + T)
    assert lib.windows_count(x_ct.shape[1], 37) == 3
    _check_windows(ps, x_ct, 37, offset=1)
    _check_windows(ps, x_ct[:, :T], 37, offset=2)  # L == T
    # L == T - 1: no window, y and the workspace untouched
    L = T - 1
    x = at_offset(torch, x_ct[:, :L], 0)
    y = torch.full((64,), 0x5A, dtype=torch.int8, device="cuda")
    ws = torch.full((lib.windows_workspace(L) + 64,), 0x5A, dtype=torch.int8, device="cuda")
    for layout in (0, 1):
        rc = lib.load().net_model_compute_windows(x.data_ptr(), layout, L, 1, y.data_ptr(), ws.data_ptr(),
                                                  lib.windows_workspace(L), 0, None)
        assert rc == lib.NET_OK
    torch.cuda.synchronize()
    assert bool((y == 0x5A).all()) and bool((ws == 0x5A).all())
    assert lib.forward_windows_torch(x, 1).shape == (0, N)


_VARIANTS = [dict(reorder_bn=False), dict(clip_balanced=True), dict(weight_bits=4), dict(stress=True),
             dict(extreme=0), dict(extreme=3)]


@pytest.mark.parametrize("kw", _VARIANTS, ids=lambda kw: "-".join(f"{k}={v}" for k, v in kw.items()))
@pytest.mark.parametrize("C,T,N", [(38, 480, 2), (22, 1125, 4)])
def test_variants(C, T, N, kw, gpu):
    """Both BN branches, both clips, int4 weights, stress ranges and the out-of-envelope sets
    (folded to the float kernels at mids = 0, exact division at mids = 3), on a general and on a
    compiled geometry."""
    if "extreme" in kw:
        ps = ParamSet.synthetic_extreme(seed=C + T, C=C, T=T, N=N, mids=kw["extreme"])
    else:
        ps = ParamSet.synthetic(seed=C + T, C=C, T=T, N=N, **kw)
    lib.params_load(ps)
    if "extreme" in kw:
        assert lib.params_info()["exact_division"] == (kw["extreme"] > 0)
    hop, W = 9, 29
    _check_windows(ps, recording(ps, T + (W - 1) * hop + 4, C + len(kw)), hop, offset=2)


@pytest.mark.parametrize("C,T,N,layout", [(19, 480, 3, 1), (19, 480, 3, 0), (22, 1125, 4, 1), (64, 513, 2, 0)])
def test_workspace(C, T, N, layout, gpu):
    """The workspace is the reference's layer-1 output of the whole recording, zero from L to the
    row stride, and neither it nor the logits are written past their ends."""
    import torch

    ps = ParamSet.synthetic(seed=C + T + N, C=C, T=T, N=N)
    lib.params_load(ps)
    co = oracle.COracle(ps)
    d = ps.dims
    hop = 11
    L = T + 20 * hop + 3
    x_ct = recording(ps, L, L)
    W = lib.windows_count(L, hop)
    wsb, rs = lib.windows_workspace(L), lib.windows_row_stride(L)
    x = at_offset(torch, x_ct if layout == 1 else x_ct.T, 3)
    y = torch.full((W * N + 64,), 0x5A, dtype=torch.int8, device="cuda")
    ws = torch.full((wsb + 64,), 0x5A, dtype=torch.int8, device="cuda")
    rc = lib.load().net_model_compute_windows(x.data_ptr(), layout, L, hop, y.data_ptr(), ws.data_ptr(), wsb, 0, None)
    assert rc == lib.NET_OK
    torch.cuda.synchronize()
    assert bool((y[W * N:] == 0x5A).all()) and bool((ws[wsb:] == 0x5A).all())
    y1 = ws[:wsb].view(16, rs).cpu().numpy()
    for s in (0, 5, L - T):
        want = co.layer1(oracle.to_tc_align(x_ct[:, s: s + T], d.C_ALIGN))[:, :T]
        np.testing.assert_array_equal(y1[:, s: s + T], want, err_msg=f"workspace at {s}")
    assert not y1[:, L:].any()
    want = co.batch(pack_trials(sliding_windows(x_ct, T, hop)), nthreads=NTH)
    np.testing.assert_array_equal(y[: W * N].view(W, N).cpu().numpy(), want)
    # the Python entry returns the same workspace
    y2, ws2 = lib.forward_windows_torch(x, hop, layout="ct" if layout == 1 else "tc", return_y1=True)
    assert tuple(ws2.shape) == (16, rs)
    np.testing.assert_array_equal(ws2.cpu().numpy()[:, :L], y1[:, :L])
    np.testing.assert_array_equal(y2.cpu().numpy(), want)


@pytest.mark.parametrize("layout", ["tc", "ct"])
def test_recording_at_the_offset_limit(layout, gpu):
    """A recording one sample short of the 32-bit offset limit (L C = 2^31 - 2 bytes, a partial
    last block): its first and last windows and the workspace under the last one."""
    import torch

    ps = ParamSet.synthetic(seed=29)
    lib.params_load(ps)
    C, T = 22, 1125
    L = (2**31 - 1) // C
    assert L * C < 2**31 <= (L + 1) * C and L % 16 != 0
    hop = L - T
    assert lib.windows_count(L, hop) == 2
    g = torch.Generator(device="cuda").manual_seed(29)
    shape = (L, C) if layout == "tc" else (C, L)
    x = torch.randint(-128, 128, shape, dtype=torch.int8, device="cuda", generator=g)
    first = (x[:T].T if layout == "tc" else x[:, :T]).cpu().numpy()
    last = (x[L - T:].T if layout == "tc" else x[:, L - T:]).cpu().numpy()
    y, ws = lib.forward_windows_torch(x, hop, layout=layout, return_y1=True)
    co = oracle.COracle(ps)
    want = co.batch(pack_trials(np.stack([first, last])), nthreads=2)
    np.testing.assert_array_equal(y.cpu().numpy(), want)
    y1_last = co.layer1(oracle.to_tc_align(last, ps.dims.C_ALIGN))[:, :T]
    np.testing.assert_array_equal(ws[:, L - T: L].cpu().numpy(), y1_last)
    assert not bool(ws[:, L:].any())
    del x, ws
    torch.cuda.empty_cache()


def test_python_entries_reject_wrong_tensors(gpu):
    """forward_windows_torch / forward_windows_f32_torch check what the C ABI cannot see: element
    type, orientation, channel count, contiguity, the layout name and the hop."""
    import torch

    ps = ParamSet.synthetic(seed=19, C=19, T=480, N=3)
    lib.params_load(ps)
    good = torch.zeros((19, 600), dtype=torch.int8, device="cuda")
    assert lib.forward_windows_torch(good, 8).shape == (16, 3)
    assert lib.forward_windows_torch(good.T.contiguous(), 8, layout="tc").shape == (16, 3)
    bad = [
        (good.to(torch.int16), dict()),                         # element type
        (good.to(torch.float32), dict()),
        (good.cpu(), dict()),                                   # not on the device
        (good.T.contiguous(), dict()),                          # [L][C] passed as "ct"
        (good, dict(layout="tc")),                              # [C][L] passed as "tc"
        (torch.zeros((20, 600), dtype=torch.int8, device="cuda"), dict()),   # channel count
        (torch.zeros((2, 19, 600), dtype=torch.int8, device="cuda"), dict()),  # a batch, not a recording
        (torch.zeros((19, 1200), dtype=torch.int8, device="cuda")[:, ::2], dict()),  # strided
        (good.T, dict()),                                       # [C][L] view of an [L][C] buffer
        (good, dict(layout="xx")),
    ]
    for x, kw in bad:
        with pytest.raises(ValueError):
            lib.forward_windows_torch(x, 8, **kw)
    for hop in (0, -3):
        with pytest.raises(ValueError):
            lib.forward_windows_torch(good, hop)
        with pytest.raises(ValueError):
            lib.forward_windows_f32_torch(good.to(torch.float32), hop, 1.0)
    for x in (good, good.to(torch.float64), good.to(torch.float32).cpu(),
              torch.zeros((600, 19), dtype=torch.float32, device="cuda")):
        with pytest.raises(ValueError):
            lib.forward_windows_f32_torch(x, 8, 1.0)
    assert lib.forward_windows_f32_torch(good.to(torch.float32), 8, 1.0).shape == (16, 3)


def test_image_lifetime_and_graph_replay(gpu):
    """Each loaded set keeps its own device copy of the window kernels' image: a reload of a set
    reuses its copy, and a captured windows call keeps replaying the set it was captured with."""
    import torch

    ps_a = ParamSet.synthetic(seed=61)
    ps_b = ParamSet.synthetic(seed=62, reorder_bn=False, clip_balanced=True)
    hop, W = 5, 47
    L = 1125 + (W - 1) * hop
    x_ct = recording(ps_a, L, 61)
    packed = pack_trials(sliding_windows(x_ct, 1125, hop))
    want_a = oracle.COracle(ps_a).batch(packed, nthreads=NTH)
    want_b = oracle.COracle(ps_b).batch(packed, nthreads=NTH)
    assert not np.array_equal(want_a, want_b)
    x = at_offset(torch, x_ct, 1)
    lib.params_load(ps_a)
    np.testing.assert_array_equal(lib.forward_windows_torch(x, hop).cpu().numpy(), want_a)
    lib.params_load(ps_b)
    np.testing.assert_array_equal(lib.forward_windows_torch(x, hop).cpu().numpy(), want_b)
    up = lib.upload_stats()[0]
    lib.params_load(ps_a)
    np.testing.assert_array_equal(lib.forward_windows_torch(x, hop).cpu().numpy(), want_a)
    assert lib.upload_stats()[0] == up  # A's copy was still there
    # capture on a side stream (a linear graph; the eager call above uploaded the parameters)
    y = torch.zeros((W, 4), dtype=torch.int8, device="cuda")
    ws = torch.zeros((lib.windows_workspace(L),), dtype=torch.int8, device="cuda")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            rc = lib.load().net_model_compute_windows(x.data_ptr(), 1, L, hop, y.data_ptr(), ws.data_ptr(), ws.numel(),
                                                      0, s.cuda_stream)
    assert rc == lib.NET_OK
    g.replay()
    torch.cuda.synchronize()
    np.testing.assert_array_equal(y.cpu().numpy(), want_a)
    lib.params_load(ps_b)
    np.testing.assert_array_equal(lib.forward_windows_torch(x, hop).cpu().numpy(), want_b)
    y.zero_()
    ws.zero_()
    g.replay()
    torch.cuda.synchronize()
    np.testing.assert_array_equal(y.cpu().numpy(), want_a)
    del g
