"""Windows at given onsets and the sliding windows of many recordings in one call
(net_model_compute_windows_at, win::k_forward_y1_at; forward_windows_multi_torch): logit row i must
be byte-identical to the forward of the materialised trial x[:, onsets[i] : onsets[i] + T].

The reference is always the C oracle on gathered trials (-> [W][C][T] -> pack_trials ->
COracle.batch); the existing entries (forward_windows_torch, forward_ct_torch) are a second
witness.  Inputs are uniform int8 from seeded generators.
"""
import numpy as np
import pytest

import oracle
from mibminet import lib
from mibminet.params import ParamSet, pack_trials
from support import _BAD, NTH, at_offset, float_recording, length, recording, tile_sweep, want, windows_at

pytestmark = pytest.mark.gpu


def _want_at(ps, x_ct, onsets):
    return want(ps, windows_at(x_ct, onsets, ps.dims.T))


def _check_at(ps, x_ct, onsets, offset=0, layouts=("ct", "tc"), witness=False):
    """Both int8 layouts of recording x_ct at `onsets` against the oracle (and forward_ct_torch) on
    the gathered windows.  The set must be loaded.  Returns the expected logits."""
    import torch

    want = _want_at(ps, x_ct, onsets)
    if witness:
        full = lib.forward_ct_torch(torch.from_numpy(windows_at(x_ct, onsets, ps.dims.T)).cuda()).cpu().numpy()
        np.testing.assert_array_equal(full, want, err_msg="forward_ct_torch vs oracle")
    for layout in layouts:
        x = at_offset(torch, x_ct if layout == "ct" else x_ct.T, offset)
        got = lib.forward_windows_at_torch(x, onsets, layout=layout).cpu().numpy()
        assert got.shape == (len(onsets), ps.dims.N)
        np.testing.assert_array_equal(got, want, err_msg=f"{layout} offset {offset}")
    return want


def _irregular(L, T, n, seed):
    """n unsorted onsets in 0 .. L - T with duplicates, 0 and L - T among them."""
    on = [int(v) for v in np.random.default_rng(seed).integers(0, L - T + 1, size=n)]
    on[1], on[n // 2], on[n - 1], on[n - 2] = L - T, 0, on[0], L - T
    return on


@pytest.mark.parametrize("hop", [1, 3, 16])
def test_regular_onsets_equal_the_regular_entry(hop, gpu):
    """onsets = arange(W) hop: byte-identical to forward_windows_torch and to the oracle, in both
    int8 layouts and float32 with non-finite samples planted."""
    import torch

    ps = ParamSet.synthetic(seed=19, C=19, T=480, N=3)
    lib.params_load(ps)
    assert lib.params_info()["path"] == "general"
    d = ps.dims
    L = length(d.T, hop, (5 * hop) % 16)
    W = lib.windows_count(L, hop)
    assert 40 <= W <= 56
    onsets = (np.arange(W, dtype=np.int64) * hop).tolist()
    x_ct = recording(ps, L, 77 + hop)
    want = _check_at(ps, x_ct, onsets, offset=hop % 4, witness=True)
    for layout in ("ct", "tc"):
        x = at_offset(torch, x_ct if layout == "ct" else x_ct.T, 1)
        reg = lib.forward_windows_torch(x, hop, layout=layout)
        got = lib.forward_windows_at_torch(x, torch.arange(W, dtype=torch.int64, device="cuda") * hop, layout=layout)
        assert bool((reg == got).all())
        np.testing.assert_array_equal(got.cpu().numpy(), want)
    xf, q_ct = float_recording(torch, d.C, L, 4 * (hop % 2), L)
    want_f = _want_at(ps, q_ct, onsets)
    got_f = lib.forward_windows_at_torch(xf, onsets, scale=3.0)
    np.testing.assert_array_equal(got_f.cpu().numpy(), want_f, err_msg="f32")
    assert bool((got_f == lib.forward_windows_f32_torch(xf, hop, 3.0)).all())


@pytest.mark.parametrize("extra", [100, 96, 97, 111])
def test_arbitrary_onsets(extra, gpu):
    """64 unsorted onsets with duplicates over every residue mod 16, 0 and L - T among them, the
    recording 1-3 bytes into its allocation, L = T + 100 and L % 16 in {0, 1, 15}; the workspace
    is the one the regular entry leaves."""
    import torch

    ps = ParamSet.synthetic(seed=19, C=19, T=480, N=3)
    lib.params_load(ps)
    T = 480
    L = T + extra
    assert extra == 100 or L % 16 in (0, 1, 15)
    rng = np.random.default_rng(extra)
    base = int(rng.integers(1, extra - 50))
    onsets = [0, L - T, L - T, 0] + [int(v) for v in rng.permutation(np.arange(base, base + 48))]  # 48 consecutive
    onsets += [int(v) for v in rng.integers(0, L - T + 1, size=12)]
    assert len(onsets) == 64 and {o % 16 for o in onsets} == set(range(16)) and len(set(onsets)) < 64
    assert onsets != sorted(onsets) and min(onsets) == 0 and max(onsets) == L - T
    x_ct = recording(ps, L, L)
    for offset in (1, 2, 3):
        _check_at(ps, x_ct, onsets, offset=offset, witness=offset == 1)
    x = at_offset(torch, x_ct, 1 + extra % 3)
    y, ws = lib.forward_windows_at_torch(x, onsets, return_y1=True)
    y_reg, ws_reg = lib.forward_windows_torch(x, 1, return_y1=True)
    assert tuple(ws.shape) == (16, lib.windows_row_stride(L)) and bool((ws == ws_reg).all())
    assert bool((y == y_reg[torch.tensor(onsets, device="cuda")]).all())
    # float32, the same onsets
    xf, q_ct = float_recording(torch, 19, L, 4, L)
    got_f = lib.forward_windows_at_torch(xf, onsets, scale=3.0).cpu().numpy()
    np.testing.assert_array_equal(got_f, _want_at(ps, q_ct, onsets))


_EDGES = [(1, 64, 1, {}), (5, 100, 16, {}), (64, 513, 2, {})] + [tile_sweep()[r] for r in (0, 1, 16, 17)]


@pytest.mark.parametrize("C,T,N,kw", _EDGES)
def test_edges(C, T, N, kw, gpu):
    """One channel, one and sixteen classes, the shortest T, T = 1 mod 16, layer 2's tile residues
    0, 1, 16 and 17: the onsets {L - T, 0, 7}, and the single onset 0 of a recording with L == T."""
    ps = ParamSet.synthetic(seed=C * T + N, C=C, T=T, N=N, **kw)
    lib.params_load(ps)
    L = T + 37
    x_ct = recording(ps, L, C + T)
    _check_at(ps, x_ct, [L - T, 0, 7], offset=1)
    _check_at(ps, x_ct[:, :T], [0], offset=2)  # L == T


def test_persistent_loop_with_invalid_onsets(gpu):
    """More windows than resident workgroups (two or three passes each), every seventh onset
    invalid, among them values whose low 32 bits would be valid: their rows are zero, n_bad counts
    them exactly, every other row matches the oracle and nothing is written past y or the
    workspace."""
    import torch

    ps = ParamSet.synthetic(seed=41, C=5, T=64, N=3)
    lib.params_load(ps)
    T, N, W = 64, 3, 1300
    L = T + W - 1
    last = L - T
    grid = 2 * torch.cuda.get_device_properties(0).multi_processor_count  # at most two workgroups per CU
    assert W > grid
    onsets = [int(v) for v in np.random.default_rng(41).permutation(W)]  # every onset 0 .. L - T once
    bad = list(range(0, W, 7))
    for j, i in enumerate(bad):
        v = _BAD[j % 7]
        onsets[i] = last + 1 if v is None else v
    # the low 32 bits of 2^32, 2^32 + 5 and INT64_MIN are valid onsets: the check must see 64 bits
    assert all(0 <= (v & 0xFFFFFFFF) <= last for v in (2**32, 2**32 + 5, -(2**63)))
    # invalid entries on a workgroup's first pass, on its last (the pass before the one that only
    # finishes) and on one in between
    assert bad[0] < grid and bad[-1] + grid >= W and any(grid <= i < W - grid for i in bad)
    ok = [i for i in range(W) if i % 7]
    x_ct = recording(ps, L, 41)
    want = _want_at(ps, x_ct, [onsets[i] for i in ok])
    x = at_offset(torch, x_ct, 3)
    on = torch.tensor(onsets, dtype=torch.int64, device="cuda")
    wsb = lib.windows_workspace(L)
    y = torch.full((W * N + 64,), 0x5A, dtype=torch.int8, device="cuda")
    ws = torch.full((wsb + 64,), 0x5A, dtype=torch.int8, device="cuda")
    nb = torch.zeros((3,), dtype=torch.int32, device="cuda")
    rc = lib.load().net_model_compute_windows_at(x.data_ptr(), 1, L, on.data_ptr(), W, y.data_ptr(), nb.data_ptr() + 4,
                                                 ws.data_ptr(), wsb, 0, None)
    assert rc == lib.NET_OK
    torch.cuda.synchronize()
    assert nb.cpu().tolist() == [0, len(bad), 0]
    assert bool((y[W * N:] == 0x5A).all()) and bool((ws[wsb:] == 0x5A).all())
    rows = y[: W * N].view(W, N).cpu().numpy()
    np.testing.assert_array_equal(rows[ok], want)
    assert not rows[bad].any()
    assert want.any(axis=1).sum() > len(ok) // 2  # the valid rows are not zero themselves
    # n_bad == NULL: the same rows, nothing counted
    got = lib.forward_windows_at_torch(x, on, check=False).cpu().numpy()
    np.testing.assert_array_equal(got, rows)
    with pytest.raises(ValueError, match=f"{len(bad)} of {W}"):
        lib.forward_windows_at_torch(x, on)
    # no window: nothing is written
    assert lib.forward_windows_at_torch(x, []).shape == (0, N)


_LENGTHS = [480 + 5 * 7 + 3, 0, 479, 480, 487, 961]


@pytest.mark.parametrize("kind", ["ct", "tc", "f32"])
def test_many_recordings(kind, gpu):
    """Six recordings (one empty, one a sample short, one exactly T) as a list and as one
    concatenated tensor with lengths, in one chunk and in three: the per-recording
    forward_windows_torch results concatenated, and the oracle's."""
    import torch

    ps = ParamSet.synthetic(seed=19, C=19, T=480, N=3)
    lib.params_load(ps)
    T, hop = 480, 7
    total = sum(_LENGTHS)
    bounds = np.concatenate(([0], np.cumsum(_LENGTHS))).tolist()
    on_want, first_want = [], [0]
    for r, n in enumerate(_LENGTHS):
        on_want += [bounds[r] + k * hop for k in range(lib.windows_count(n, hop))]
        first_want.append(len(on_want))
    assert first_want == [0, 6, 6, 6, 7, 9, 78]
    layout, scale = ("tc", None) if kind == "tc" else ("ct", 3.0 if kind == "f32" else None)
    if kind == "f32":
        cat, q_ct = float_recording(torch, 19, total, 0, 5)
        single = lambda t: lib.forward_windows_f32_torch(t, hop, 3.0)
    else:
        q_ct = recording(ps, total, 5)
        cat = torch.from_numpy(np.ascontiguousarray(q_ct if kind == "ct" else q_ct.T)).cuda()
        single = lambda t: lib.forward_windows_torch(t, hop, layout=layout)
    axis = 1 if layout == "ct" else 0
    recs = [cat.narrow(axis, bounds[r], n).contiguous() for r, n in enumerate(_LENGTHS)]
    want = _want_at(ps, q_ct, on_want)
    per_rec = torch.cat([single(t) for t in recs], dim=0)
    np.testing.assert_array_equal(per_rec.cpu().numpy(), want)
    per = max(16, 19 * (4 if kind == "f32" else 1))
    assert lib._plan_chunks(_LENGTHS, per, 1000 * per) == [(0, 3), (3, 5), (5, 6)]
    for rec in (recs, (cat, _LENGTHS)):
        for max_bytes in (None, 1000 * per):
            y, first = lib.forward_windows_multi_torch(rec, hop, layout=layout, scale=scale, max_bytes=max_bytes)
            assert first == first_want and tuple(y.shape) == (78, 3)
            assert bool((y == per_rec).all())
    with pytest.raises(ValueError, match="overlap"):
        lib.forward_windows_multi_torch(recs, hop, layout=layout, scale=scale, max_bytes=961 * per)


_VARIANTS = [dict(reorder_bn=False), dict(clip_balanced=True), dict(weight_bits=4), dict(extreme=0), dict(extreme=3)]


@pytest.mark.parametrize("kw", _VARIANTS, ids=lambda kw: "-".join(f"{k}={v}" for k, v in kw.items()))
@pytest.mark.parametrize("C,T,N", [(38, 480, 2), (22, 1125, 4)])
def test_variants(C, T, N, kw, gpu):
    """Both BN branches, both clips, int4 weights and the out-of-envelope sets (folded to the float
    kernels at mids = 0, exact division at mids = 3), on a general and on a compiled geometry, 29
    irregular onsets."""
    if "extreme" in kw:
        ps = ParamSet.synthetic_extreme(seed=C + T, C=C, T=T, N=N, mids=kw["extreme"])
    else:
        ps = ParamSet.synthetic(seed=C + T, C=C, T=T, N=N, **kw)
    lib.params_load(ps)
    if "extreme" in kw:
        assert lib.params_info()["exact_division"] == (kw["extreme"] > 0)
    L = T + 260
    _check_at(ps, recording(ps, L, C + len(kw)), _irregular(L, T, 29, C + T), offset=2)


@pytest.mark.parametrize("C,T", [(22, 1125), (64, 1000), (64, 480)])
def test_compiled_geometries(C, T, gpu):
    """The compiled geometries run the new kernel through the window kernels' parameter image; the
    compiled kernels and what net_params_info reports stay as they were."""
    import torch

    ps = ParamSet.synthetic(seed=C + T, C=C, T=T)
    lib.params_load(ps)
    info = lib.params_info()
    assert info["path"] == "float"
    L = T + 231
    _check_at(ps, recording(ps, L, C * T), _irregular(L, T, 33, T), offset=1, witness=True)
    assert lib.params_info() == info
    xp = pack_trials(np.random.default_rng(T).integers(-128, 128, size=(41, C, T)))
    got = lib.forward_torch(torch.from_numpy(xp).cuda()).cpu().numpy()
    np.testing.assert_array_equal(got, oracle.COracle(ps).batch(xp, nthreads=NTH))


def test_graph_capture_and_replay(gpu):
    """One eager call uploads the parameters; a captured net_model_compute_windows_at (a linear
    graph on a side stream) then keeps replaying the set it was captured with, after a reload of
    another set too."""
    import torch

    ps_a = ParamSet.synthetic(seed=61)
    ps_b = ParamSet.synthetic(seed=62, reorder_bn=False, clip_balanced=True)
    T, W = 1125, 47
    L = T + 300
    onsets = _irregular(L, T, W, 61)
    x_ct = recording(ps_a, L, 61)
    want_a, want_b = _want_at(ps_a, x_ct, onsets), _want_at(ps_b, x_ct, onsets)
    assert not np.array_equal(want_a, want_b)
    x = at_offset(torch, x_ct, 1)
    on = torch.tensor(onsets, dtype=torch.int64, device="cuda")
    lib.params_load(ps_b)
    np.testing.assert_array_equal(lib.forward_windows_at_torch(x, on).cpu().numpy(), want_b)
    lib.params_load(ps_a)
    np.testing.assert_array_equal(lib.forward_windows_at_torch(x, on).cpu().numpy(), want_a)  # eager: uploads
    y = torch.zeros((W, 4), dtype=torch.int8, device="cuda")
    nb = torch.zeros((1,), dtype=torch.int32, device="cuda")
    ws = torch.zeros((lib.windows_workspace(L),), dtype=torch.int8, device="cuda")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            rc = lib.load().net_model_compute_windows_at(x.data_ptr(), 1, L, on.data_ptr(), W, y.data_ptr(),
                                                         nb.data_ptr(), ws.data_ptr(), ws.numel(), 0, s.cuda_stream)
    assert rc == lib.NET_OK
    g.replay()
    torch.cuda.synchronize()
    np.testing.assert_array_equal(y.cpu().numpy(), want_a)
    lib.params_load(ps_b)
    np.testing.assert_array_equal(lib.forward_windows_at_torch(x, on).cpu().numpy(), want_b)
    y.zero_()
    ws.zero_()
    g.replay()
    torch.cuda.synchronize()
    np.testing.assert_array_equal(y.cpu().numpy(), want_a)
    assert int(nb.item()) == 0
    del g
