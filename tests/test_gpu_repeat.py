"""GPU repetition checks: rare, timing-dependent corruption does not show in one call.

The single-workgroup layer-1 path once returned a wrong row in about 2 % of calls on gfx950 while
its fragment loads were still in flight ("A rare layer-1 row fault"); one call per
fixture passed most of the time.  These tests repeat the paths and compare every result.
"""
import os

import numpy as np
import pytest

import oracle
from mibminet import lib
from mibminet.params import ParamSet
from support import NTH

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


def test_layer1_repeated(gpu):
    f = np.load(os.path.join(GOLDEN, "fixture_b22_stress.npz"))
    ps = ParamSet.from_blob(f["blob"].tobytes())
    lib.params_load(ps)
    xa = oracle.to_tc_align(f["x"][0], ps.dims.C_ALIGN)
    bad = [i for i in range(400) if not np.array_equal(lib.net_layer1(xa), f["y1"])]
    assert not bad, f"{len(bad)} of 400 net_layer1 calls differ from the fixture (first: call {bad[0]})"


@pytest.mark.parametrize("stress", [False, True])
def test_batch_repeated_vs_oracle(stress, gpu):
    """B = 65536, 40 launches, every output compared with the oracle's logits."""
    import torch

    B = 65536
    ps = ParamSet.synthetic(seed=11, stress=stress)
    lib.params_load(ps)
    stride = lib.trial_stride()
    g = torch.Generator(device="cuda").manual_seed(5)
    x = torch.randint(-128, 128, (B, stride), dtype=torch.int8, device="cuda", generator=g)
    x[:, 22 * 1125:] = 0
    want = torch.from_numpy(oracle.COracle(ps).batch(x.cpu().numpy(), nthreads=NTH)).cuda()
    y = torch.empty((B, 4), dtype=torch.int8, device="cuda")
    bad = []
    for i in range(40):
        y.fill_(0x55)
        lib.model_compute_batch(x.data_ptr(), y.data_ptr(), B)
        torch.cuda.synchronize()
        n = int((y != want).any(dim=1).sum())
        if n:
            bad.append((i, n))
    assert not bad, f"launches with wrong trials (launch, trials): {bad[:5]}"
