"""net_bank_replace without a GPU (no device holds a copy of these banks, so only the host master is
at stake): what it refuses, each refusal leaving every set's image and net_bank_info as they were;
what it accepts, the new image held to the image that slot has in a bank freshly created with the new
list; ParamSet.with_head; the feature entries' own argument check; and the certification of the inputs
of tests/test_gpu_features.py and tests/test_gpu_bank_replace.py."""
import ctypes

import numpy as np
import pytest

import support_bank as sb
import support_features as sf
from mibminet import lib
from mibminet.params import ParamSet
from support import want

INV, RNG, UNS, BLOB, OK = lib.NET_ERR_INVALID, lib.NET_ERR_RANGE, lib.NET_ERR_UNSUPPORTED, lib.NET_ERR_BLOB, lib.NET_OK
C, T, N = 19, 480, 3
S, X = ParamSet.synthetic, ParamSet.synthetic_extreme


def _state(bank):
    return [bank.image(s) for s in range(bank.n_sets)], bank.info()


def _refused(bank, s, new, scale=None):
    before = _state(bank)
    with pytest.raises(lib.NetError) as e:
        bank.replace(s, new, scale)
    assert _state(bank) == before, "a refused replacement changed the bank"
    assert bank.device_copies() == 0
    return e.value.code


def _raw(bank_handle, s, blob, scale=0.0, device=0):
    buf = None if blob is None else ctypes.create_string_buffer(blob, len(blob))
    return lib.load().net_bank_replace(bank_handle, s, buf, 0 if blob is None else len(blob), scale, device, None)


def test_refusals_leave_the_bank_as_it_was():
    sets = sb.sets(C, T, N)
    good = S(seed=sf.NEW_SEED, C=C, T=T, N=N)
    blob = good.to_blob()
    with lib.Bank(sets) as bank:
        assert not bank.exact_division
        assert _refused(bank, 5, good) == INV and _refused(bank, 2**40, good) == INV      # a bad index
        assert _refused(bank, 2, blob[:-4]) == BLOB                                      # malformed
        assert _refused(bank, 2, b"MIBMINET" + bytes(56)) == BLOB
        assert _refused(bank, 2, S(seed=9, C=C, T=T, N=N + 1)) == UNS                    # N + 1 classes
        assert _refused(bank, 2, S(seed=9, C=C, T=T + 8, N=N)) == UNS
        assert _refused(bank, 2, S(seed=9, C=C + 1, T=T, N=N)) == UNS
        assert _refused(bank, 2, S(seed=9, C=C, T=T, N=N, reorder_bn=False)) == UNS      # plain BN into a canonical bank
        assert _refused(bank, 2, S(seed=9, C=C, T=T, N=N, clip_balanced=True)) == UNS
        assert _refused(bank, 2, S(seed=9, C=65, T=T, N=N)) == UNS                       # outside the family: its own code
        assert _refused(bank, 2, X(seed=77, C=C, T=T, N=N, mids=3)) == UNS               # exact division into a float bank
        before = _state(bank)
        assert _raw(None, 2, blob) == INV
        assert _raw(bank.handle, 2, None) == INV
        assert _raw(bank.handle, 2, blob, device=-1) == INV and _raw(bank.handle, 2, blob, device=1 << 20) == INV
        assert _state(bank) == before
        # without scales the scale is ignored, whatever it is
        assert _raw(bank.handle, 2, blob, scale=float("nan")) == OK
        assert bank.image(2) != before[0][2] and bank.info() == before[1]
    with lib.Bank(sets, [1.0, 2.0, 3.0, 4.0, 5.0]) as bank:
        for scale, code in ((0.0, INV), (-1.0, INV), (float("nan"), INV), (float("inf"), INV), (1e-30, RNG), (2.0**61, RNG)):
            assert _refused(bank, 2, good, scale) == code, scale
        with pytest.raises(ValueError):
            bank.replace(2, good)  # the bank has scales: the set needs one
        # a bad blob and a bad scale: the blob's code comes first; a mismatch before the scale
        assert _refused(bank, 2, blob[:100], 0.0) == BLOB
        assert _refused(bank, 2, S(seed=9, C=C, T=T, N=N + 1), 0.0) == UNS
        bank.replace(2, good, 2.0**-60)
        bank.replace(2, good, 2.0**60)


def _fresh(param_sets, s, scales=None):
    with lib.Bank(param_sets, scales) as b:
        return b.image(s), b.info()


def test_a_replaced_slot_is_the_slot_of_a_fresh_bank():
    sets = list(sb.sets(C, T, N))
    new, head = sf.new_set(C, T, N), sf.head_set(C, T, N)
    with lib.Bank(sets) as bank:
        others = {s: bank.image(s) for s in range(5)}
        info = bank.info()
        bank.replace(2, new)
        assert bank.image(2) == _fresh(sets[:2] + [new] + sets[3:], 2)[0] != others[2]
        assert all(bank.image(s) == others[s] for s in (0, 1, 3, 4)) and bank.info() == info
        # the same slot again, right away: the second one wins
        bank.replace(2, head)
        bank.replace(2, head.to_blob())
        assert bank.image(2) == _fresh(sets[:2] + [head] + sets[3:], 2)[0]
        # set 0 is replaceable like any other, and the bank is still held to what it was created with
        bank.replace(0, new)
        assert bank.image(0) == _fresh([new] + sets[1:], 0)[0] and bank.image(1) == others[1]
        assert _refused(bank, 1, S(seed=9, C=C, T=T + 8, N=N)) == UNS
        bank.replace(0, sets[0])
        bank.replace(2, sets[2])
        assert [bank.image(s) for s in range(5)] == [others[s] for s in range(5)] and bank.info() == info
        assert bank.device_copies() == 0


def test_an_exact_bank_takes_a_float_set_in_the_exact_form():
    """A float set into the all-exact bank: its image is the promoted image that slot has in a freshly
    created (then mixed) bank, not the one the set gets alone; the bank stays exact.  A set that
    needs exact division goes in as it is; set 0 of a mixed bank too."""
    ex = list(sb.VARIANTS["all-exact"](C, T, N))
    fl = sb.sets(C, T, N)[1]
    with lib.Bank(ex) as bank, lib.Bank([fl]) as alone:
        assert bank.exact_division and not alone.exact_division
        bank.replace(3, fl)
        want_img, want_info = _fresh(ex[:3] + [fl] + ex[4:], 3)
        assert bank.image(3) == want_img != alone.image(0)
        assert bank.info() == want_info and bank.exact_division is True and bank.info()[4] == 1
        bank.replace(0, fl)
        assert bank.image(0) == _fresh([fl] + ex[1:3] + [fl] + ex[4:], 0)[0]
        bank.replace(3, ex[0])
        assert bank.image(3) == _fresh(ex[:3] + [ex[0]] + ex[4:], 3)[0]
        assert _refused(bank, 1, S(seed=9, C=C, T=T, N=N, reorder_bn=False)) == UNS


def test_replacement_installs_the_scale():
    """The scale entry is not in the image: held to a fresh bank through the float entry's check alone
    here (tests/test_gpu_bank_replace.py runs it); the image must not depend on it."""
    sets = list(sb.sets(C, T, N))
    with lib.Bank(sets, [1.0] * 5) as bank:
        bank.replace(2, sf.new_set(C, T, N), 3.0)
        assert bank.image(2) == _fresh(sets[:2] + [sf.new_set(C, T, N)] + sets[3:], 2)[0]
        assert bank.has_scales and bank.info()[5] == 1


def test_with_head_lays_the_rows_out():
    sets = sb.sets(C, T, N)
    a, b = sets[2], sets[3]
    d = a.dims
    w = b.l5_weight.reshape(d.N, d.F2, d.T64_ALIGN)[:, :, : d.T64]
    got = a.with_head(w, b.l5_bias, b.l5_factor)
    assert got.to_blob() == sb.hybrid(a, b, 5).to_blob() == sf.head_set(C, T, N).to_blob()
    assert d.T64 % 4 != 0 and not got.l5_weight.reshape(d.N, d.F2, d.T64_ALIGN)[:, :, d.T64:].any()
    assert a.with_head(w.astype(np.int64), b.l5_bias.astype(np.int32), 7).l5_factor == 7
    for bad in (lambda: a.with_head(w[:, :, :-1], b.l5_bias, 1), lambda: a.with_head(w, b.l5_bias[:-1], 1),
                lambda: a.with_head(w.astype(np.int32) + 300, b.l5_bias, 1), lambda: a.with_head(w.astype(np.float32), b.l5_bias, 1),
                lambda: a.with_head(w, b.l5_bias, 0)):
        with pytest.raises(ValueError):
            bad()


def test_feature_entries_check_their_buffer():
    """feat stands beside y: NULL with E > 0, or not 16-byte aligned, is NET_ERR_INVALID before any
    device call; E == 0 touches nothing."""
    buf = np.zeros(256, np.uint8)
    a = (buf.ctypes.data + 15) // 16 * 16
    x, on, y, nb, so, feat = a, a + 16, a + 32, a + 48, a + 64, a + 80
    L = 4000
    with lib.Bank(sb.sets(C, T, N), [1.0] * 5) as bank:
        assert bank.feature_bytes() == 16 * (T // 64) and lib.load().net_bank_feature_bytes(None) == 0
        for fn in (lib.load().net_model_compute_epochs_bank_feat, lib.load().net_model_compute_epochs_bank_feat_f32):
            def call(E=7, y=y, feat=feat, bank=bank.handle, dev=0):
                return fn(bank, x, C * L, L, None, on, so, E, y, feat, nb, dev, None)

            assert call(E=0) == OK and call(E=0, feat=None) == OK and call(E=0, y=None, feat=None) == OK
            assert call(feat=None) == INV and call(y=None) == INV and call(bank=None) == INV
            for off in (1, 2, 4, 8, 15):
                assert call(feat=feat + off) == INV and call(feat=feat + off, E=0) == INV
            assert call(dev=-1) == INV and call(E=2**31 - 65535) == INV
        assert bank.device_copies() == 0
    assert lib.load().net_streams_windows_at_feat(None, None, None, 0, None, None, None, None) == INV


# ---- certification of the GPU tests' inputs -----------------------------------------------------------
@pytest.mark.parametrize("C,T,N", sb.GEOMETRIES)
def test_feature_rows_are_certified(C, T, N):
    """A condition on the inputs, not a measurement.  On the first 23 epochs of support_bank.case no
    reference feature row under any of the five sets is all zeros (what an invalid item writes), the
    share of non-zero bytes is 0.40 .. 0.87 (neither empty nor saturated), the rows of two sets differ
    on every epoch, and the chain's logits are support_bank's."""
    feat, logits = sf.table(C, T, N)
    d = sb.sets(C, T, N)[0].dims
    assert feat.shape == (5, sf.E, 16, d.T64) and np.array_equal(logits, sb.table(C, T, N)[:, : sf.E])
    assert feat.reshape(5, sf.E, -1).any(axis=2).all()
    share = float((feat != 0).mean())
    assert 0.40 <= share <= 0.87, share
    for a in range(5):
        for b in range(a):
            assert (feat[a] != feat[b]).reshape(sf.E, -1).any(axis=1).all(), (a, b)


@pytest.mark.parametrize("variant", ["plain-bn", "all-exact"])
def test_variant_feature_rows_are_certified(variant):
    feat, _ = sf.table(19, 480, 3, variant)
    assert feat.reshape(5, sf.E, -1).any(axis=2).all()


@pytest.mark.parametrize("C,T,N", [(8, 64, 2), (19, 480, 3), (4, 4096, 16)])
def test_replacement_sets_are_certified(C, T, N):
    """The sets that replace slot 2 change the reference logits of every one of the 23 epochs under
    it, so a call that read the old set, or mixed the two, cannot pass; no new row is all zeros.  If
    a seed ever fails this, take the next one."""
    ep, old = sb.epochs(C, T)[: sf.E], sb.table(C, T, N)[sf.SLOT, : sf.E]
    for new in (sf.new_set(C, T, N), sf.head_set(C, T, N)):
        rows = want(new, ep)
        assert (rows != old).any(axis=1).all() and rows.any(axis=1).all()
    # the head-only set shares layers 1-4: its features are slot 2's
    f_old = sf.table(C, T, N)[0][sf.SLOT]
    assert np.array_equal(sf.features(sf.head_set(C, T, N), ep)[0], f_old)
