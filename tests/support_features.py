"""What the test modules of the feature-returning entries and of net_bank_replace share
(tests/test_bank_replace_cpu.py, tests/test_gpu_features.py, tests/test_gpu_bank_replace.py): the
reference of a feature row and the sets that replace one.

The reference of a feature row is the C oracle's single-trial chain layer1 .. layer3_flip, layer4 on
the materialised item, with the T64_ALIGN pad columns dropped; the chain is held to the oracle's own
model on every item (layer5 of the row it returns is model's logits), and the logits' reference stays
support.want.  Nothing here comes from a GPU entry."""
import functools

import numpy as np

import oracle
import support_bank as sb
from mibminet.params import ParamSet

E = 23          # the epochs of support_bank.case the GPU tests use
SLOT = 2        # the slot the replacement tests replace
NEW_SEED = 106  # the unrelated set that goes into it (support_bank's are 101 .. 105)
# the geometries of the replacement tests: minimum T, and tail tiles
REPLACE_GEOMETRIES = [(8, 64, 2), (19, 480, 3)]


def features(ps, trials_ct):
    """([B][16][T64] int8, [B][N] int8): the oracle's layer-4 output of every trial [C][T] with the pad
    columns dropped, and its logits.  layer5 of each row must be what model returns for the trial."""
    d = ps.dims
    orc = oracle.COracle(ps)
    feat = np.zeros((len(trials_ct), d.F2, d.T64), np.int8)
    logits = np.zeros((len(trials_ct), d.N), np.int8)
    for b, x in enumerate(trials_ct):
        xa = oracle.to_tc_align(x, d.C_ALIGN)
        y4 = orc.layer4(orc.layer3_flip(orc.layer3(orc.layer2(orc.layer1(xa)))))
        logits[b] = orc.model(xa)
        assert np.array_equal(orc.layer5(y4), logits[b]), b
        feat[b] = y4[:, : d.T64]
    return feat, logits


@functools.lru_cache(maxsize=None)
def table(C, T, N, variant=None):
    """([set][E][16][T64], [set][E][N]): features and logits of the first E epochs of
    support_bank.case(C, T) under each of the five sets (of the named variant).  Computed once,
    read-only."""
    sets = sb.sets(C, T, N) if variant is None else sb.VARIANTS[variant](C, T, N)
    both = [features(ps, sb.epochs(C, T)[:E]) for ps in sets]
    f, y = np.stack([b[0] for b in both]), np.stack([b[1] for b in both])
    f.setflags(write=False)
    y.setflags(write=False)
    return f, y


def reference(tab, set_of):
    """Row e of the result: the row of epoch e under set set_of[e] (support_bank.reference)."""
    return sb.reference(tab, set_of)


@functools.lru_cache(maxsize=None)
def new_set(C, T, N):
    """The unrelated set that replaces slot SLOT."""
    return ParamSet.synthetic(seed=NEW_SEED, C=C, T=T, N=N)


@functools.lru_cache(maxsize=None)
def head_set(C, T, N):
    """Slot SLOT's set with the head (layer 5) of set 3: layers 1-4, and with them every ring, stay."""
    s = sb.sets(C, T, N)
    return sb.hybrid(s[SLOT], s[3], 5)
