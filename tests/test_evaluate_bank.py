"""evaluate.evaluate_bank: many networks scored on one labelled set in one bank call, against one
evaluate call per network on that network's trials."""
import numpy as np
import pytest

from mibminet import evaluate as E
from mibminet import lib
from mibminet.params import ParamSet

pytestmark = pytest.mark.gpu


def _signals(rng, n, C, T):
    """Per-channel sinusoids plus noise (tests/test_evaluate.py): they move the synthetic networks'
    logits enough to give several classes."""
    t = np.arange(T)
    f = rng.uniform(0.002, 0.05, (n, C, 1))
    ph = rng.uniform(0, 2 * np.pi, (n, C, 1))
    amp = rng.uniform(0, 3, (n, C, 1))
    return (amp * np.sin(2 * np.pi * f * t + ph) + rng.normal(0, 0.3, (n, C, T))).astype(np.float32)


@pytest.mark.parametrize("grouped", [True, False])
def test_evaluate_bank_gives_the_classes_of_one_evaluate_per_set(gpu, grouped):
    C, T, N, n = 22, 1125, 4, 90
    rng = np.random.default_rng(17)
    # seeds whose networks give at least two classes on these signals (101 and 102 give one)
    sets = [ParamSet.synthetic(seed=s, C=C, T=T, N=N) for s in (2, 6, 103)]
    scales = [2.0, 1.75, 2.5]
    samples, labels = _signals(rng, n, C, T), rng.integers(0, N, size=n)
    set_of = np.sort(rng.integers(0, 3, size=n)) if grouped else rng.integers(0, 3, size=n)
    single = [E.evaluate(sets[s], samples[set_of == s], labels[set_of == s], scales[s]) for s in range(3)]
    assert len({tuple(map(tuple, r["confusion"])) for r in single}) == 3  # the three networks differ
    assert all((np.asarray(r["confusion"]).sum(axis=0) > 0).sum() >= 2 for r in single)  # none collapses
    lib.params_unload()
    got = E.evaluate_bank(sets, scales, samples, labels, set_of)
    assert got["per_set"] == single
    assert got["n"] == n and got["correct"] == sum(r["correct"] for r in single)
    assert got["accuracy"] == got["correct"] / n
    np.testing.assert_array_equal(np.asarray(got["confusion"]), sum(np.asarray(r["confusion"]) for r in single))
    assert lib.params_dims() == {}  # no set was loaded for it
    with pytest.raises(ValueError):
        E.evaluate_bank(sets, scales, samples, labels, set_of[:-1])
    with pytest.raises(ValueError):
        E.evaluate_bank(sets, scales, samples, labels, np.full(n, 3))
