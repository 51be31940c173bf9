"""CPU: adt_seqbatch_draw, the host entry to the inline function adt_seqbatch_build's kernel draws negatives with (include/adt_hip.h;
adt_amd/csrc/adt_seqbatch.cuh).  A pure function of (seed, step, row, t, attempt, item_size), so every check below is deterministic.
Needs only the built library."""
import numpy as np
import pytest

from adt_amd import ops

SEED, STEP = 1234, 17


def draws(seed, step, rows, ts, attempt, item_size):
    return np.array([ops.seqbatch_draw(seed, step, r, t, attempt, item_size) for r in rows for t in ts])


@pytest.mark.parametrize("item_size", [2, 3, 65, 12103])
def test_draw_range(item_size):
    v = np.concatenate([draws(SEED, STEP, range(40), range(25), a, item_size) for a in (0, 1, 31)])
    assert v.min() >= 1 and v.max() <= item_size - 1
    if item_size == 2:
        assert (v == 1).all()
    if item_size in (3, 65):       # 3,000 draws over at most 64 ids: every id turns up
        assert set(v.tolist()) == set(range(1, item_size))


def test_draw_uniform():
    """20,000 draws (200 rows x 100 positions, attempt 0) over the 50 ids of item_size 51: chi-square against the uniform law, below its
    1 - 1e-6 quantile at 49 degrees of freedom (111.1; this seed and step give 49.1)."""
    from scipy.stats import chi2
    v = draws(SEED, STEP, range(200), range(100), 0, 51)
    assert v.size == 20000
    counts = np.bincount(v, minlength=51)
    assert counts[0] == 0
    expect = v.size / 50.0
    stat = float(((counts[1:] - expect) ** 2 / expect).sum())
    print("chi2 = %.2f" % stat)
    assert stat < chi2.ppf(1 - 1e-6, 49)


@pytest.mark.parametrize("which", ["seed", "step", "row", "t", "attempt"])
def test_draw_sensitive_to_every_argument(which):
    """Changing one argument changes at least 90 % of 1,000 draws at item_size 12,103 (two independent ids collide about once in 1e4)."""
    base = {"seed": 11, "step": 5, "row": 0, "t": 0, "attempt": 2}
    other = dict(base, **{which: base[which] + 1})

    def grid(a):      # 40 rows x 25 positions, offset by the `row` / `t` entries
        return np.array([ops.seqbatch_draw(a["seed"], a["step"], a["row"] + 100 * r, a["t"] + 100 * t, a["attempt"], 12103)
                         for r in range(40) for t in range(25)])
    assert (grid(base) != grid(other)).mean() >= 0.9
