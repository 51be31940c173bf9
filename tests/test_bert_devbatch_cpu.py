"""CPU: adt_bertbatch_token, the host entry to the inline masking rule adt_bertbatch_build's kernel applies (include/adt_hip.h;
adt_amd/csrc/adt_bertbatch.cuh), and the command-line contract of --remask_every_epoch.  The rule is a pure function of (seed, salt,
example, position), so every check below is deterministic.  Needs only the built library.

The item handed to the rule is 0, which is no item id: a masked position then shows its kind by its token alone -- itemnum + 1 is
[MASK], 1..itemnum a replacement, 0 the kept item."""
import numpy as np
import pytest

from adt_amd import ops

ITEMS = 50
PAIRS = [(1234, 0), (23, 7), (987654321, 3)]       # (seed, salt)


def grid(seed, salt, examples, positions, mask_prob=0.2, itemnum=ITEMS):
    thr = ops.bertbatch_threshold(mask_prob)
    out = [ops.bertbatch_token(seed, salt, e, j, thr, itemnum, 0) for e in examples for j in positions]
    return np.array([t for t, _ in out]), np.array([m for _, m in out])


def test_threshold():
    assert ops.bertbatch_threshold(0.0) == 0 and ops.bertbatch_threshold(0.5) == 2 ** 31
    assert ops.bertbatch_threshold(0.2) == int(np.floor(0.2 * 2.0 ** 32)) and ops.bertbatch_threshold(1.0 - 2.0 ** -40) == 2 ** 32 - 1
    for bad in (-0.1, 1.0, 1.5):
        with pytest.raises(Exception):
            ops.bertbatch_threshold(bad)


def test_probability_zero_masks_nothing_and_an_unmasked_position_keeps_its_item():
    tok, masked = grid(5, 1, range(20), range(50), mask_prob=0.0)
    assert not masked.any() and (tok == 0).all()
    thr = ops.bertbatch_threshold(0.2)
    for e in range(30):
        t, m = ops.bertbatch_token(5, 1, e, 3, thr, ITEMS, 17)
        assert (t == 17 and not m) or (m and (t == ITEMS + 1 or 1 <= t <= ITEMS))


@pytest.mark.parametrize("seed,salt", PAIRS)
def test_law_of_the_rule(seed, salt):
    """20,000 positions (200 examples x 100 positions) at mask_prob 0.2: the masked count within 5 sigma of the binomial mean; the split
    [MASK] / replacement / kept below the 1 - 1e-6 chi-square quantile (2 degrees of freedom) against 0.8 / 0.1 / 0.1; the replacement
    ids below the 1 - 1e-6 quantile (49 degrees of freedom) against the uniform law over the 50 items."""
    from scipy.stats import chi2
    n, p = 20000, 0.2
    tok, masked = grid(seed, salt, range(200), range(100), p)
    assert tok.size == n
    k = int(masked.sum())
    sigma = np.sqrt(n * p * (1 - p))
    print("masked %d of %d (mean %.0f, sigma %.1f)" % (k, n, n * p, sigma))
    assert abs(k - n * p) < 5 * sigma
    assert (tok[~masked] == 0).all()
    t = tok[masked]
    kinds = np.array([(t == ITEMS + 1).sum(), ((t >= 1) & (t <= ITEMS)).sum(), (t == 0).sum()], np.float64)
    assert kinds.sum() == k
    expect = k * np.array([0.8, 0.1, 0.1])
    stat = float(((kinds - expect) ** 2 / expect).sum())
    print("kinds %s, chi2 = %.2f" % (kinds, stat))
    assert stat < chi2.ppf(1 - 1e-6, 2)
    ids = t[(t >= 1) & (t <= ITEMS)]
    counts = np.bincount(ids, minlength=ITEMS + 1)[1:]
    e_id = ids.size / float(ITEMS)
    stat = float(((counts - e_id) ** 2 / e_id).sum())
    print("%d replacement ids, chi2 = %.2f" % (ids.size, stat))
    assert stat < chi2.ppf(1 - 1e-6, ITEMS - 1)


@pytest.mark.parametrize("which", ["seed", "salt", "example", "position"])
def test_rule_sensitive_to_every_argument(which):
    """Changing one argument changes the decision pattern of a 1,000-position grid (40 examples x 25 positions).  Two independent patterns
    at mask_prob 0.2 disagree on the masked flag at 2 * 0.2 * 0.8 = 32 % of the positions (sigma 1.5 % over 1,000), so less than 20 %
    would mean the two are not independent."""
    base = {"seed": 11, "salt": 5, "example": 0, "position": 0}
    other = dict(base, **{which: base[which] + 1})

    def pattern(a):      # offset by the `example` / `position` entries; strides keep the shifted grid from overlapping the base one
        thr = ops.bertbatch_threshold(0.2)
        out = [ops.bertbatch_token(a["seed"], a["salt"], a["example"] + 100 * e, a["position"] + 100 * j, thr, ITEMS, 0)
               for e in range(40) for j in range(25)]
        return np.array([t for t, _ in out]), np.array([m for _, m in out])
    (t0, m0), (t1, m1) = pattern(base), pattern(other)
    assert not np.array_equal(m0, m1) and not np.array_equal(t0, t1)
    assert (m0 != m1).mean() >= 0.2


def test_remask_every_epoch_needs_device_batches():
    from adt_amd.bert4rec.main import parse_args
    with pytest.raises(SystemExit):
        parse_args(["--remask_every_epoch"])
    a = parse_args(["--device_batches", "--remask_every_epoch"])
    assert a.device_batches and a.remask_every_epoch
    a = parse_args([])
    assert not a.device_batches and not a.remask_every_epoch
