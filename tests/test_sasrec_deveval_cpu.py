"""CPU side of the device-resident sampled evaluation of SASRec-ADT: the candidate stream against its table, the
condition under which the GPU replay test exercises the sampling path and not the guard, metrics_from_hist, the launchers' argument
errors (no launch) and DeviceEvalData's user lists.  No GPU."""
import ctypes

import numpy as np
import pytest

from adt_amd import _lib, ops
from adt_amd.sasrec import utils as U
from adt_amd.sasrec.device_eval import DeviceEvalData

import sasrec_deveval_cases as cases


def test_stream_follows_the_table():
    """16 ids, two of count zero (id 0 and an interior one), n = 200,000 stream values: no zero-count id appears, and every other id's
    frequency lies within 6 sqrt(n p (1 - p)) + 1 + n * total / 2^32 of n p -- six binomial standard deviations, one for rounding the
    bound itself, and the multiply-high bias (at most total / 2^32 per draw)."""
    count = np.array([0, 5, 1, 9, 30, 2, 7, 0, 12, 3, 100, 1, 4, 8, 20, 6], np.int64)
    cum = np.concatenate([[0], np.cumsum(count)])
    n, total = 200000, int(cum[-1])
    xs = ops.evalcand_stream(cum, 23, 1, 7, 0, n)
    got = np.bincount(xs, minlength=16)
    assert xs.min() >= 0 and xs.max() < 16 and got[count == 0].sum() == 0
    for i in np.nonzero(count)[0]:
        p = count[i] / total
        bound = 6 * np.sqrt(n * p * (1 - p)) + 1 + n * total / 2.0 ** 32
        print(i, got[i], n * p, bound)
        assert abs(got[i] - n * p) <= bound, (i, got[i], n * p, bound)
    # the entry point is positional: a window of the stream is that window
    assert np.array_equal(ops.evalcand_stream(cum, 23, 1, 7, 1000, 50), xs[1000:1050])
    assert not np.array_equal(ops.evalcand_stream(cum, 23, 2, 7, 0, 50), xs[:50])
    assert not np.array_equal(ops.evalcand_stream(cum, 23, 1, 8, 0, 50), xs[:50])


@pytest.mark.parametrize("S,max_hist", cases.SAMPLER_CASES)
@pytest.mark.parametrize("mode", ["val", "test"])
def test_replay_stays_clear_of_the_guard(S, max_hist, mode):
    """Every user of the GPU replay test finds its S candidates within ADT_EVALCAND_MAX_DRAWS stream values, so that test compares the
    sampling path; the user built for the guard does not."""
    train, valid, test, usernum, itemnum = cases.make_data(max_hist)
    data = DeviceEvalData(train, valid, test, usernum, itemnum, 8, S, mode, device="cpu")
    assert ops.EVALCAND_MAX_DRAWS == cases.MAX_DRAWS
    seen = cases.seen_rows(train, valid, test, data.users, mode)
    worst = 0
    for row, s in enumerate(seen):
        ids, filled, used = cases.replay_row(data.cum_host, s, S, 23, 0, row)
        assert used is not None and used < cases.MAX_DRAWS and filled == S and len(set(ids)) == S, (row, used)
        assert 0 not in ids and itemnum not in ids and cases.ZERO_ID not in ids and not set(ids) & set(s.tolist())
        worst = max(worst, used)
    print("most stream values used:", worst)
    cum, gseen, free = cases.guard_table(S + 1)
    ids, filled, used = cases.replay_row(cum, gseen, S, 23, 0, 3)
    assert used is None and filled == S and len(set(ids)) == S and set(ids) <= set(free)


def test_metrics_from_hist_agrees_with_metrics_from_ranks():
    """N = 6,040 random ranks over C = 101 candidates: HR equal exactly, NDCG and AUC within N * 2^-52 relative (the bound for reordering a
    float64 sum of N terms)."""
    N, C = 6040, 101
    ranks = np.random.RandomState(3).randint(0, C, size=N)
    (nd_r, hr_r), auc_r = U.metrics_from_ranks(ranks, C, (5, 10))
    (nd_h, hr_h), auc_h = U.metrics_from_hist(np.bincount(ranks, minlength=C), C, (5, 10))
    tol = N * 2.0 ** -52
    for k in (5, 10):
        assert hr_h[k] == hr_r[k]
        assert abs(nd_h[k] - nd_r[k]) <= tol * abs(nd_r[k]), (k, nd_h[k], nd_r[k])
    assert abs(auc_h - auc_r) <= tol * abs(auc_r), (auc_h, auc_r)
    assert isinstance(auc_h, float) and isinstance(nd_h[10], float)


def test_launchers_reject_bad_arguments_without_a_launch():
    lib = _lib.load()
    fake = ctypes.c_void_p(4096)      # never dereferenced: each call fails on its scalars (or on the NULL) first

    def draw(cum=fake, n_ids=16, total=100, seen_off=fake, seen_items=fake, targets=fake, S=5, ldc=None, cand=fake):
        return lib.adt_evalcand_draw(cum, n_ids, total, seen_off, seen_items, targets, 4, 0, 4, S, 1, 2, cand, 1 + S if ldc is None else ldc, None, None)

    def rank(C=101, d=64, ldf=64, F=fake, E=fake, cand=fake, hist=fake, rpg=4):
        return lib.adt_cand_rank_hist(F, ldf, E, None, cand, 8, rpg, C, d, hist, None, None)
    for call, word in ((lambda: draw(total=2 ** 32), "total"), (lambda: draw(total=2 ** 40), "total"), (lambda: draw(total=0), "total"),
                       (lambda: draw(S=0), "S=0"), (lambda: draw(S=ops.EVALCAND_MAX_S + 1), "S="), (lambda: draw(cum=None), "NULL"),
                       (lambda: draw(seen_off=None), "NULL"), (lambda: draw(seen_items=None), "NULL"), (lambda: draw(targets=None), "NULL"),
                       (lambda: draw(cand=None), "NULL"), (lambda: draw(ldc=5), "ldc"), (lambda: rank(C=0), "C=0"), (lambda: rank(C=-1), "C=-1"),
                       (lambda: rank(d=50, ldf=52), "d=50"), (lambda: rank(d=0), "d=0"), (lambda: rank(ldf=60), "ldf"),
                       (lambda: rank(rpg=3), "multiple"), (lambda: rank(F=None), "NULL"), (lambda: rank(hist=None), "NULL")):
        assert call() != 0
        assert word in lib.adt_last_error().decode(), (word, lib.adt_last_error().decode())
    # the host stream reads its table, so it sees the total itself
    big = np.array([0, 2 ** 31, 2 ** 32], np.int64)
    with pytest.raises(_lib.AdtError, match="total"):
        ops.evalcand_stream(big, 1, 2, 0, 0, 4)
    assert lib.adt_evalcand_stream(None, 16, 1, 2, 0, 0, 4, fake) != 0
    ok = np.array([0, 2 ** 31, 2 ** 32 - 1], np.int64)
    assert set(ops.evalcand_stream(ok, 1, 2, 0, 0, 64).tolist()) <= {0, 1}


@pytest.mark.parametrize("mode", ["val", "test"])
def test_user_lists_and_targets_equal_evaldataset(mode):
    train, valid, test, usernum, itemnum = cases.make_data(60)
    sampler = U.PopularSampler(train, valid, test, usernum, itemnum, 5)
    ds = U.EvalDataset(train, valid, test, usernum, itemnum, 8, sampler, mode, -1, frozen=False)
    data = DeviceEvalData(train, valid, test, usernum, itemnum, 8, 5, mode, -1, device="cpu")
    assert data.users == ds.users and len(data.users) == usernum - 2      # users 1 and 2 have no held-out item
    assert 1 not in data.users and 2 not in data.users
    assert data.targets_host.tolist() == [U.eval_target(ds, u) for u in ds.users]
    assert data.cand[:, 0].tolist() == data.targets_host.tolist()
    # PopularSampler's table: the same counts, as exact prefix sums
    want = np.array([sum(h[u].count(i) for h in (train, valid, test) for u in h) for i in range(itemnum)], np.int64)
    assert np.array_equal(np.diff(data.cum_host), want) and data.cum_host[0] == 0 and want[0] == 0 and want[cases.ZERO_ID] == 0
    assert np.allclose(want / want.sum(), sampler.popular_p, rtol=0, atol=1e-15)
    # a drawn subset follows EvalDataset's rule and order as well
    np.random.seed(11)
    ds2 = U.EvalDataset(train, valid, test, usernum, itemnum, 8, sampler, mode, 12, frozen=False)
    np.random.seed(11)
    d2 = DeviceEvalData(train, valid, test, usernum, itemnum, 8, 5, mode, 12, device="cpu")
    assert d2.users == ds2.users and 0 < len(d2.users) <= 12
    # and from_dataset takes the dataset's own list
    assert DeviceEvalData.from_dataset(ds2, device="cpu", upload=False).users == ds2.users


def test_too_few_drawable_items_is_an_error():
    """The reference would spin forever on such a user; the kernel would fill id 0: DeviceEvalData refuses it at construction."""
    train, valid, test, usernum, itemnum = cases.make_data(60)
    with pytest.raises(_lib.AdtError, match="drawable"):
        DeviceEvalData(train, valid, test, usernum, itemnum, 8, 100, "val", device="cpu")
    with pytest.raises(_lib.AdtError, match="sample_size"):
        DeviceEvalData(train, valid, test, usernum, itemnum, 8, 0, "val", device="cpu")
