"""CPU: the host side of full-catalogue evaluation (adt_amd/sasrec/utils.py: full_rank_stats, eval_seen_csr, evaluate_full's inputs;
adt_amd/ops.py: seen_csr_host).  No GPU, no HIP call."""
import numpy as np
import scipy.sparse as sp

from adt_amd import ops
from adt_amd.sasrec import utils as U


def test_full_rank_stats_are_additive_and_match_a_direct_computation():
    r = np.random.RandomState(0)
    ranks = r.randint(0, 40, 200)
    ranks[:7] = 0
    n_elig = ranks + r.randint(1, 3000, 200)
    ks = (5, 10)
    whole = U.full_rank_stats(ranks, n_elig, ks)
    halves = U.full_rank_stats(ranks[:77], n_elig[:77], ks) + U.full_rank_stats(ranks[77:], n_elig[77:], ks)
    assert whole.dtype == np.float64 and whole.shape == U.rank_stats(ranks, 100, ks).shape
    np.testing.assert_allclose(halves, whole, rtol=1e-13)
    (ndcg, hr), auc = U.metrics_from_stats(whole, ks)
    for k in ks:
        assert hr[k] == np.mean(ranks < k)
        np.testing.assert_allclose(ndcg[k], np.mean(np.where(ranks < k, 1.0 / np.log2(ranks + 2.0), 0.0)), rtol=1e-13)
    np.testing.assert_allclose(auc, np.mean((n_elig - ranks) / n_elig), rtol=1e-13)
    # a target that beats everything scores 1, one that loses to everything 0
    assert U.metrics_from_stats(U.full_rank_stats([0, 50], [50, 50], ks), ks)[1] == 0.5


def _five_users():
    train = {1: [3, 4, 5], 2: [9], 3: [1, 2], 4: [7, 7, 8], 5: []}
    val = {1: [6], 2: [2], 3: [], 4: [1], 5: [4]}
    test = {1: [7], 2: [3], 3: [], 4: [2], 5: [5]}
    return train, val, test


def test_seen_sets_for_val_and_test():
    train, val, test = _five_users()
    for mode in ("val", "test"):
        ds = U.EvalDataset(train, val, test, 5, 9, 4, None, mode)
        assert ds.users == [1, 2, 4]           # user 3 has nothing held out, user 5 no training items
        indptr, indices = U.eval_seen_csr(ds, ds.users)
        assert indptr.dtype == np.int32 and indices.dtype == np.int32
        got = [indices[indptr[i]:indptr[i + 1]].tolist() for i in range(3)]
        if mode == "val":
            assert got == [[3, 4, 5], [9], [7, 7, 8]]
            assert [U.eval_target(ds, u) for u in ds.users] == [6, 2, 1]
            assert ds.sequence(1).tolist() == [0, 3, 4, 5]
        else:                                    # the validation item has been seen by test time, and is fed
            assert got == [[3, 4, 5, 6], [9, 2], [7, 7, 8, 1]]
            assert [U.eval_target(ds, u) for u in ds.users] == [7, 3, 2]
            assert ds.sequence(1).tolist() == [3, 4, 5, 6]
        assert ds.sequence(2).dtype == np.int32
        # the sequence is the one sample_data builds
        ds.negative_sampler = type("S", (), {"get_negative_samples": lambda self, user, mode, rng: [1, 2]})()
        assert np.array_equal(ds.sample_data(4)[1], ds.sequence(4))


def test_seen_csr_same_for_scipy_dense_and_pair():
    r = np.random.RandomState(3)
    dense = (r.rand(9, 50) < 0.2).astype(np.int8)
    dense[4] = 0
    a = ops.seen_csr_host(sp.csr_matrix(dense), 9)
    b = ops.seen_csr_host(dense, 9)
    c = ops.seen_csr_host(a, 9)
    for x in (a, b, c):
        assert x[0].dtype == np.int32 and x[1].dtype == np.int32 and x[0].flags.c_contiguous and x[1].flags.c_contiguous
        assert np.array_equal(x[0], a[0]) and np.array_equal(x[1], a[1])
    assert a[0][-1] == dense.sum() and a[0][5] == a[0][4]
    rows, cols = np.nonzero(dense)
    assert np.array_equal(a[1], cols)
    assert ops.seen_csr_host(None, 9) == (None, None)
    assert ops.seen_csr_host(np.zeros((9, 50)), 9) == (None, None)
    assert ops.seen_csr_host(sp.csr_matrix((9, 50)), 9) == (None, None)
