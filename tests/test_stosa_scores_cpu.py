"""CPU: the histogram identity behind STOSA-ADT's device-side scores (adt_amd/stosa/trainer.py:scores_from_hist)
against get_full_sort_score, and replay_hit_hist -- a numpy replay of adt_hit_hist's rule (first match, K when none, a -1 never matches,
group-major rows) that tests/test_stosa_scores_hip.py takes as its reference.

Tolerance 1e-12 absolute: both sides are float64 sums of at most N terms no larger than 1 divided by N, so they differ by no more than
N * 2^-53 <= 300 * 1.2e-16 = 3.4e-14."""
import numpy as np
import pytest

from adt_amd._lib import AdtError
from adt_amd.stosa.trainer import get_full_sort_score, scores_from_hist

TOL = 1e-12


def replay_hit_hist(top_idx, answers, rows_per_group=None):
    """(hist (groups, K + 1) int64, hit_pos (N,) int32) of list rows top_idx (N, K): row r belongs to group r // rows_per_group and its
    answer is answers[r % rows_per_group]; position = the first j with top_idx[r][j] == answer, K when there is none; -1 never matches."""
    top_idx = np.asarray(top_idx)
    ans = np.asarray(answers).reshape(-1)
    N, K = top_idx.shape
    rpg = len(ans) if rows_per_group is None else rows_per_group
    assert len(ans) == rpg and rpg >= 1 and N % rpg == 0
    groups = N // rpg
    hist = np.zeros((groups, K + 1), np.int64)
    pos = np.full(N, K, np.int32)
    for r in range(N):
        a = ans[r % rpg]
        for j in range(K):
            if top_idx[r, j] >= 0 and top_idx[r, j] == a:
                pos[r] = j
                break
        hist[r // rpg, pos[r]] += 1
    return hist, pos


def placed_lists(r, N, K=40, n_items=200):
    """N id lists of K distinct ids out of 0..n_items-1 and one answer per user: user u's answer stands at position u % (K + 2) for
    positions 0..K-1, is absent for K, and for K + 1 the answer is 0 with id 0 listed (at position u % K)."""
    pred = np.stack([r.permutation(n_items)[:K] for _ in range(N)]).astype(np.int64)
    ans = np.zeros((N, 1), np.int64)
    want = np.zeros(N, np.int64)
    for u in range(N):
        kind = u % (K + 2)
        if kind < K:
            ans[u, 0], want[u] = pred[u, kind], kind
        elif kind == K:
            ans[u, 0], want[u] = n_items + 5, K
        else:
            j = u % K
            pred[u][pred[u] == 0] = n_items + 1        # at most one 0 in the list: where the test puts it
            pred[u, j] = 0
            ans[u, 0], want[u] = 0, j
    return pred, ans, want


@pytest.mark.parametrize("N", (1, 7, 300))
def test_scores_from_hist_matches_get_full_sort_score(N):
    r = np.random.RandomState(N)
    pred, ans, want = placed_lists(r, N)
    hist, pos = replay_hit_hist(pred, ans)
    assert np.array_equal(pos, want) and hist.shape == (1, 41) and hist.sum() == N
    got, ref = scores_from_hist(hist[0]), get_full_sort_score(ans, pred)
    err = np.abs(np.array(got) - np.array(ref)).max()
    print("N", N, "max |scores_from_hist - get_full_sort_score|", err)
    assert len(got) == 13 and err <= TOL


def test_random_answers_with_misses():
    r = np.random.RandomState(11)
    N, K = 300, 40
    pred = np.stack([r.permutation(400)[:K] for _ in range(N)]).astype(np.int64)
    ans = r.randint(0, 400, size=(N, 1)).astype(np.int64)
    hist, _ = replay_hit_hist(pred, ans)
    assert 0 < hist[0, K] < N                                   # hits and misses both
    err = np.abs(np.array(scores_from_hist(hist[0])) - np.array(get_full_sort_score(ans, pred))).max()
    assert err <= TOL


def test_longer_lists_score_their_first_40_positions():
    """K = 64: positions 40..63 count as users (N) but reach no HIT@k / NDCG@k; MRR runs over all K."""
    r = np.random.RandomState(12)
    N, K = 50, 64
    pred = np.stack([r.permutation(100)[:K] for _ in range(N)]).astype(np.int64)
    ans = r.randint(0, 100, size=(N, 1)).astype(np.int64)
    hist, _ = replay_hit_hist(pred, ans)
    got, ref = scores_from_hist(hist[0]), get_full_sort_score(ans, pred)
    assert np.abs(np.array(got) - np.array(ref)).max() <= TOL


def test_replay_rule():
    top = np.array([[5, 7, 5, -1], [-1, -1, -1, -1], [0, 3, 2, 1], [9, 8, 7, 6], [4, 4, 4, 4], [1, 2, 3, 0]], np.int32)
    hist, pos = replay_hit_hist(top, np.array([5, -1, 0]), rows_per_group=3)      # rows 0-2: group 0, rows 3-5: group 1
    assert pos.tolist() == [0, 4, 0, 4, 4, 3]                   # the first of two 5s; -1 matches nothing, not even the answer -1
    assert hist.tolist() == [[2, 0, 0, 0, 1], [0, 0, 0, 1, 2]]


def test_small_k_and_bad_rows_raise():
    with pytest.raises(AdtError):
        scores_from_hist(np.ones(40, np.int64))                 # K = 39
    with pytest.raises(AdtError):
        scores_from_hist(np.zeros(41, np.int64))                # no users
    with pytest.raises(AdtError):
        scores_from_hist(np.ones((2, 41), np.int64))
    with pytest.raises(AdtError):
        scores_from_hist(np.ones(41, np.float64))
    assert len(scores_from_hist(np.ones(41, np.int64))) == 13
