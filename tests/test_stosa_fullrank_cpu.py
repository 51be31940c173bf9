"""CPU: the host-only parts of the fused STOSA-ADT evaluation (adt_amd/fullrank.py): scores of adt_full_rank on packed images back to
Wasserstein distances, and the decision of full_sort(fused=True) / evaluate_candidates(fused=True) to recompute a batch two-pass."""
import numpy as np
import torch

from adt_amd.fullrank import dist_from_scores, fused_ids_or_two_pass


def test_dist_from_scores_and_inf_tail():
    inf = float("inf")
    na = torch.tensor([10.0, 3.0, 7.5])
    top_idx = torch.tensor([[4, 2, 9], [5, -1, -1], [-1, -1, -1]], dtype=torch.int32)
    top_val = torch.tensor([[4.0, 1.5, -2.0], [0.25, -inf, -inf], [-inf, -inf, -inf]])
    d = dist_from_scores(na, top_idx, top_val)
    assert d.dtype == torch.float32 and d.shape == (3, 3)
    assert torch.equal(d, torch.tensor([[2.0, 7.0, 14.0], [2.5, inf, inf], [inf, inf, inf]]))      # ascending as the scores descend
    # the tail follows the ids, not the scores: a -1 slot is +inf whatever its score field holds, no NaN from inf arithmetic
    d2 = dist_from_scores(torch.tensor([inf]), torch.tensor([[1, -1]], dtype=torch.int32), torch.tensor([[1.0, 5.0]]))
    assert torch.equal(d2, torch.tensor([[inf, inf]])) and not torch.isnan(d2).any()


def test_fallback_decision_on_stubbed_outputs():
    calls = []

    def two_pass():
        calls.append(1)
        return np.full((2, 3), 7, np.int64)
    full = torch.tensor([[0, 5, 2], [3, 1, 4]], dtype=torch.int32)         # item 0 is a legitimate entry, not a short row
    ids, fell_back = fused_ids_or_two_pass(full, two_pass)
    assert not fell_back and not calls and ids.dtype == np.int64 and np.array_equal(ids, [[0, 5, 2], [3, 1, 4]])
    short = torch.tensor([[0, 5, 2], [3, 1, -1]], dtype=torch.int32)       # one user with fewer than k unseen items
    ids, fell_back = fused_ids_or_two_pass(short, two_pass)
    assert fell_back and len(calls) == 1 and np.array_equal(ids, np.full((2, 3), 7))      # the whole batch is the two-pass result
