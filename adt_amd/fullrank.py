"""Full-catalogue ranking and top-K recommendation for the dot-product backbones (SASRecADT, SASRecADTWide, BertModel): one
adt_full_rank call on the final feature rows and the item table (include/adt_hip.h; adt_amd/csrc/adt_fullrank.cuh).  No (B, V) logit
matrix exists at any point; only B ranks, B counts and the (B, k) best items come back."""
import numpy as np
import torch

from . import ops


class FullRankMixin:
    """A model supplies _full_rank_operands(log_seqs) -> (F, E, n_items, bias): F the (B, d) final feature rows (any row stride), E the
    item table with at least n_items + 1 rows of width d, bias a per-item bias or None."""

    @torch.no_grad()
    def rank_full(self, log_seqs, targets, seen=None, topk=0):
        """Rank of targets[b] among ALL items 1..n_items the user has not seen (`seen`: a scipy CSR matrix, a dense 0/1 array, an
        (indptr, indices) pair or None, one row per user; the target stays eligible even when listed).  Returns device tensors
        (rank (B,) -- the number of eligible items scoring strictly higher, -1 without a target --, n_elig (B,) eligible items other
        than the target, top_idx (B, topk), top_val (B, topk)); the last two are None when topk = 0."""
        F, E, n_items, bias = self._full_rank_operands(log_seqs)
        B = F.shape[0]
        tgt = None
        if targets is not None:
            tgt = targets.to(device=E.device, dtype=torch.int32).contiguous() if isinstance(targets, torch.Tensor) else \
                torch.from_numpy(np.ascontiguousarray(np.asarray(targets), dtype=np.int32)).to(E.device)
            assert tgt.numel() == B, (tgt.shape, B)
        indptr, indices = ops.seen_csr(seen, B, E.device)
        return ops.full_rank(F, F.stride(0), E, n_items, tgt, bias, indptr, indices, topk)

    def recommend(self, log_seqs, k, seen=None):
        """The k best unseen items of every user: (ids (B, k) int32, scores (B, k)), best first, ties to the smaller id; -1 / -inf where
        fewer than k items are left."""
        _, _, idx, val = self.rank_full(log_seqs, None, seen, k)
        return idx, val
