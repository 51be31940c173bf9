"""Full-catalogue ranking and top-K recommendation for the dot-product backbones (SASRecADT, SASRecADTWide, BertModel): one
adt_full_rank call on the final feature rows and the item table (include/adt_hip.h; adt_amd/csrc/adt_fullrank.cuh).  No (B, V) logit
matrix exists at any point; only B ranks, B counts and the (B, k) best items come back.

STOSA-ADT (DistRankMixin) ranks by ascending Wasserstein distance through the same kernel: adt_wdist_pack turns the two item tables and
the users' last states into 2d-wide row images with dist[b][j] = na[b] - 2 (A[b] . W[j] + bias[j]) ("STOSA").
A distance_metric='kl' model ranks on request (rowwise=True) by the row-wise KL divergence it is trained on, the same way:
adt_klrow_pack's images give KL[b][j] = nu[b] - (A[b] . W[j] + bias[j])."""
import numpy as np
import torch

from . import _lib, ops


def _targets(targets, B, device):
    if targets is None:
        return None
    tgt = targets.to(device=device, dtype=torch.int32).contiguous() if isinstance(targets, torch.Tensor) else \
        torch.from_numpy(np.ascontiguousarray(np.asarray(targets), dtype=np.int32)).to(device)
    assert tgt.numel() == B, (tgt.shape, B)
    return tgt


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
        indptr, indices = ops.seen_csr(seen, B, E.device)
        return ops.full_rank(F, F.stride(0), E, n_items, _targets(targets, B, E.device), bias, indptr, indices, topk)

    @torch.no_grad()
    def rank_full_rows(self, log_seqs, targets, seen_off, seen_items, row0=0, topk=0):
        """rank_full for rows row0 .. row0 + B - 1 of an evaluation set that lives on the device (DeviceEvalData.full_batch): `targets`
        (int32) and the CSR seen_off (int64) / seen_items (int32) are the RESIDENT tensors of the whole set and are read in place by
        adt_full_rank_groups (one group); nothing is built on the host or uploaded.  Returns what rank_full returns."""
        F, E, n_items, bias = self._full_rank_operands(log_seqs)
        B = F.shape[0]
        return ops.full_rank_groups(F, F.stride(0), E, n_items, targets, seen_off, seen_items, B, B, row0=row0, bias=bias, k=topk)

    def recommend(self, log_seqs, k, seen=None):
        """The k best unseen items of every user: (ids (B, k) int32, scores (B, k)), best first, ties to the smaller id; -1 / -inf where
        fewer than k items are left."""
        _, _, idx, val = self.rank_full(log_seqs, None, seen, k)
        return idx, val


# ---- STOSA-ADT: Wasserstein distance ---------------------------------------------------------------------------------------------------
def _seen(seen, B, device):
    """ops.seen_csr, or an (indptr, indices) pair that is on the device already."""
    if isinstance(seen, tuple) and all(x is None or isinstance(x, torch.Tensor) for x in seen):
        return seen
    return ops.seen_csr(seen, B, device)


def dist_from_scores(na, top_idx, top_val):
    """Scores of adt_full_rank on packed images back to distances: top_dist = na[:, None] - 2 * top_val (ascending, as top_val
    descends); +inf where top_idx is -1 (fewer than k eligible items)."""
    dist = na[:, None] - 2.0 * top_val
    return torch.where(top_idx < 0, torch.full_like(dist, float("inf")), dist)


def fused_ids_or_two_pass(top_idx, two_pass):
    """The fused top-k ids of one evaluation batch as an int64 array -- unless some row came back with a -1 (fewer than k unseen
    items: the reference's sort then continues into the seen items, pushed to 1e24): then the whole batch is two_pass(), the form that
    reproduces it.  Returns (ids, fell_back)."""
    ids = top_idx.cpu().numpy().astype(np.int64)
    if (ids < 0).any():
        return two_pass(), True
    return ids, False


def kl_dist_from_scores(nu, top_idx, top_val):
    """Scores of adt_full_rank on adt_klrow_pack's images back to row-wise KL divergences: top_dist = nu[:, None] - top_val (ascending, as
    top_val descends); +inf where top_idx is -1."""
    dist = nu[:, None] - top_val
    return torch.where(top_idx < 0, torch.full_like(dist, float("inf")), dist)


class DistRankMixin:
    """A model supplies _dist_tables() -> (Em, Ec, n_items): the item mean / raw covariance tables (n_items + 1 rows are ranked) and
    _last_state(input_ids) -> (sm, sc): the (B, d) mean / covariance of the last position.  Wasserstein distance by default; a model with
    distance_metric 'kl' ranks only on request (rowwise=True), by the row-wise KL divergence it is trained on."""

    def _check_wasserstein(self):
        if getattr(self, "distance_metric", "wasserstein") != "wasserstein":
            raise _lib.AdtError("fused full-catalogue ranking is built for distance_metric='wasserstein' only: the %r scores depend on the eval "
                                "batch's size and row order, not on (user, item) alone; use predict_full + topk_masked" % (self.distance_metric,))

    def _rowwise_kl(self, rowwise):
        """True when this call ranks by the row-wise KL divergence: a KL model that was asked to.  A KL model that was not asked raises as
        it always has; a Wasserstein model is row-wise already, so `rowwise` changes nothing for it."""
        if getattr(self, "distance_metric", "wasserstein") == "kl" and rowwise:
            return True
        self._check_wasserstein()
        return False

    @torch.no_grad()
    def item_image(self):
        """(W (n_items + 1, 2d), bias (n_items + 1,)) of the two item tables.  Packed on every call -- no cache: it is stale after any
        weight update -- so a caller that ranks many batches under the same weights holds on to it and passes it as `image`."""
        self._check_wasserstein()
        Em, Ec, _ = self._dist_tables()
        return self._wdist_pack(Em, Ec, True, -0.5)

    def _wdist_pack(self, M, C, elu, nrm_scale):
        """ops.wdist_pack, lane-aware for a model at a padded width (model.lanes): ELU(0) + 1 = 1 on a pad lane of
        the item covariances must not reach the image; with zero pad columns on both sides the ranking kernel needs no change."""
        lanes = getattr(self, "lanes", None)
        return ops.wdist_pack(M, C, elu, nrm_scale) if lanes is None else ops.wdist_pack_lanes(M, C, elu, nrm_scale, lanes)

    @torch.no_grad()
    def kl_row_image(self):
        """item_image() of a KL model for rowwise=True: (W, bias) with KL[u][v] = nu[u] - (A[u] . W[v] + bias[v]) (ops.klrow_pack).  Packed
        on every call, no cache, as item_image().  A Wasserstein model raises."""
        if getattr(self, "distance_metric", "wasserstein") != "kl":
            raise _lib.AdtError("kl_row_image is the item image of distance_metric='kl'; a %r model ranks on item_image()"
                                % (getattr(self, "distance_metric", "wasserstein"),))
        Em, Ec, _ = self._dist_tables()
        return self._klrow_pack(Em, Ec, True)

    def _klrow_pack(self, M, C, items):
        """ops.klrow_pack, lane-aware for a model at a padded width as _wdist_pack: a pad lane holds ELU(0) + 1 = 1
        on the item side and a covariance 0 on the user side, and neither may reach an image or an offset."""
        lanes = getattr(self, "lanes", None)
        return ops.klrow_pack(M, C, items) if lanes is None else ops.klrow_pack_lanes(M, C, items, lanes)

    @torch.no_grad()
    def _rank_states(self, sm, sc, targets, seen, topk, image, first_id, rowwise=False):
        kl = self._rowwise_kl(rowwise)
        if image is None:
            image = self.kl_row_image() if kl else self.item_image()
        W, bias = image
        n_items = self._dist_tables()[2]
        A, na = self._klrow_pack(sm, sc, False) if kl else self._wdist_pack(sm, sc, False, 1.0)
        B = A.shape[0]
        indptr, indices = _seen(seen, B, A.device)
        rank, n_elig, top_idx, top_val = ops.full_rank(A, A.stride(0), W, n_items, _targets(targets, B, A.device), bias, indptr, indices, topk,
                                                       first_id=first_id)
        if top_idx is None:
            return rank, n_elig, None, None
        return rank, n_elig, top_idx, (kl_dist_from_scores if kl else dist_from_scores)(na, top_idx, top_val)

    @torch.no_grad()
    def rank_full(self, input_ids, targets, seen=None, topk=0, image=None, first_id=1, rowwise=False):
        """As FullRankMixin.rank_full with `smaller distance` for `higher score`: (rank (B,) -- eligible items strictly closer than the
        target, -1 without one --, n_elig (B,), top_idx (B, topk), top_dist (B, topk) ascending, ties to the smaller id, -1 / +inf
        tail).  image: item_image() of the current weights; first_id = 0 lets the padding item 0 compete, as the reference's full sort
        does (targets stay 1..n_items).

        rowwise=True on a distance_metric='kl' model (which raises without it): the distance is the row-wise KL divergence of the user's
        last state from the item, kl_distance -- the function the model is trained on -- NOT the reference's batch-dependent
        kl_predict_full score; image is then kl_row_image().  On a Wasserstein model rowwise changes nothing."""
        self._rowwise_kl(rowwise)
        sm, sc = self._last_state(input_ids)
        return self._rank_states(sm, sc, targets, seen, topk, image, first_id, rowwise)

    def recommend(self, input_ids, k, seen=None, image=None, rowwise=False):
        """The k closest unseen items of every user: (ids (B, k) int32, distances (B, k)), closest first; -1 / +inf where fewer than k
        items are left.  The padding item 0 is never recommended.  rowwise: as rank_full."""
        _, _, idx, dist = self.rank_full(input_ids, None, seen, k, image, 1, rowwise)
        return idx, dist
