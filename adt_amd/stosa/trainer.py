"""Fused training step and full-sort evaluation for STOSA-ADT: the train branch of the reference's
DistSAModelTrainer.iteration (stosa/trainer.py:525-560: finetune, bpr_optimization, reconstruction + independence terms,
backward, Adam -- no gradient clipping) as one device-side launch sequence, optionally replayed from a HIP graph, and the
full-sort branch (:583-612: distance of the last state to every item, seen items masked, 40 smallest).

Data-parallel (one process per GPU, RCCL over xGMI): batch rows shard across ranks with GLOBAL normalisers (sum of
istarget, B*L*d, B*L*H of the whole batch) and GLOBAL dropout indices; one sum all-reduce of the flat gradient buffer;
Adam runs identically on every rank on the reduced buffer over the trained prefix only (the parameters the reference
leaves at grad=None are outside it).
"""
import numpy as np
import torch

from .. import _lib, ops
from ..fullrank import _seen, fused_ids_or_two_pass
from ..wide import TapeTrainer, loss_norms


class FusedStosaTrainer(TapeTrainer):
    def __init__(self, model, lambda1, lambda2, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, process_group=None, use_graph=False,
                 seed=42):
        self.lambda1, self.lambda2 = [float(x) for x in lambda1], [float(x) for x in lambda2]
        nl = model.num_layers
        assert len(self.lambda1) == nl and len(self.lambda2) == nl
        w = [1.0, 1.0, 0.0]             # loss slots {bpr, pvn (weighted), auc, mse.., nll..}
        for l in range(nl):
            w += [self.lambda1[l], self.lambda1[l]]
        for l in range(nl):
            w += [self.lambda2[l], self.lambda2[l]]
        # no clip_grad_norm_ in the reference (trainer.py:557-559): clip = inf
        super().__init__(model, w, "item_decoder.layer.0.enc_attention.mean_query.weight", lr, betas, eps, weight_decay, 1e30, process_group,
                         use_graph, n=model.n_trained_floats)
        model.seed_trainer(seed)
        self._device_norms = {}          # step_device: (rows, global rows) -> device normalisers

    def stage(self, input_ids, dec_ids, pos_ids, neg_ids, n_target_global=None, norms_scale=1):
        m = self.model
        st = m.stage(input_ids, dec_ids, pos_ids, neg_ids, n_target_global)
        st["norms"] = loss_norms(m, st["B"] * m.maxlen, scale=norms_scale)
        return st

    def _body(self, st, b_offset):
        m = self.model
        m.push()        # padded widths: the reference-shaped parameters are the truth between steps (no-op otherwise)
        m.loss_forward_backward(st, self.lambda1, self.lambda2, st["norms"], self.loss_slots, b_offset)
        self._buckets.finish()
        # pad weights and pad gradients are exact zeros, so Adam (and its coupled weight decay) keeps them zero
        ops.clip_adam_l2(m.flat, m.flat_grad, self.m, self.v, self.wd, self.clip, self.lr, self.betas[0], self.betas[1], self.eps, self.scal,
                         n=m.n_trained_floats)
        m.pull()

    def step(self, input_ids, dec_ids, pos_ids, neg_ids, n_target_global=None, b_offset=0, norms_scale=1):
        self.step_staged(self.stage(input_ids, dec_ids, pos_ids, neg_ids, n_target_global, norms_scale), b_offset)

    def step_device(self, st, b_offset=0):
        """One step on a batch that is on the device already (DeviceDisenData.train_stage): adds the normalisers -- kept per
        (rows, global rows), so a step uploads nothing -- and runs step_staged.  Under data parallelism st holds this rank's rows of a
        batch of st["B_global"] sequences and b_offset is the first of them."""
        key = (st["B"], st.get("B_global", st["B"]))
        if key not in self._device_norms:
            self._device_norms[key] = loss_norms(self.model, key[0] * self.model.maxlen, scale=key[1] / float(key[0]))
        self.step_staged(dict(st, norms=self._device_norms[key]), b_offset)

    # ------------------------------------------------------------------------------------------------------------------
    def _rowwise_kl(self, rowwise):
        """rowwise=True on a KL model: rank by the row-wise KL divergence (DistRankMixin.rank_full).  On a Wasserstein
        model the keyword changes nothing: that distance is row-wise already."""
        return bool(rowwise) and self.model.distance_metric == "kl"

    @torch.no_grad()
    def full_sort(self, batches, topk=40, fused=False, rowwise=False):
        """Full-sort evaluation (stosa/trainer.py:583-612) over an iterable of (input_ids (B, L), seen, answers (B, A)): rank all
        items by ascending distance with the seen items pushed to 1e24 and keep `topk`, all on the device (model.predict_full: adt_wdist_full,
        or adt_kldist_full for distance_metric 'kl', whose scores depend on each batch's rows being the eval batch -- pass the reference's
        eval batches -- then adt_topk_masked); only the (B, topk) ids come back.  `seen` is the users' rows of the train/valid rating matrix as a scipy
        CSR matrix, a dense (B, item_size) 0/1 array, an int32 (indptr, indices) pair, or None (ops.seen_csr).  input_ids may be a device int32
        tensor and `seen` a pair of device int32 tensors (DeviceDisenData.eval_batch): both are used where they are, nothing is copied from the
        host.  Returns (pred_list (N, topk), answers (N, A)) for get_full_sort_score.

        fused=True (Wasserstein only; 'kl' raises): no (B, item_size) distance matrix -- the item image is packed once for all batches
        (adt_wdist_pack) and every batch is one adt_full_rank_from call with first_id = 0 (the padding item competes, as in the
        reference).  A batch in which some user has fewer than `topk` unseen items is recomputed by the two-pass form, whose list
        continues into the seen items the way the reference's does.

        rowwise=True on a 'kl' model (fused=True still raises): the ranking by the row-wise KL divergence the model is trained on, not
        by kl_predict_full's batch-dependent score -- kl_row_image() packed once, every batch one rank_full(first_id=0, rowwise=True).
        There is no matrix form to fall back to: a row with fewer than `topk` unseen items keeps its -1 tail, which holds no held-out
        item (one is never in the seen list) and which the metrics count as no hit."""
        preds, answers = [], []
        m = self.model
        dev = m.dev
        image = m.item_image() if fused else None
        rowwise = self._rowwise_kl(rowwise)
        row_image = m.kl_row_image() if rowwise else None
        self.fused_fallbacks = 0

        def two_pass(input_ids, indptr, indices):
            return ops.topk_masked(m.predict_full(input_ids), topk, indptr, indices).cpu().numpy().astype(np.int64)
        for input_ids, seen, ans in batches:
            indptr, indices = _seen(seen, len(input_ids), dev)
            if indices is not None and indices.numel() == 0:      # a device pair that lists nothing: as the host forms, no seen list
                indptr, indices = None, None
            if rowwise:
                preds.append(m.rank_full(input_ids, None, (indptr, indices), topk, row_image, first_id=0, rowwise=True)[2].cpu().numpy().astype(np.int64))
            elif fused:
                _, _, top_idx, _ = m.rank_full(input_ids, None, (indptr, indices), topk, image, first_id=0)
                ids, fell_back = fused_ids_or_two_pass(top_idx, lambda: two_pass(input_ids, indptr, indices))
                self.fused_fallbacks += int(fell_back)
                preds.append(ids)
            else:
                preds.append(two_pass(input_ids, indptr, indices))
            answers.append(np.asarray(ans))
        return np.concatenate(preds), np.concatenate(answers)

    @torch.no_grad()
    def full_sort_scores(self, batches, topk=40, fused=False, rowwise=False):
        """full_sort + get_full_sort_score without the id lists leaving the GPU: the same loop over the same
        batches, both distance metrics ('kl' two-pass only: fused=True raises as in full_sort), but every batch's (B, topk) device ids go
        straight into ops.hit_hist with the batch's held-out ids (one per user; uploaded as int32 when they arrive as numpy, used where
        they are when they are a device tensor).  Nothing is copied from the device until the one copy of the histogram after the last
        batch.  Returns (scores -- the 13 numbers of get_full_sort_score, by scores_from_hist --, hist (topk + 1,) numpy int64).

        A batch is (input_ids, seen, answers), (input_ids, seen, answers, min_unseen) or the dict of DeviceDisenData.eval_stage.
        fused=True recomputes a batch two-pass when some row could come back short, decided from host data: a row has
        item_size - (its seen count) candidates (first_id = 0: all item_size ids compete), so the batch falls back when the smallest such
        count is below topk.  The count comes from the host indptr of a host `seen` (a repeated stored id only makes it larger: more
        fallbacks, never fewer, and the two-pass form is the reference's own); for a device (indptr, indices) pair the caller passes it as
        min_unseen.  Sets self.fused_fallbacks as full_sort does.  rowwise: as full_sort; no batch falls back and min_unseen is not read."""
        hist = self.full_sort_hist(batches, topk, fused, rowwise).cpu().numpy()
        return scores_from_hist(hist), hist

    @torch.no_grad()
    def full_sort_hist(self, batches, topk=40, fused=False, rowwise=False):
        """The loop of full_sort_scores; returns the (topk + 1,) int64 histogram still on the device (data-parallel callers all-reduce it
        before the copy)."""
        m = self.model
        dev = m.dev
        image = m.item_image() if fused else None
        rowwise = self._rowwise_kl(rowwise)
        row_image = m.kl_row_image() if rowwise else None
        self.fused_fallbacks = 0
        hist = torch.zeros(1, topk + 1, device=dev, dtype=torch.int64)
        for batch in batches:
            if isinstance(batch, dict):
                input_ids, seen, ans, min_unseen = batch["inp"], (batch["indptr"], batch["indices"]), batch["answers"], batch["min_unseen"]
            else:
                input_ids, seen, ans = batch[:3]
                min_unseen = batch[3] if len(batch) > 3 else None
            B = len(input_ids)
            if isinstance(seen, tuple) and all(x is None or isinstance(x, torch.Tensor) for x in seen):
                indptr, indices = seen
                if fused and min_unseen is None and indices is not None and indices.numel() > 0:
                    raise _lib.AdtError("full_sort_scores(fused=True): a device seen list needs the batch's smallest unseen count (min_unseen; "
                                        "DeviceDisenData.eval_stage gives it): it is not read back from the device")
            else:
                ip, ix = ops.seen_csr_host(seen, B)
                min_unseen = m.item_size if ip is None else m.item_size - int(np.diff(ip[:B + 1]).max())
                indptr, indices = (None, None) if ip is None else (torch.from_numpy(ip).to(dev), torch.from_numpy(ix).to(dev))
            if indices is not None and indices.numel() == 0:      # as full_sort: a pair that lists nothing is no seen list
                indptr, indices, min_unseen = None, None, m.item_size
            if not isinstance(ans, torch.Tensor):
                ans = np.asarray(ans)
                assert ans.ndim == 1 or ans.shape[1] == 1, "scores_from_hist needs one held-out item per user"
                ans = torch.from_numpy(np.ascontiguousarray(ans.reshape(-1), dtype=np.int32)).to(dev)
            if rowwise:
                top_idx = m.rank_full(input_ids, None, (indptr, indices), topk, row_image, first_id=0, rowwise=True)[2]
            elif fused and min_unseen >= topk:
                top_idx = m.rank_full(input_ids, None, (indptr, indices), topk, image, first_id=0)[2]
            else:
                self.fused_fallbacks += int(bool(fused))
                top_idx = ops.topk_masked(m.predict_full(input_ids), topk, indptr, indices)
            ops.hit_hist(top_idx, ans, hist=hist)
        return hist[0]


def recall_at_k(actual, predicted, topk):
    """stosa/utils.py:228-242: mean over the users that have answers of |top-k hits| / |answers|."""
    s, n = 0.0, 0
    for a, p in zip(actual, predicted):
        a = set(int(x) for x in a)
        if a:
            s += len(a & set(int(x) for x in p[:topk])) / float(len(a))
            n += 1
    return s / n


def ndcg_k(actual, predicted, topk):
    """stosa/utils.py:327-345 (ideal DCG over min(topk, |answers|) positions, 1.0 when that is empty)."""
    res = 0.0
    for a, p in zip(actual, predicted):
        aset = set(int(x) for x in a)
        idcg = sum(1.0 / np.log2(i + 2) for i in range(min(topk, len(a)))) or 1.0
        res += sum(1.0 / np.log2(j + 2) for j in range(topk) if int(p[j]) in aset) / idcg
    return res / float(len(actual))


def cal_mrr(actual, predicted):
    """stosa/utils.py:244-267: reciprocal rank of the first hit in the predicted list, averaged over all users."""
    s = 0.0
    for a, p in zip(actual, predicted):
        aset = set(int(x) for x in a)
        hits = [j for j, it in enumerate(p) if int(it) in aset]
        if hits:
            s += 1.0 / (hits[0] + 1)
    return s / float(len(predicted))


def get_full_sort_score(answers, pred_list):
    """Trainer.get_full_sort_score (stosa/trainer.py:62-86): [HIT@1, NDCG@1, HIT@5, NDCG@5, ... @10, @15, @20, @40, MRR]."""
    out = []
    for k in (1, 5, 10, 15, 20, 40):
        out += [recall_at_k(answers, pred_list, k), ndcg_k(answers, pred_list, k)]
    return out + [cal_mrr(answers, pred_list)]


_SCORE_KS = (1, 5, 10, 15, 20, 40)


def scores_from_hist(hist_row):
    """get_full_sort_score from the histogram of hit positions (ops.hit_hist), on the host in float64.  hist_row: one
    (K + 1,) integer row h, h[j] = the users whose held-out item stands at position j of their top-K list, h[K] = those whose list does
    not hold it; N = sum(h).  HIT@k = sum(h[:k]) / N, NDCG@k = sum_{j<k} h[j] / log2(j + 2) / N, MRR = sum_{j<K} h[j] / (j + 1) / N.

    Precondition: every user has exactly ONE held-out item (DisenDataset._views and DeviceDisenData.answers produce nothing else).  Then
    the ideal DCG is 1, recall is hit / 1 and the first hit is the only one, so the three metrics depend on the hit position alone.
    K >= 40, the largest k reported; otherwise AdtError."""
    h = np.asarray(hist_row)
    if h.ndim != 1 or not np.issubdtype(h.dtype, np.integer):
        raise _lib.AdtError("scores_from_hist: one (K + 1,) integer row, got %s %s" % (h.dtype, h.shape))
    K = h.size - 1
    if K < _SCORE_KS[-1]:
        raise _lib.AdtError("scores_from_hist: K=%d < %d, the largest k reported" % (K, _SCORE_KS[-1]))
    n = float(h.sum())
    if n <= 0:
        raise _lib.AdtError("scores_from_hist: an empty histogram")
    hf = h[:K].astype(np.float64)
    j = np.arange(K, dtype=np.float64)
    gain = hf / np.log2(j + 2.0)
    out = []
    for k in _SCORE_KS:
        out += [float(hf[:k].sum() / n), float(gain[:k].sum() / n)]
    return out + [float((hf / (j + 1.0)).sum() / n)]
