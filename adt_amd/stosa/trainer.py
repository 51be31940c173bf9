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

from .. import ops
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
        m.loss_forward_backward(st, self.lambda1, self.lambda2, st["norms"], self.loss_slots, b_offset)
        self._buckets.finish()
        ops.clip_adam_l2(m.flat, m.flat_grad, self.m, self.v, self.wd, self.clip, self.lr, self.betas[0], self.betas[1], self.eps, self.scal,
                         n=m.n_trained_floats)

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
    @torch.no_grad()
    def full_sort(self, batches, topk=40, fused=False):
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
        continues into the seen items the way the reference's does."""
        preds, answers = [], []
        m = self.model
        dev = m.dev
        image = m.item_image() if fused else None
        self.fused_fallbacks = 0

        def two_pass(input_ids, indptr, indices):
            return ops.topk_masked(m.predict_full(input_ids), topk, indptr, indices).cpu().numpy().astype(np.int64)
        for input_ids, seen, ans in batches:
            indptr, indices = _seen(seen, len(input_ids), dev)
            if indices is not None and indices.numel() == 0:      # a device pair that lists nothing: as the host forms, no seen list
                indptr, indices = None, None
            if fused:
                _, _, top_idx, _ = m.rank_full(input_ids, None, (indptr, indices), topk, image, first_id=0)
                ids, fell_back = fused_ids_or_two_pass(top_idx, lambda: two_pass(input_ids, indptr, indices))
                self.fused_fallbacks += int(fell_back)
                preds.append(ids)
            else:
                preds.append(two_pass(input_ids, indptr, indices))
            answers.append(np.asarray(ans))
        return np.concatenate(preds), np.concatenate(answers)


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
