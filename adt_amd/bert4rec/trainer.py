"""Fused training step for BERT4Rec-ADT: the loop body of the reference's BertTrainer.train (bert4rec/trainer.py:100-138:
forward, CE + reconstruction + independence losses, backward, clip_grad_norm_, Adam with coupled weight decay) as one
device-side launch sequence, optionally replayed from a HIP graph, plus the evaluate() ranking metrics (:49-86).

Data-parallel (one process per GPU, torch.distributed "nccl" = RCCL over xGMI): every rank runs the same sequence on
its contiguous slice of the batch with GLOBAL loss normalisers (count of labels != 0, B*L*d, B*L*H of the whole batch)
and GLOBAL dropout indices; the flat gradient buffer is summed with one all-reduce; clipping and Adam run identically
on every rank on the reduced buffer.
"""
import numpy as np
import torch

from .. import ops
from .._lib import AdtError
from ..dp import reduce_sum
from ..wide import TapeTrainer, loss_norms


class FusedBertTrainer(TapeTrainer):
    def __init__(self, model, lambda1, lambda2, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, clip=5.0, process_group=None,
                 use_graph=False, seed=23, mcap_frac=1.0):
        self.lambda1, self.lambda2 = [float(x) for x in lambda1], [float(x) for x in lambda2]
        assert len(self.lambda1) == model.num_layers and len(self.lambda2) == model.num_layers
        # tail bucket: decoder layers + output head (their backward runs first); head bucket: embeddings (word_emb also receives
        # the all-item-logits gradient) + encoder, reduced at the end
        super().__init__(model, [1.0] + self.lambda1 + self.lambda2, "decoder.decoder_layers.0.dec_multi_head_attention.query_transfer.weight",
                         lr, betas, eps, weight_decay, clip, process_group, use_graph)
        self.norms = torch.zeros(3, device=model.dev, dtype=torch.float32)
        self.mcap_frac = float(mcap_frac)   # the masked-row GEMMs are launched for at most this fraction of B*L rows
        self._device_norms = {}             # step_device: (rows, global rows) -> device normalisers
        model.seed_trainer(seed)

    # ------------------------------------------------------------------------------------------------------------------
    def stage(self, src, dec, labels, n_valid_global=None, norms_scale=1):
        """Upload one batch; n_valid_global / norms_scale give the GLOBAL normalisers under data parallelism."""
        m = self.model
        st = m.stage(src, dec, labels, n_valid_global)
        T = st["B"] * m.maxlen
        st["norms"] = loss_norms(m, T, scale=norms_scale)
        cap = int(np.ceil(self.mcap_frac * T))
        over = st["M_host"] > cap
        if self.world > 1:      # every rank must reach the same decision, or the ranks that go on hang in the gradient all-reduce
            t = torch.tensor([1.0 if over else 0.0], device=m.dev)
            torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX, group=self.pg)
            over = bool(t.item() > 0)
        if over:
            raise ValueError("a rank's shard has more masked rows than the capacity %d (this rank: %d; mcap_frac=%g)" % (cap, st["M_host"], self.mcap_frac))
        return st

    def _body(self, st, b_offset):
        m = self.model
        T = st["B"] * m.maxlen
        m.push()        # padded widths: the reference-shaped parameters are the truth between steps (no-op otherwise)
        m.loss_forward_backward(st, self.lambda1, self.lambda2, st["norms"], self.loss_slots, b_offset, int(np.ceil(self.mcap_frac * T)))
        self._buckets.finish()
        # pad weights and pad gradients are exact zeros, so the coupled weight decay keeps them zero
        ops.clip_adam_l2(m.flat, m.flat_grad, self.m, self.v, self.wd, self.clip, self.lr, self.betas[0], self.betas[1], self.eps, self.scal)
        m.pull()

    def step(self, src, dec, labels, n_valid_global=None, b_offset=0, norms_scale=1):
        self.step_staged(self.stage(src, dec, labels, n_valid_global, norms_scale), b_offset)

    def step_device(self, st, b_offset=0):
        """One step on a batch that is on the device already (DeviceBertData.train_stage): adds the normalisers -- kept per
        (rows, global rows), so a step uploads nothing -- and runs step_staged.  Under data parallelism st holds this rank's rows of a
        batch of st["B_global"] examples and b_offset is the first of them.  The masked-row count stays on the device, so the capacity
        check of stage() cannot be made: only mcap_frac = 1.0 is accepted, where the capacity is B * L and cannot be exceeded."""
        if self.mcap_frac != 1.0:
            raise AdtError("step_device: mcap_frac = %g needs the masked-row count on the host (stage / step); use mcap_frac = 1.0" % self.mcap_frac)
        key = (st["B"], st.get("B_global", st["B"]))
        if key not in self._device_norms:
            self._device_norms[key] = loss_norms(self.model, key[0] * self.model.maxlen, scale=key[1] / float(key[0]))
        self.step_staged(dict(st, norms=self._device_norms[key]), b_offset)

    # ------------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def evaluate(self, batches, ks=(5, 10), device_scores=False):
        """BertTrainer.evaluate (trainer.py:49-86) over an iterable of (seq (B, L), candidates (B, C)) -- host arrays or device int32
        tensors (DeviceBertData.eval_batch), which are used where they are -- with the positive in column 0: rank = number of
        candidates scored above it, HR@k, NDCG@k, and the AUC with the reference's candidates_size = 1 + C.  device_scores (DESIGN.md
        section 28): the ranks are counted on the device and one histogram is read after the last batch (_evaluate_hist)."""
        self.model.eval()
        ks = tuple(ks)
        if device_scores:
            return self._evaluate_hist(batches, ks)
        # additive statistics [n, sum of AUC terms, per k: hits, sum 1/log2(rank+2)]: under data parallelism rank r scores batches
        # r, r+W, ... and the statistics are sum-reduced in float64, so every rank ends up with the metrics of the whole user set
        stats = np.zeros(2 + 2 * len(ks), np.float64)
        for i, (seq, cand) in enumerate(batches):
            if i % self.world != self.rank:
                continue
            _, rank = self.model.predict(None, seq, None, None, cand, want_rank=True)
            r = rank.cpu().numpy().astype(np.int64)
            size = 1 + (cand if isinstance(cand, torch.Tensor) else np.asarray(cand)).shape[1]
            stats[0] += len(r)
            stats[1] += float(((size - (r + 1)) / (size - 1)).sum())
            for j, k in enumerate(ks):
                stats[2 + 2 * j] += float((r < k).sum())
                stats[3 + 2 * j] += float((1.0 / np.log2(r[r < k] + 2)).sum())
        if self.world > 1:
            t = torch.from_numpy(stats).to(self.model.dev)
            stats = reduce_sum(t, self.pg).cpu().numpy()
        n = stats[0]
        ndcg = {k: float(stats[3 + 2 * j] / n) for j, k in enumerate(ks)}
        hr = {k: float(stats[2 + 2 * j] / n) for j, k in enumerate(ks)}
        return (ndcg, hr), float(stats[1] / n)

    def _evaluate_hist(self, batches, ks):
        """evaluate() without a copy per batch: every batch is encoded as predict() encodes it (_full_rank_operands: the head rows of the
        last position) and scored, ranked and counted by adt_cand_rank_hist into one (1, C) int64 histogram, which is read once and
        turned into the metrics by metrics_from_hist with the same n_candidates = C (size = 1 + C).  Under data parallelism rank r
        takes batches r, r + W, ... as evaluate() does and the histogram is sum-reduced: integers, so the result is exact."""
        from ..sasrec.utils import metrics_from_hist
        m = self.model
        C, hist = None, None
        for i, (seq, cand) in enumerate(batches):
            c = (cand if isinstance(cand, torch.Tensor) else np.asarray(cand)).shape[1]
            if C is None:       # every rank sees every batch's shape, so all of them reach the same decision
                C, hist = c, torch.zeros(1, c, device=m.dev, dtype=torch.int64)
            elif c != C:
                raise AdtError("evaluate(device_scores=True): batch %d has %d candidates, the first batch has %d (one histogram per pass)" % (i, c, C))
            if i % self.world != self.rank:
                continue
            cand = m.ids(cand)
            F, E, _, bias = m._full_rank_operands(seq)
            ops.cand_rank_hist(F, F.stride(0), E, cand, cand.shape[0], cand.shape[0], hist=hist, bias=bias)
        if C is None:
            raise AdtError("evaluate(device_scores=True): no batches")
        if self.world > 1:
            if torch.distributed.get_backend(self.pg) == "nccl":
                torch.distributed.all_reduce(hist, group=self.pg)
            else:
                h = hist.cpu()
                torch.distributed.all_reduce(h, group=self.pg)
                hist = h
        return metrics_from_hist(hist.cpu().numpy()[0], C, ks)
