"""SuperBertModel on the MI355X hot path -- drop-in for the reference's bert4rec/model/superbert.py (+ SuperEncoder / SuperDecoder,
bert4rec/model/modules.py:217-259, :356-393, base_super_modules.py): the weight-sharing BERT4Rec-ADT supernet that
bert4rec/evolution.py warms up and scores.

Differences from BertModel that the reference's supernet has and this one keeps: the vocabulary is itemnum + 2 (superbert.py:21), the
feed-forward width is 4 * hidden_units (:35), every depth holds rec_size * ind_size candidate encoder and decoder layers;
`set_choice(block_cand)` selects four of them per depth.  The encoder mixes the four candidates' outputs and head-classifier scores
with the bilinear weights and applies log_softmax to the mixed scores (modules.py:250-258); the DECODER sums its four candidates
WITHOUT the weights (modules.py:386-390: `seqs_list.append(c_logits)`).  The classifier scores are mixed as log-probabilities here:
log_softmax(sum_k w_k (z_k - lse_k)) == log_softmax(sum_k w_k z_k) because each lse_k is constant along the softmax axis.

Every candidate layer runs on the same stage kernels as BertModel (adt_amd/bert4rec/model.py); `SuperBertTrainer.step` is the loop
body of SearcherEvolution._train_warmup (bert4rec/evolution.py:266-296): CE over the masked positions + rec_weights[i] * MSE +
ind_weights[stale i] * NLL, clip_grad_norm_, torch.optim.AdamW (decoupled decay) with torch's bookkeeping for parameters whose grad is
None (candidates that were not selected keep their moments, their own step count, and are not decayed).
"""
import math

import numpy as np
import torch

from .. import ops
from ..supersearch import SupernetTrainer, candidate_features, get_shared
from ..wide import Act, Tape, loss_norms
from .model import SITE_EMB_DEC, SITE_EMB_SEQ, BertModel, dec_sites, enc_sites

CAND_SITE = 4096


def _cand_sites(sites, k):
    """Dropout sites of candidate slot k of a depth: every selected layer draws its own stream."""
    return {n: v + CAND_SITE * (k + 1) for n, v in sites.items()}


class SuperBertModel(BertModel):
    def __init__(self, usernum, itemnum, rec_choice, ind_choice, args, allow_lanes=False):
        """allow_lanes: every (hidden_units, num_heads) BertModel takes is opt-in (bert4rec/evolution.py passes True):
        the padded tables with `block` candidate layers per depth.  Without it a width the kernels do not tile raises, as it always has;
        a tiled width runs the same code with or without it."""
        self.rec_choice, self.ind_choice = np.asarray(rec_choice, np.float64), np.asarray(ind_choice, np.float64)
        self.block = len(self.rec_choice) * len(self.ind_choice)
        super().__init__(usernum, itemnum, args, vocab=itemnum + 2, inner_units=4 * args.hidden_units, block=self.block,
                         allow_block_lanes=bool(allow_lanes))
        # SearcherEvolution._generate_supernet (bert4rec/evolution.py:104-112): trunc_normal_(std = initializer_range) on every tensor
        # whose name holds neither 'layer_norm' nor 'bias'; the others keep torch's constructor defaults (LayerNorm 1 / 0, mask_bias 0,
        # Linear bias U(-1/sqrt(fan_in), 1/sqrt(fan_in))).  Shapes and fans are the reference's: at a padded width the live lanes only
        # are written (R(): the reference-shaped parameters), then pushed
        g = torch.Generator(device="cpu").manual_seed(torch.initial_seed() % (1 << 31))
        std = float(getattr(args, "initializer_range", 0.02))
        ref_table = [(name, (self._ref_views or self._views)[name][2]) for name, _ in self.table]
        shapes = dict(ref_table)
        for name, shape in ref_table:
            v = self.R(name)
            if "layer_norm" in name:
                v.fill_(1.0 if name.endswith("weight") else 0.0)
            elif name == "mask_bias":
                v.zero_()
            elif "bias" in name:
                fan_in = shapes[name[:-4] + "weight"][1]
                v.copy_((torch.rand(shape, generator=g) * 2 - 1) / math.sqrt(fan_in))
            else:
                t = torch.empty(shape)
                torch.nn.init.trunc_normal_(t, std=std, generator=g)
                v.copy_(t)
        self.push()
        self.shared = [((0, 0, 0, 0), (0.0, 0.0, 0.0, 0.0)) for _ in range(self.num_layers)]

    def set_choice(self, cand):
        """superbert.py:121-123 / base_super_modules.py:42-57."""
        self.shared = get_shared(self.rec_choice, self.ind_choice, np.asarray(cand, np.float64))

    def layer_range(self, kind, depth, cand):
        """Flat [lo, hi) of one candidate layer (its tensors are consecutive in the table)."""
        p = "%s.%s_layers.%d.%d." % (kind, kind, depth, cand)
        names = [n for n, _ in self.table if n.startswith(p)]
        lo = self._views[names[0]][0]
        o, n, _ = self._views[names[-1]]
        return lo, o + (n + 3) // 4 * 4

    def shared_ranges(self):
        """Flat ranges torch's optimizer would step: everything outside the candidate layers + the selected candidates."""
        first = self._views["encoder.encoder_layers.0.0.multi_head_attention.query_transfer.weight"][0]
        tail = self._views["mask_trans_feat.weight"][0]
        ranges = [(0, first), (tail, self.flat.numel())]
        for depth, (idxs, _) in enumerate(self.shared):
            for idx in sorted(set(idxs)):
                ranges += [self.layer_range("encoder", depth, idx), self.layer_range("decoder", depth, idx)]
        return ranges

    # ------------------------------------------------------------------------------------------------------------------
    def _encode(self, tp, src, B):
        """log2feats + SuperEncoder.forward (superbert.py:66-73, modules.py:243-259)."""
        x = self._embed(tp, src, SITE_EMB_SEQ)
        enc_inputs, recs = [], []
        for i, (idxs, ws) in enumerate(self.shared):
            enc_inputs.append(x)
            outs, inds = [], []
            for k, (idx, w) in enumerate(zip(idxs, ws)):
                y, rec = self._enc_layer(tp, "encoder.encoder_layers.%d.%d" % (i, idx), x, src, B, _cand_sites(enc_sites(i), k))
                outs.append((y, float(w)))
                inds.append((rec, float(w)))
            x = tp.mix(outs)
            recs.append(tp.log_softmax(tp.mix(inds), self.num_heads))
        return x, enc_inputs, recs

    def _decode(self, tp, dec, src, enc, B):
        """decode + SuperDecoder.forward (superbert.py:75-84, modules.py:382-393): the four candidates are SUMMED, unweighted."""
        x = self._embed(tp, dec, SITE_EMB_DEC)
        tp.mark_decoder_start()
        outs = []
        for i, (idxs, _) in enumerate(self.shared):
            parts = [(self._dec_layer(tp, "decoder.decoder_layers.%d.%d" % (i, idx), x, dec, src, enc, B, _cand_sites(dec_sites(i), k)), 1.0)
                     for k, idx in enumerate(idxs)]
            x = tp.mix(parts)
            outs.append(x)
        return outs

    def _candidate_head_rows(self, seqs, shared_list, stats=None):
        """(h, B): the head's input to the item scores at the last position under EVERY block choice of `shared_list`, (P * B, d) stacked
        group-major.  One pass: depth-0 layers shared between candidates, deeper layers once per distinct layer on the stacked inputs
        (supersearch.candidate_features)."""
        src = self.ids(seqs)
        B, L = src.shape
        was = self.training
        self.eval()
        self.push()      # padded widths: the reference-shaped parameters are the truth between steps (no-op otherwise)
        tp = Tape(self, self.prec, False)
        flat = src.view(-1)
        x0 = self._embed(tp, flat, SITE_EMB_SEQ)

        def run_layer(depth, idx, x, n):
            ids = flat if n == 1 else flat.repeat(n)
            y, _ = self._enc_layer(tp, "encoder.encoder_layers.%d.%d" % (depth, idx), Act(x[0]), ids, B * n, enc_sites(depth))
            # no backward follows: drop the layer's closures now, and with them its intermediate activations.  Left on the tape (which
            # they reference back, so only the cycle collector frees them) they add up over the stacked layers of a pass: at the ml-1m
            # template shape, about 1 GB per layer evaluation of 256 sequences
            del tp.bw[:]
            return (y.t,)
        feats = candidate_features(run_layer, (x0.t,), shared_list, self.num_layers, stats=stats)
        P = len(shared_list)
        F = feats[0][0] if P == 1 else torch.cat([f[0] for f in feats], 0)
        rows = torch.arange(L - 1, P * B * L, L, device=self.dev, dtype=torch.int32)
        h = self._head(tp, Act(ops.gather_rows(F, rows)))
        del tp.bw[:]
        self.train(was)
        return h.t, B

    @torch.no_grad()
    def predict_rank_candidates(self, seqs, candidates, shared_list, stats=None):
        """Ranks of the positive (column 0 of `candidates`) at the last position under EVERY block choice of `shared_list`: (P, B), in one
        pass (_candidate_head_rows)."""
        cand = self.ids(candidates)
        h, B = self._candidate_head_rows(seqs, shared_list, stats)
        P = len(shared_list)
        if P > 1:
            cand = cand.repeat(P, 1)
        _, rank = ops.score_rank_bias(h, self.dp, self.P("item_emb.word_emb.weight"), self.P("mask_bias"), cand, P * B, cand.shape[1], True)
        return rank.view(P, B)

    @torch.no_grad()
    def rank_hist_candidates(self, seqs, candidates, shared_list, hist, stats=None):
        """predict_rank_candidates with the scores counted on the device: the same pass, then adt_cand_rank_hist on the stacked rows with
        rows_per_group = B, so the (B, C) candidates are read by every group and not repeated P times, and the ranks are counted into hist
        (P, C) int64 (accumulated in place; returned) instead of being read back.  seqs / candidates: host arrays or device int32."""
        cand = self.ids(candidates)
        h, B = self._candidate_head_rows(seqs, shared_list, stats)
        return ops.cand_rank_hist(h, h.stride(0), self.P("item_emb.word_emb.weight"), cand, len(shared_list) * B, rows_per_group=B, hist=hist,
                                  bias=self.P("mask_bias"))


class SuperBertTrainer(SupernetTrainer):
    """SearcherEvolution._train_warmup's optimiser step (bert4rec/evolution.py:266-296) with torch.optim.AdamW's bookkeeping (decoupled decay)."""

    _adam_range = staticmethod(ops.adamw_range)

    def __init__(self, model, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, clip=5.0, seed=2022):
        super().__init__(model, 1 + 2 * model.num_layers, lr, betas, eps, weight_decay, clip, seed)
        self._norms = {}      # step_device: rows -> device normalisers

    def _stage(self, src, dec, labels):
        m = self.model
        st = m.stage(src, dec, labels)
        return st, loss_norms(m, st["B"] * m.maxlen)

    def _device_norms(self, st):
        """step_device (DeviceBertData.train_stage): one loss_norms per row count, kept, so a step uploads nothing -- as
        FusedBertTrainer.step_device does.  The masked-row count stays on the device; the masked-row GEMMs are launched for B * L rows."""
        if st["B"] not in self._norms:
            self._norms[st["B"]] = loss_norms(self.model, st["B"] * self.model.maxlen)
        return self._norms[st["B"]]

    def _ind_lambdas(self):
        nl = self.model.num_layers
        return [self.ind_weights[nl - 1]] * nl        # `ind_weights[i]` with the reconstruction loop's stale i (evolution.py:291)

    def _loss_w(self):
        m = self.model
        nl = m.num_layers
        return [1.0] + list(self.rec_weights) + [self.ind_weights[nl - 1] if m.num_heads > 1 else 0.0] * nl
