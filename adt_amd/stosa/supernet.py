"""DisenDistSASupernet on the MI355X hot path -- drop-in for the reference's stosa/supernet.py (+ SuperDistSAEncoder /
SuperDistSADecoder, stosa/super_modules.py:63-136): the weight-sharing STOSA-ADT supernet that stosa/searcher.py warms up and
scores.

Per depth there are rec_size * ind_size candidate encoder and decoder layers; `set_choice(block_cand)` selects four of them and their
bilinear weights.  Unlike the SASRec / BERT4Rec supernets the four selected layers are CHAINED: the reference's inner loop rebinds
`mean_hidden_states, cov_hidden_states` to each candidate's output, so candidate k+1 reads candidate k's output, and the four
intermediate results are mixed with the weights (super_modules.py:81-95, :123-133; encoder and decoder alike).  The head-classifier
scores are mixed and log_softmax'd (:96-97); they are mixed as log-probabilities here, which is the same function (each candidate's
log-sum-exp is constant along the softmax axis).  The supernet has no decLayerNorm (supernet.py:10-19).

Every candidate layer runs on the stage kernels of DisenDistSAModel (adt_amd/stosa/models.py); `SuperStosaTrainer.step` is the loop
body of SuperDistSAModelTrainer.iteration (stosa/super_trainer.py:205-235): BPR + pvn + lambda1[l] * MSE (mean and covariance) +
lambda2[l] * NLL (mean and covariance), Adam with coupled weight decay, torch's bookkeeping for parameters whose grad is None.
"""
import numpy as np
import torch

from .. import _lib, ops
from ..supersearch import SupernetTrainer, candidate_features, get_shared
from ..wide import Act, Tape, loss_norms
from .models import SITE_EMB, DisenDistSAModel, dec_sites, enc_sites

CAND_SITE = 4096


def _cand_sites(sites, k):
    return {n: v + CAND_SITE * (k + 1) for n, v in sites.items()}


class DisenDistSASupernet(DisenDistSAModel):
    def __init__(self, args, rec_choice, ind_choice, allow_kl=False, allow_lanes=False):
        """allow_kl: distance_metric='kl' is opt-in (SearcherEvolution passes True).  Without it the constructor refuses anything but
        'wasserstein', as it always has; with it 'kl' runs the KL attention, the KL warm-up loss and the grouped KL full sort (DESIGN.md
        section 19), and any other string still raises in the base class.
        allow_lanes: every (hidden_units, num_heads) DisenDistSAModel takes with allow_kl_lanes=True and allow_wide_heads=True is opt-in too
        (SearcherEvolution passes True): padded widths (50 / 1, 100 / 2) and heads of 128 lanes (128 / 1, 100 / 1).
        Without it such a shape raises, as it always has; a shape the kernels tile runs the same code with or without it."""
        if getattr(args, "distance_metric", "wasserstein") != "wasserstein" and not allow_kl:
            raise _lib.AdtError("DisenDistSASupernet (adt_amd): only distance_metric='wasserstein' is built for the supernet unless allow_kl=True "
                                "is passed, got %r" % (args.distance_metric,))
        self.rec_choice, self.ind_choice = np.asarray(rec_choice, np.float64), np.asarray(ind_choice, np.float64)
        self.block = len(self.rec_choice) * len(self.ind_choice)
        lanes = bool(allow_lanes)
        super().__init__(args, block=self.block, dec_layernorm=False, allow_kl_lanes=lanes, allow_wide_heads=lanes,
                         allow_block_lanes=lanes)                         # init_weights is the plain model's (supernet.py:101-111)
        self.shared = [((0, 0, 0, 0), (0.0, 0.0, 0.0, 0.0)) for _ in range(self.num_layers)]

    def set_choice(self, cand):
        """supernet.py:113-115 / super_modules.py:45-58 (encoder and decoder receive the same choice)."""
        self.shared = get_shared(self.rec_choice, self.ind_choice, np.asarray(cand, np.float64))

    def layer_range(self, kind, depth, cand):
        """Flat [lo, hi) of the trained tensors of one candidate layer (consecutive in the table; a decoder layer's dec_attention
        lives in the untrained tail)."""
        p = "%s.layer.%d.%d." % (kind, depth, cand)
        names = [n for n, _ in self.table if n.startswith(p) and ".dec_attention." not in n]
        lo = self._views[names[0]][0]
        o, n, _ = self._views[names[-1]]
        return lo, o + (n + 3) // 4 * 4

    def shared_ranges(self):
        """Flat ranges torch's optimizer would step: the embeddings + LayerNorm, and the selected candidate layers."""
        ranges = [(0, self._views["item_encoder.layer.0.0.attention.mean_query.weight"][0])]
        for depth, (idxs, _) in enumerate(self.shared):
            for idx in sorted(set(idxs)):
                ranges += [self.layer_range("item_encoder", depth, idx), self.layer_range("item_decoder", depth, idx)]
        return ranges

    def _finetune(self, tp, inp, dec, B):
        """finetune's token-major body with the super encoder / decoder (supernet.py:55-99, super_modules.py:75-136)."""
        m, c = self._embed(tp, inp, "mean", SITE_EMB["seq_mean"]), self._embed(tp, inp, "cov", SITE_EMB["seq_cov"])
        dm, dc = self._embed(tp, dec, "mean", SITE_EMB["dec_mean"]), self._embed(tp, dec, "cov", SITE_EMB["dec_cov"])
        enc_inputs, enc_recs, dec_outs = [], [], []
        H = self.num_heads
        for i, (idxs, ws) in enumerate(self.shared):
            enc_inputs.append((m, c))
            ms, cs, rms, rcs = [], [], [], []
            for k, (idx, w) in enumerate(zip(idxs, ws)):
                m, c, rm, rc = self._enc_layer(tp, "item_encoder.layer.%d.%d" % (i, idx), m, c, inp, B, _cand_sites(enc_sites(i), k))   # chained
                ms.append((m, float(w))); cs.append((c, float(w))); rms.append((rm, float(w))); rcs.append((rc, float(w)))
            m, c = tp.mix(ms), tp.mix(cs)
            enc_recs.append((tp.log_softmax(tp.mix(rms), H), tp.log_softmax(tp.mix(rcs), H)))
        tp.mark_decoder_start()
        for i, (idxs, ws) in enumerate(self.shared):
            ms, cs = [], []
            for k, (idx, w) in enumerate(zip(idxs, ws)):
                dm, dc = self._dec_layer(tp, "item_decoder.layer.%d.%d" % (i, idx), dm, dc, m, c, inp, B, _cand_sites(dec_sites(i), k))  # chained
                ms.append((dm, float(w))); cs.append((dc, float(w)))
            dm, dc = tp.mix(ms), tp.mix(cs)
            dec_outs.append((dm, dc))
        return m, c, enc_inputs, enc_recs, dec_outs

    @torch.no_grad()
    def _last_state_candidates(self, input_ids, shared_list, stats=None):
        """(mean, covariance) (P * B, d) of the last position under EVERY block choice of `shared_list`, candidate-major.  One pass: chain
        prefixes of depth 0 are shared between candidates, deeper links run once per distinct layer on the stacked inputs
        (supersearch.candidate_features, chain=True)."""
        inp = self.ids(input_ids)
        B, L = inp.shape
        was = self.training
        self.eval()
        self.push()      # padded widths: the reference-shaped parameters are the truth between steps (no-op otherwise)
        tp = Tape(self, self.prec, False)
        flat = inp.view(-1)
        m0, c0 = self._embed(tp, flat, "mean", SITE_EMB["seq_mean"]), self._embed(tp, flat, "cov", SITE_EMB["seq_cov"])

        def run_layer(depth, idx, x, n):
            ids = flat if n == 1 else flat.repeat(n)
            m, c, _, _ = self._enc_layer(tp, "item_encoder.layer.%d.%d" % (depth, idx), Act(x[0]), Act(x[1]), ids, B * n, enc_sites(depth))
            return (m.t, c.t)
        feats = candidate_features(run_layer, (m0.t, c0.t), shared_list, self.num_layers, chain=True, stats=stats)
        self.train(was)
        P = len(shared_list)
        M = feats[0][0] if P == 1 else torch.cat([f[0] for f in feats], 0)
        C = feats[0][1] if P == 1 else torch.cat([f[1] for f in feats], 0)
        rows = torch.arange(L - 1, P * B * L, L, device=self.dev, dtype=torch.int32)
        return ops.gather_rows(M, rows), ops.gather_rows(C, rows)

    @torch.no_grad()
    def kl_item_image(self):
        """(img (item_size, 2d), lv (item_size,)) of the two item tables for the grouped KL full sort (ops.kldist_pack).  Packed on every
        call, like item_image(): no cache, it is stale after any weight update; a caller that scores many passes under the same weights
        holds on to it and passes it as `image`.  At a padded width: ops.kldist_pack_lanes of the padded tables, (item_size, 2 d_pad) with
        +0.0 on the pad lanes of both halves."""
        self.push()
        Em, Ec = self.P("item_mean_embeddings.weight"), self.P("item_cov_embeddings.weight")
        return ops.kldist_pack(Em, Ec) if self.lanes is None else ops.kldist_pack_lanes(Em, Ec, self.lanes)

    @torch.no_grad()
    def predict_full_candidates(self, input_ids, shared_list, stats=None, image=None):
        """Full-sort distances of the last state to every item under EVERY block choice of `shared_list`: (P * B, item_size),
        candidate-major (the feature pass of _last_state_candidates, then adt_wdist_full).  distance_metric 'kl': kl_predict_full per
        candidate with the B rows of this call as the eval batch (adt_kldist_full_groups with E = B: the chunking never pairs rows of two
        candidates); image: kl_item_image() of the current weights, packed here when None.  The Wasserstein path takes no image."""
        sm, sc = self._last_state_candidates(input_ids, shared_list, stats)
        ln = self.lanes      # a padded width: the lane-aware twins, scores over the live lanes at the true d
        if self.distance_metric == "kl":
            img, lv = self.kl_item_image() if image is None else image
            E = sm.shape[0] // len(shared_list)
            if ln is not None:
                return ops.kldist_full_groups_lanes(sm, sc, img, lv, E, self.item_size, ln)
            return ops.kldist_full_groups(sm, sc, img, lv, E, self.item_size)
        Em, Ec = self.P("item_mean_embeddings.weight"), self.P("item_cov_embeddings.weight")
        return ops.wdist_full(sm, sc, Em, Ec, self.item_size) if ln is None else ops.wdist_full_lanes(sm, sc, Em, Ec, self.item_size, ln)

    @torch.no_grad()
    def rank_full_candidates(self, input_ids, shared_list, targets=None, seen=None, topk=0, image=None, stats=None, first_id=1, rowwise=False):
        """DistRankMixin.rank_full under every block choice of `shared_list` with ONE fused call on the stacked P * B last states:
        (rank, n_elig, top_idx, top_dist) with P * B rows, candidate-major.  targets: (B,) (repeated per candidate), (P * B,) or None;
        seen: the CSR of the P * B stacked rows (any form ops.seen_csr takes, or a device (indptr, indices) pair); image: item_image().
        Wasserstein by default (DistRankMixin._check_wasserstein): the reference's KL score is not a function of (user, item) alone.
        rowwise=True under 'kl' ranks by the row-wise KL divergence instead (DistRankMixin.rank_full); image: kl_row_image(), packed
        once here when None -- the candidates share the item tables."""
        self._rowwise_kl(rowwise)
        sm, sc = self._last_state_candidates(input_ids, shared_list, stats)
        PB = sm.shape[0]
        if targets is not None:
            targets = torch.as_tensor(np.asarray(targets.cpu() if isinstance(targets, torch.Tensor) else targets)).reshape(-1)
            if targets.numel() != PB:
                targets = targets.repeat(len(shared_list))
        return self._rank_states(sm, sc, targets, seen, topk, image, first_id, rowwise)


class SuperStosaTrainer(SupernetTrainer):
    """SuperDistSAModelTrainer.iteration's optimiser step (stosa/super_trainer.py:205-235) with torch.optim.Adam's bookkeeping (coupled
    weight decay); the reference does not clip the gradient: clip = inf."""

    _adam_range = staticmethod(ops.adam_range)

    def __init__(self, model, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, seed=42):
        super().__init__(model, 3 + 4 * model.num_layers, lr, betas, eps, weight_decay, 1e30, seed)

    def _stage(self, input_ids, dec_ids, pos_ids, neg_ids):
        m = self.model
        st = m.stage(input_ids, dec_ids, pos_ids, neg_ids)
        return st, loss_norms(m, st["B"] * m.maxlen)

    def _loss_w(self):
        w = [1.0, 1.0, 0.0]
        for l in range(self.model.num_layers):
            w += [self.rec_weights[l]] * 2
        for l in range(self.model.num_layers):
            w += [self.ind_weights[l]] * 2
        return w
