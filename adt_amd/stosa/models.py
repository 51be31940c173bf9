"""DisenDistSAModel on the MI355X hot path -- drop-in for the reference's stosa/models.py:DisenDistSAModel (STOSA-ADT:
stochastic mean/covariance item embeddings, Wasserstein-distance self-attention, reconstruction decoder, per-head
independence classifiers on both the mean and the covariance contexts).

Same constructor (`DisenDistSAModel(args)`), `finetune(input_ids, dec_ids, user_ids)` 7-tuple and state_dict names /
shapes, `item_mean_embeddings` / `item_cov_embeddings` reachable as attributes (the reference's trainer
reads them directly, stosa/trainer.py:361-364,466-467).  All arithmetic runs in libadt_hip.so: dense layers
(adt_gemm.cuh), the Wasserstein attention and the BPR / full-sort distance kernels (adt_stosa.cuh, exact fp32 wave-level
reductions), LayerNorm / dropout / ELU row kernels.  maxlen up to 1024: past ops.wattn_max_len(head size) rows (256; 141 at head size 64)
the attention runs on the streamed matrix-core kernels of adt_wattn_long.cuh.
Under the Wasserstein distance -- and, with allow_kl_lanes=True, under 'kl'  -- any (hidden_units, num_heads) that wide.padded_layout accepts with heads of up to 64 lanes runs too (50 / 1,
100 / 2, 48 / 4, 150 / 3): activations and parameters are padded to d_pad columns, the registered parameters keep the reference's shapes
(DESIGN.md section 26).  With allow_wide_heads=True heads of 128 lanes run as well (128 / 1, 256 / 2; 100 / 1 and 200 / 2 padded): their attention
is the streamed family at head size 128 (ops.wattn_hd128_* / klattn_hd128_*) at every maxlen.
"""
import math

import numpy as np
import torch

from .. import _lib, custom_ops, ops
from ..fullrank import DistRankMixin
from ..wide import Act, FlatModule, Tape, give, padded_layout

LN_EPS = 1e-12
MAXLEN_MAX = 1024      # the streamed distance attention's bound (ops.wattn_long_fwd)
SITE_EMB = {"seq_mean": 1, "seq_cov": 2, "dec_mean": 3, "dec_cov": 4}


def enc_sites(i):
    b = 16 + 8 * i
    return {"attn": b, "out_mean": b + 1, "out_cov": b + 2, "ffn_mean": b + 3, "ffn_cov": b + 4}


def dec_sites(i):
    b = 128 + 8 * i
    return {"attn": b, "out_mean": b + 1, "out_cov": b + 2, "ffn_mean": b + 3, "ffn_cov": b + 4}


# path components in the order the reference's constructors register them (stosa/models.py:169-178, modules.py)
REF_ORDER = ["item_mean_embeddings", "item_cov_embeddings", "position_mean_embeddings", "position_cov_embeddings", "user_margins",
             "item_encoder", "item_decoder", "layer", "attention", "dec_attention", "enc_attention", "mean_intermediate", "cov_intermediate",
             "mean_independence_layer", "cov_independence_layer", "mean_query", "cov_query", "mean_key", "cov_key", "mean_value",
             "cov_value", "mean_dense", "cov_dense", "dense_1", "dense_2", "LayerNorm", "decLayerNorm", "weight", "bias"]


def param_table(item_size, maxlen, d, H, nl, num_users, block=0, dec_layernorm=True):
    """([(state_dict name, shape)] in flat order, index of the first parameter outside the loss graph).  block > 0: the supernet's
    layout, `block` candidate layers per depth named item_encoder.layer.<depth>.<candidate>.* (stosa/super_modules.py:66-72);
    dec_layernorm: the plain model's unused decLayerNorm (stosa/models.py:176; the supernet has none).  Within an
    attention block the mean q/k/v weights (then biases), and the covariance ones, are consecutive so that each triple
    runs as one GEMM.  Parameters the reference never trains (grad None: user_margins, decLayerNorm, every decoder
    layer's dec_attention, stosa/modules.py:537-538) sit at the end, outside the optimizer's prefix."""
    hd = d // H

    def att(p):
        o = []
        for kind in ("mean", "cov"):
            o += [(p + ".%s_%s.weight" % (kind, n), (d, d)) for n in ("query", "key", "value")]
            o += [(p + ".%s_%s.bias" % (kind, n), (d,)) for n in ("query", "key", "value")]
        for n in ("mean_dense", "cov_dense"):
            o += [(p + "." + n + ".weight", (d, d)), (p + "." + n + ".bias", (d,))]
        return o + [(p + ".LayerNorm.weight", (d,)), (p + ".LayerNorm.bias", (d,))]

    def inter(p):
        return [(p + ".dense_1.weight", (4 * d, d)), (p + ".dense_1.bias", (4 * d,)), (p + ".dense_2.weight", (d, 4 * d)), (p + ".dense_2.bias", (d,)),
                (p + ".LayerNorm.weight", (d,)), (p + ".LayerNorm.bias", (d,))]

    t = [("item_mean_embeddings.weight", (item_size, d)), ("item_cov_embeddings.weight", (item_size, d)),
         ("position_mean_embeddings.weight", (maxlen, d)), ("position_cov_embeddings.weight", (maxlen, d)),
         ("LayerNorm.weight", (d,)), ("LayerNorm.bias", (d,))]
    prefixes = lambda kind, i: ["%s.layer.%d" % (kind, i)] if block == 0 else ["%s.layer.%d.%d" % (kind, i, c) for c in range(block)]
    for i in range(nl):
        for p in prefixes("item_encoder", i):
            t += att(p + ".attention") + inter(p + ".mean_intermediate") + inter(p + ".cov_intermediate")
            t += [(p + ".mean_independence_layer.weight", (H, hd)), (p + ".mean_independence_layer.bias", (H,)),
                  (p + ".cov_independence_layer.weight", (H, hd)), (p + ".cov_independence_layer.bias", (H,))]
    for i in range(nl):
        for p in prefixes("item_decoder", i):
            t += att(p + ".enc_attention") + inter(p + ".mean_intermediate") + inter(p + ".cov_intermediate")
    n_trained = len(t)
    t += [("user_margins.weight", (num_users, 1))]
    if dec_layernorm:
        t += [("decLayerNorm.weight", (d,)), ("decLayerNorm.bias", (d,))]
    for i in range(nl):
        for p in prefixes("item_decoder", i):
            t += att(p + ".dec_attention")
    return t, n_trained


def padded_tables(item_size, maxlen, d, H, nl, num_users, dec_layernorm=True, block=0):
    """(ref_table, padded table, prefix, n_trained as param_table's) of a width the kernels do not tile (wide.padded_layout): every d becomes
    d_pad (channel h * hd + j at h * hd_pad + j), the head classifiers' (H, hd) become (H, hd_pad), and the 4d of the intermediates becomes
    4 * d_pad with the 4d live channels as a zero-tailed PREFIX (element j stays at j; wide.lane_index's `prefix`): ELU(0) = 0, so the tail
    of the inner activation is zero, and (4 d_pad, d_pad) / (d_pad, 4 d_pad) are the shapes the dense arms run at width d_pad today.
    block > 0: the supernet's tables (param_table's `block`) under the same rules.  Pure arithmetic: no GPU, no library."""
    hd, hd_pad, dp = padded_layout(d, H)
    ref, n_trained = param_table(item_size, maxlen, d, H, nl, num_users, block, dec_layernorm)
    pad, prefix = [], set()
    for name, shape in ref:
        if name.endswith("_independence_layer.weight"):
            q = (H, hd_pad)
        elif name.endswith(".dense_1.weight"):
            q = (4 * dp, dp)
            prefix.add((name, 0))
        elif name.endswith(".dense_1.bias"):
            q = (4 * dp,)
            prefix.add((name, 0))
        elif name.endswith(".dense_2.weight"):
            q = (dp, 4 * dp)
            prefix.add((name, 1))
        elif name == "user_margins.weight" or name.endswith("_independence_layer.bias"):
            q = shape
        elif "_embeddings." in name:
            q = (shape[0], dp)          # (item_size | maxlen, d)
        else:
            assert all(n == d for n in shape), (name, shape)
            q = (dp,) * len(shape)      # (d, d) projections, (d,) biases and LayerNorm vectors
        pad.append((name, q))
    return ref, pad, prefix, n_trained


class DisenDistSAModel(DistRankMixin, FlatModule):
    def __init__(self, args, block=0, dec_layernorm=True, allow_kl_lanes=False, allow_wide_heads=False, allow_block_lanes=False):
        """allow_kl_lanes: take distance_metric='kl' at a padded width; without it that pair raises, as it always has.
        allow_wide_heads: take a head that pads to 128 lanes (128 / 1, 256 / 2, 100 / 1, 200 / 2); without it such a
        width raises, as it always has.  allow_block_lanes: the supernet's layout (block > 0) at a padded width or with heads of 128 lanes
        (DisenDistSASupernet(allow_lanes=True)); without it that pair raises, as it always has."""
        super().__init__()
        self.args = args
        self.item_size, self.maxlen, self.hidden_units = args.item_size, args.maxlen, args.hidden_units
        self.num_heads, self.num_layers = args.num_heads, args.num_layers
        self.dropout, self.attention_dropout = _lib.dropout_rate(args.dropout, "dropout"), _lib.dropout_rate(args.attention_dropout, "attention_dropout")
        self.prec = {"f32": ops.PREC_F32, "fp32": ops.PREC_F32, "bf16": ops.PREC_BF16}[getattr(args, "precision", "bf16")]
        d, H = self.hidden_units, self.num_heads
        tiled = d >= 64 and d % 64 == 0 and d % H == 0 and (d // H) in (16, 32, 64)      # the widths this model has always taken, as they are
        if tiled:
            self.hd, self.hd_pad, self.dp = d // H, d // H, d
        else:
            try:
                self.hd, self.hd_pad, self.dp = padded_layout(d, H)
            except _lib.AdtError as e:
                raise _lib.AdtError("DisenDistSAModel (adt_amd): %s" % e) from None
            if self.hd_pad > 128:
                raise _lib.AdtError("DisenDistSAModel (adt_amd): d=%d H=%d has head size %d, which pads to %d lanes; the distance attention is "
                                    "built for head sizes up to 128 (at 256 lanes its backward fits neither the LDS nor the register file)"
                                    % (d, H, self.hd, self.hd_pad))
            if self.hd_pad > 64 and not allow_wide_heads:
                raise _lib.AdtError("DisenDistSAModel (adt_amd): d=%d H=%d has head size %d, which pads to %d lanes; the distance attention is "
                                    "built for head sizes up to 64, and head size 128 is opt-in: pass allow_wide_heads=True to DisenDistSAModel "
                                    "(stosa/main.py does)" % (d, H, self.hd, self.hd_pad))
            if block and not allow_block_lanes:
                raise _lib.AdtError("DisenDistSASupernet (adt_amd): the supernet is built for hidden_units a multiple of 64 with head size "
                                    "16/32/64 only (padded widths run on DisenDistSAModel), got d=%d H=%d" % (d, H))
        # dp == d: the kernels tile the width as it is.  Otherwise activations and parameters are padded to dp columns (head h at
        # [h * hd_pad, h * hd_pad + hd), zero pad lanes; DESIGN.md sections 11 and 26); LayerNorm, the score scale, the dropout indices, the
        # ELU + 1 of the covariances and the distances keep the true width.  hidden_units stays the true d; dp is the row the kernels see.
        self.lanes = (H, self.hd, self.hd_pad) if self.dp != d else None
        self.distance_metric = getattr(args, "distance_metric", "wasserstein")
        if self.distance_metric not in ("wasserstein", "kl"):
            raise _lib.AdtError("DisenDistSAModel (adt_amd): distance_metric must be 'wasserstein' or 'kl', got %r" % (self.distance_metric,))
        kl = self.distance_metric == "kl"
        if kl and self.lanes is not None and not allow_kl_lanes:
            raise _lib.AdtError("DisenDistSAModel (adt_amd): distance_metric='kl' at a padded width (d=%d H=%d runs as d_pad=%d) is opt-in: "
                                "its kernels form 1 / cov and log-determinants, which the lane-aware KL kernels keep off the zero pad lanes; "
                                "pass allow_kl_lanes=True to DisenDistSAModel (stosa/main.py does), or use 'wasserstein' or a hidden_units that "
                                "is a multiple of 64 with head size 16/32/64" % (d, H, self.dp))
        # attention, BPR loss and full-sort score of the chosen metric (stosa/modules.py:244-248, trainer.py:372-379, :597-600)
        self._attn_fwd, self._attn_bwd = (ops.klattn_fwd, ops.klattn_bwd) if kl else (ops.wattn_fwd, ops.wattn_bwd)
        # past the length the whole-(b, h) kernels hold in LDS (256; 141 at head size 64): the streamed kernels, up to 1024 (adt_wattn_long.cuh)
        if not 1 <= int(args.maxlen) <= MAXLEN_MAX:
            raise _lib.AdtError("DisenDistSAModel (adt_amd): maxlen must be in 1..%d, got %r" % (MAXLEN_MAX, args.maxlen))
        self._long_attn = self.maxlen > ops.wattn_max_len(self.hd_pad)
        if self._long_attn:
            self._attn_fwd, self._attn_bwd = (ops.klattn_long_fwd, ops.klattn_long_bwd) if kl else (ops.wattn_long_fwd, ops.wattn_long_bwd)
        # head size 128 (allow_wide_heads): its own streamed family at every maxlen, scale and live lanes always given
        wide_heads = self.hd_pad == 128
        if wide_heads:
            self._set_scaled_attn(*((ops.klattn_hd128_fwd, ops.klattn_hd128_bwd) if kl else (ops.wattn_hd128_fwd, ops.wattn_hd128_bwd)))
        self._dist_bpr, self._dist_full = (ops.kldist_bpr, ops.kldist_full) if kl else (ops.wdist_bpr, ops.wdist_full)
        if self.lanes is None:
            table, n_trained = param_table(args.item_size, args.maxlen, d, H, args.num_layers, args.num_users, block, dec_layernorm)
            self._build_flat(table, getattr(args, "device", "cuda:0"), REF_ORDER)
            ref_table = self.table
        else:
            ln = self.lanes
            if not wide_heads:
                if kl:
                    fwd, bwd = (ops.klattn_long_scaled_fwd, ops.klattn_long_scaled_bwd) if self._long_attn else (ops.klattn_scaled_fwd, ops.klattn_scaled_bwd)
                else:
                    fwd, bwd = (ops.wattn_long_scaled_fwd, ops.wattn_long_scaled_bwd) if self._long_attn else (ops.wattn_scaled_fwd, ops.wattn_scaled_bwd)
                self._set_scaled_attn(fwd, bwd)
            dist_bpr, dist_full = (ops.kldist_bpr_lanes, ops.kldist_full_lanes) if kl else (ops.wdist_bpr_lanes, ops.wdist_full_lanes)
            self._dist_bpr = lambda *a: dist_bpr(*a, ln)
            self._dist_full = lambda *a: dist_full(*a, ln)
            ref_table, table, prefix, n_trained = padded_tables(args.item_size, args.maxlen, d, H, args.num_layers, args.num_users, dec_layernorm, block)
            self._build_flat(table, getattr(args, "device", "cuda:0"), REF_ORDER, ref_table=ref_table, width=(d, H), prefix=prefix)
        self.n_trained_floats = self._views[table[n_trained][0]][0]     # optimizer prefix (flat floats)
        # init_weights (stosa/models.py:262-272): N(0.01, initializer_range) on Linear/Embedding weights, LayerNorm 1/0, biases 0
        g = torch.Generator(device="cpu").manual_seed(torch.initial_seed() % (1 << 31))
        std = float(getattr(args, "initializer_range", 0.02))
        for name, shape in ref_table:
            v = self.R(name)         # reference shape (a view of the flat buffer itself without padding)
            if "LayerNorm.weight" in name:
                v.fill_(1.0)
            elif name.endswith(".weight"):
                v.copy_(0.01 + std * torch.randn(shape, generator=g))
        self.push()

    def _set_scaled_attn(self, fwd, bwd):
        """The attention through entry points that take (scale, hd_live): the score scale of the TRUE head size, for both directions."""
        scaled = (1.0 / math.sqrt(self.hd), self.hd)
        self._attn_fwd = lambda Qm, Qc, Km, Kc, Vm, Vc, kid, B, H, L, *a, **k: fwd(Qm, Qc, Km, Kc, Vm, Vc, kid, B, H, L, *scaled, *a, **k)
        self._attn_bwd = lambda Qm, Qc, Km, Kc, Vm, Vc, kid, Om, Oc, LSE, dOm, dOc, B, H, L, *a, **k: \
            bwd(Qm, Qc, Km, Kc, Vm, Vc, kid, Om, Oc, LSE, dOm, dOc, B, H, L, *scaled, *a, **k)

    # ------------------------------------------------------------------------------------------------------------------
    def _embed(self, tp, ids, which, site):
        """add_position_mean_embedding / add_position_cov_embedding (stosa/models.py:183-210)."""
        P, G = self.P, self.G
        L = self.maxlen
        en, pn = "item_%s_embeddings.weight" % which, "position_%s_embeddings.weight" % which
        x0 = Act(ops.embed_sum_fwd(ids, P(en), P(pn), L))

        def bw():   # runs after the LayerNorm / dropout closures registered below
            if x0.g is None:
                return
            T, d = x0.g.shape
            _lib.check(self.lib.adt_item_scatter(ops._p(ids), ops._p(x0.g), d, None, T, d, 1.0, 0.0, None, 0, 0, ops._p(G(en)), 1, 0, ops._stream()),
                       "item_scatter")   # padding_idx = 0: rows of id 0 are skipped
            _lib.check(self.lib.adt_posemb_bwd(ops._p(self._ones(T)), ops._p(x0.g), T, L, d, 0.0, None, 0, 0, ops._p(G(pn)), ops._stream()), "posemb_bwd")
        tp.bw.append(bw)
        z = tp.layernorm(x0, P("LayerNorm.weight"), P("LayerNorm.bias"), G("LayerNorm.weight"), G("LayerNorm.bias"), LN_EPS)
        return tp.dropact(z, self.dropout, site, ops.ACT_ELU1 if which == "cov" else ops.ACT_ELU)

    def _ones(self, T):
        if getattr(self, "_ones_buf", None) is None or self._ones_buf.numel() < T:
            self._ones_buf = torch.ones(T, device=self.dev, dtype=torch.int32)
        return self._ones_buf

    def _attention(self, tp, p, mq, cq, mkv, ckv, key_ids, B, st):
        """DistAttention.forward / DistEDAttention.forward (stosa/modules.py:222-275, 311-361) -> (mean_hidden, cov_hidden,
        mean context, cov context)."""
        P, G, sp = self.P, self.G, self.span
        d, H, L = self.dp, self.num_heads, self.maxlen
        pa = tp.p_eff(self.attention_dropout)

        def proj(x, kind, first, last, n, act):
            w0, w1 = p + ".%s_%s.weight" % (kind, first), p + ".%s_%s.weight" % (kind, last)
            b0, b1 = p + ".%s_%s.bias" % (kind, first), p + ".%s_%s.bias" % (kind, last)
            if act != ops.ACT_NONE and tp.lanes is not None:
                # padded widths: ELU(0) + 1 = 1 on a pad lane would feed the next layer's pad weight columns a gradient; the projection
                # runs without its epilogue and one lane pass applies the activation to the live lanes (no dense instantiation changes)
                y = tp.dense(x, sp(w0, w1, (n * d, d)), sp(b0, b1, (n * d,)), sp(w0, w1, (n * d, d), grad=True), sp(b0, b1, (n * d,), grad=True))
                return tp.act_lanes(y, act)
            return tp.dense(x, sp(w0, w1, (n * d, d)), sp(b0, b1, (n * d,)), sp(w0, w1, (n * d, d), grad=True), sp(b0, b1, (n * d,), grad=True), act=act)
        if mq is mkv:
            pm, pc = proj(mq, "mean", "query", "value", 3, ops.ACT_NONE), proj(cq, "cov", "query", "value", 3, ops.ACT_ELU1)
            Qm, Km, Vm = pm.t[:, :d], pm.t[:, d:2 * d], pm.t[:, 2 * d:]
            Qc, Kc, Vc = pc.t[:, :d], pc.t[:, d:2 * d], pc.t[:, 2 * d:]
            holders = ((pm,), (pc,))
        else:
            qm, qc = proj(mq, "mean", "query", "query", 1, ops.ACT_NONE), proj(cq, "cov", "query", "query", 1, ops.ACT_ELU1)
            km, kc = proj(mkv, "mean", "key", "value", 2, ops.ACT_NONE), proj(ckv, "cov", "key", "value", 2, ops.ACT_ELU1)
            Qm, Km, Vm = qm.t, km.t[:, :d], km.t[:, d:]
            Qc, Kc, Vc = qc.t, kc.t[:, :d], kc.t[:, d:]
            holders = ((qm, km), (qc, kc))
        Om, Oc, LSE = self._attn_fwd(Qm, Qc, Km, Kc, Vm, Vc, key_ids, B, H, L, pa, self._seed, st["attn"], tp.b_offset, prec=self.prec)
        om, oc = Act(Om), Act(Oc)

        def bw():
            if om.g is None and oc.g is None:
                return
            T = Om.shape[0]
            gom = om.g if om.g is not None else torch.zeros_like(Om)
            goc = oc.g if oc.g is not None else torch.zeros_like(Oc)
            gm = torch.empty(T, 3 * d, device=self.dev, dtype=torch.float32)
            gc = torch.empty(T, 3 * d, device=self.dev, dtype=torch.float32)
            self._attn_bwd(Qm, Qc, Km, Kc, Vm, Vc, key_ids, Om, Oc, LSE, gom, goc, B, H, L, pa, self._seed, st["attn"], tp.b_offset,
                          out=(gm[:, :d], gc[:, :d], gm[:, d:2 * d], gc[:, d:2 * d], gm[:, 2 * d:], gc[:, 2 * d:]), prec=self.prec)
            for hold, g in ((holders[0], gm), (holders[1], gc)):
                if len(hold) == 1:
                    hold[0].g = g
                else:
                    hold[0].g, hold[1].g = g[:, :d], g[:, d:]
        tp.bw.append(bw)
        lw, lb, glw, glb = P(p + ".LayerNorm.weight"), P(p + ".LayerNorm.bias"), G(p + ".LayerNorm.weight"), G(p + ".LayerNorm.bias")
        zm = tp.dense(om, P(p + ".mean_dense.weight"), P(p + ".mean_dense.bias"), G(p + ".mean_dense.weight"), G(p + ".mean_dense.bias"),
                      p=self.dropout, site=st["out_mean"], R=mq)
        hm = tp.layernorm(zm, lw, lb, glw, glb, LN_EPS)
        zc = tp.dense(oc, P(p + ".cov_dense.weight"), P(p + ".cov_dense.bias"), G(p + ".cov_dense.weight"), G(p + ".cov_dense.bias"),
                      p=self.dropout, site=st["out_cov"], R=cq)
        hc = tp.layernorm(zc, lw, lb, glw, glb, LN_EPS)
        return hm, hc, om, oc

    def _intermediate(self, tp, p, x, site, elu1):
        """DistIntermediate.forward (stosa/modules.py:485-494); elu1: the covariance branch's ELU(.)+1 (:522,540)."""
        P, G = self.P, self.G
        h = tp.dense(x, P(p + ".dense_1.weight"), P(p + ".dense_1.bias"), G(p + ".dense_1.weight"), G(p + ".dense_1.bias"), act=ops.ACT_ELU)
        z = tp.dense(h, P(p + ".dense_2.weight"), P(p + ".dense_2.bias"), G(p + ".dense_2.weight"), G(p + ".dense_2.bias"), p=self.dropout, site=site, R=x)
        y = tp.layernorm(z, P(p + ".LayerNorm.weight"), P(p + ".LayerNorm.bias"), G(p + ".LayerNorm.weight"), G(p + ".LayerNorm.bias"), LN_EPS)
        return tp.dropact(y, 0.0, 0, ops.ACT_ELU1) if elu1 else y

    def _enc_layer(self, tp, p, m, c, inp, B, st):
        """DistLayer.forward (stosa/modules.py:518-525) -> (mean, cov, mean / cov head-classifier log-probabilities)."""
        P, G = self.P, self.G
        hm, hc, om, oc = self._attention(tp, p + ".attention", m, c, m, c, inp, B, st)
        rm = tp.headcls(om, P(p + ".mean_independence_layer.weight"), P(p + ".mean_independence_layer.bias"),
                        G(p + ".mean_independence_layer.weight"), G(p + ".mean_independence_layer.bias"))
        rc = tp.headcls(oc, P(p + ".cov_independence_layer.weight"), P(p + ".cov_independence_layer.bias"),
                        G(p + ".cov_independence_layer.weight"), G(p + ".cov_independence_layer.bias"))
        m2 = self._intermediate(tp, p + ".mean_intermediate", hm, st["ffn_mean"], False)
        c2 = self._intermediate(tp, p + ".cov_intermediate", hc, st["ffn_cov"], True)
        return m2, c2, rm, rc

    def _dec_layer(self, tp, p, dm, dc, m, c, inp, B, st):
        """DistDecLayer.forward (modules.py:535-541): dec_attention's output is discarded by the reference, so it is not computed;
        enc_attention takes queries from the decoder input and keys / values (and the mask) from the encoder side."""
        hm, hc, _, _ = self._attention(tp, p + ".enc_attention", dm, dc, m, c, inp, B, st)
        return (self._intermediate(tp, p + ".mean_intermediate", hm, st["ffn_mean"], False),
                self._intermediate(tp, p + ".cov_intermediate", hc, st["ffn_cov"], True))

    def _finetune(self, tp, inp, dec, B):
        """Token-major body of finetune (stosa/models.py:212-260)."""
        P, G = self.P, self.G
        m, c = self._embed(tp, inp, "mean", SITE_EMB["seq_mean"]), self._embed(tp, inp, "cov", SITE_EMB["seq_cov"])
        dm, dc = self._embed(tp, dec, "mean", SITE_EMB["dec_mean"]), self._embed(tp, dec, "cov", SITE_EMB["dec_cov"])
        enc_inputs, enc_recs, dec_outs = [], [], []
        for i in range(self.num_layers):
            enc_inputs.append((m, c))
            m, c, rm, rc = self._enc_layer(tp, "item_encoder.layer.%d" % i, m, c, inp, B, enc_sites(i))
            enc_recs.append((rm, rc))
        tp.mark_decoder_start()
        for i in range(self.num_layers):
            dm, dc = self._dec_layer(tp, "item_decoder.layer.%d" % i, dm, dc, m, c, inp, B, dec_sites(i))
            dec_outs.append((dm, dc))
        return m, c, enc_inputs, enc_recs, dec_outs

    def finetune(self, input_ids, dec_ids, user_ids=None):
        """stosa/models.py:212-260 -> (mean_out, cov_out, att_scores=None, margins, enc_inputs, enc_recs, dec_outputs).  The
        (B, H, L, L) attention probabilities are never materialised (no caller reads them: trainer.py:534,585).  Under autograd the
        tensors are wired into it (adt_amd::model_forward) and `item_mean_embeddings` / `item_cov_embeddings` / `user_margins` are
        callable like the reference's nn.Embedding modules, so the reference's loop body (stosa/trainer.py:534-559 with
        bpr_optimization :358-391) runs unchanged; FusedStosaTrainer.step is the fast way to train."""
        ids = [self.ids(input_ids), self.ids(dec_ids)]
        B, L = ids[0].shape
        if self.lanes is not None and custom_ops.wants_grad(self):
            raise _lib.AdtError("DisenDistSAModel (adt_amd): autograd through finetune() (the reference's loop body) is not built for padded "
                                "widths (d=%d H=%d runs as d_pad=%d); train with FusedStosaTrainer (the fused loop) or call finetune() under "
                                "torch.no_grad()" % (self.hidden_units, self.num_heads, self.dp))
        if custom_ops.wants_grad(self):
            outs = custom_ops.forward_with_grad(self, ids)
        else:
            with torch.no_grad():
                outs, _ = self._op_forward(ids, self.training)
        nl = self.num_layers
        margins = None if user_ids is None else self.user_margins(user_ids)
        pairs = [[outs[2 + 2 * i], outs[3 + 2 * i]] for i in range(3 * nl)]
        return outs[0], outs[1], None, margins, pairs[:nl], pairs[nl:2 * nl], pairs[2 * nl:]

    def _op_forward(self, ids, training):
        inp, dec = ids
        B, L = inp.shape
        d, H = self.hidden_units, self.num_heads
        if training:
            self.next_seed()
        self.push()      # padded widths: the reference-shaped parameters are the truth between steps (no-op otherwise)
        tp = Tape(self, self.prec, training)
        m, c, enc_inputs, enc_recs, dec_outs = self._finetune(tp, inp.view(-1), dec.view(-1), B)
        acts = [m, c] + [x for pr in enc_inputs for x in pr] + [x for pr in enc_recs for x in pr] + [x for pr in dec_outs for x in pr]
        nl = self.num_layers
        outs = []
        for k, a in enumerate(acts):
            is_rec = 2 + 2 * nl <= k < 2 + 4 * nl
            outs.append(a.t.view(B, L, H, H) if is_rec else self._live(a.t, B, L))
        return outs, {"tp": tp, "acts": acts}

    def _live(self, t, B, L):
        """(B * L, dp) activation as the reference's (B, L, d): the live lanes of a padded width (a copy, outside the training step)."""
        if self.lanes is None:
            return t.view(B, L, self.dp)
        return t.view(B, L, self.num_heads, self.hd_pad)[..., :self.hd].reshape(B, L, self.hidden_units)

    def _op_backward(self, st, grads):
        self.flat_grad.zero_()
        for a, g in zip(st["acts"], grads):
            give(a, custom_ops.take_grad(g, tuple(a.t.shape)))
        st["tp"].backward()
        base = self.n_trained_floats
        return custom_ops.param_grads(self, lambda n: self._views[n][0] >= base)     # the reference leaves these at grad None

    @torch.no_grad()
    def _last_state(self, input_ids, dec_ids=None):
        """(mean, covariance) (B, d) of the last position in eval mode: what every full-sort score is taken from (stosa/trainer.py:590-595)."""
        inp = self.ids(input_ids)
        dec = inp if dec_ids is None else self.ids(dec_ids)
        B, L = inp.shape
        was = self.training
        self.eval()
        self.push()
        tp = Tape(self, self.prec, False)
        m, c, _, _, _ = self._finetune(tp, inp.view(-1), dec.view(-1), B)
        rows = torch.arange(L - 1, B * L, L, device=self.dev, dtype=torch.int32)
        sm, sc = ops.gather_rows(m.t, rows), ops.gather_rows(c.t, rows)
        self.train(was)
        return sm, sc

    def _dist_tables(self):
        """The item tables for DistRankMixin (at a padded width: the padded tables, which DistRankMixin packs lane-aware).  Every row 0..item_size - 1 of the tables takes part in the reference's full sort (the
        padding row 0 only with first_id = 0), so n_items = item_size - 1."""
        return self.P("item_mean_embeddings.weight"), self.P("item_cov_embeddings.weight"), self.item_size - 1

    @torch.no_grad()
    def predict_full(self, input_ids, dec_ids=None):
        """Full-sort scores (stosa/trainer.py:583-595), (B, item_size): dist_predict_full (:464-479), the Wasserstein distance of the
        last state to every item, or kl_predict_full (:481-511), whose scores depend on the rows of this call being the eval batch."""
        sm, sc = self._last_state(input_ids, dec_ids)
        return self._dist_full(sm, sc, self.P("item_mean_embeddings.weight"), self.P("item_cov_embeddings.weight"), self.item_size)

    # ------------------------------------------------------------------------------------------------------------------
    def stage(self, input_ids, dec_ids, pos_ids, neg_ids, n_target_global=None):
        inp, dec, pos, neg = (np.ascontiguousarray(np.asarray(a), dtype=np.int32) for a in (input_ids, dec_ids, pos_ids, neg_ids))
        nt = float(max(int((pos > 0).sum()), 1) if n_target_global is None else n_target_global)
        return {"B": inp.shape[0], "inp": self.ids(inp), "dec": self.ids(dec), "pos": self.ids(pos), "neg": self.ids(neg),
                "inv_count": torch.tensor([1.0 / nt], device=self.dev, dtype=torch.float32)}

    def loss_forward_backward(self, st, lambda1, lambda2, norms, loss_slots, b_offset=0):
        """Forward, the loss assembly of DistSAModelTrainer.iteration (stosa/trainer.py:534-556) and backward into flat_grad.
        norms: device {_, n_mse, n_nll}; loss_slots: (3 + 4*num_layers) x 64 floats {bpr, pvn, auc, mse (mean, cov) per
        layer.., nll (mean, cov) per layer..}."""
        B, L, d, H, nl = st["B"], self.maxlen, self.hidden_units, self.num_heads, self.num_layers
        tp = Tape(self, self.prec, self.training, row_offset=b_offset * L, b_offset=b_offset)
        inp, dec = st["inp"].view(-1), st["dec"].view(-1)
        m, c, enc_inputs, enc_recs, dec_outs = self._finetune(tp, inp, dec, B)
        dsm, dsc = self._dist_bpr(m.t, c.t, self.P("item_mean_embeddings.weight"), self.P("item_cov_embeddings.weight"), st["pos"].view(-1),
                                 st["neg"].view(-1), float(self.args.pvn_weight), st["inv_count"], self.G("item_mean_embeddings.weight"),
                                 self.G("item_cov_embeddings.weight"), loss_slots[0:3].view(-1))
        give(m, dsm)
        give(c, dsc)
        for l in range(nl):
            for t in (0, 1):
                a, bq = enc_inputs[l][t], dec_outs[nl - 1 - l][t]      # dec_outputs.reverse() (trainer.py:540)
                if a.g is None:
                    a.g = torch.zeros_like(a.t)
                g_b = torch.empty_like(bq.t)
                ops.mse_seed(a.t, bq.t, lambda1[l], norms, a.g, True, g_b, loss_slots[3 + 2 * l + t])
                give(bq, g_b)
        for l in range(nl):
            for t in (0, 1):
                r = enc_recs[l][t]
                r.g = torch.empty_like(r.t)
                ops.nll_seed(r.t, H, lambda2[l], norms, r.g, loss_slots[3 + 2 * nl + 2 * l + t])
        tp.backward()
