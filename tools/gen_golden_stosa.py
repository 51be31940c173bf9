#!/usr/bin/env python3
"""Generate tests/golden/stosa_*.npz (and, with --metric kl, stosa_kl_*.npz) by IMPORTING the reference (read-only, /root/reference/stosa) in the build container
(run through tools/gen_golden_wide.py stosa).  Fixtures are data only: seeded inputs, the seed that regenerates the numpy
weights, and the tensors the reference produced.

The loss assembly below calls bpr_optimization's arithmetic (stosa/trainer.py:358-391, restated with the reference's own
wasserstein_distance from stosa/modules.py because the method needs a constructed Trainer with dataloaders) and the loop
body of DistSAModelTrainer.iteration (:534-559) with the same torch functions in the same order; dropout is 0.  With
metric "kl" the distances are the reference's kl_distance / kl_distance_matmul and full_dist is kl_predict_full's arithmetic
(:481-511) with the fixture batch as the eval batch; those fixtures are compacted (tools/gen_golden_inputs.py:compact) to stay
small (every float tensor above 2048 entries becomes its norm and 1024 samples), and keep no weights: after one Adam step from
zero moments they follow from the initial weights and the gradient.
"""
import os
import sys

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(REPO, "tests", "golden")


class Args:
    pass


def stosa_batch(r, B, L, V, pad_min=0):
    """Batch in the layout of stosa/datasets.py (left-padded input_ids, dec_ids shifted by one, target_pos = next item,
    target_neg sampled, 0 where padded).  Row 0 is full length; every other row has a padded prefix of at least pad_min positions."""
    inp = np.zeros((B, L), np.int64)
    dec = np.zeros((B, L), np.int64)
    pos = np.zeros((B, L), np.int64)
    neg = np.zeros((B, L), np.int64)
    for b in range(B):
        n = L if b == 0 else int(r.randint(2, L + 1 - pad_min))
        items = r.randint(1, V, size=n + 1)
        inp[b, L - n:] = items[:-1]
        pos[b, L - n:] = items[1:]
        neg[b, L - n:] = r.randint(1, V, size=n)
        dec[b, 1:] = inp[b, :-1]
    return inp, dec, pos, neg


def kl_predict_full(modules, mo, co, Em, Ec):
    """kl_predict_full (stosa/trainer.py:481-511) with Em / Ec the item tables (Ec already through ELU(.)+1)."""
    V, E = Em.shape[0], mo.shape[0]
    pad = E - V % E
    cm = torch.cat((Em, torch.zeros(pad, Em.shape[1])), 0)
    cc = torch.cat((Ec, torch.ones(pad, Em.shape[1])), 0)
    res = torch.zeros(E, cm.shape[0])
    for s0 in range(0, cm.shape[0], E):
        res[:, s0:s0 + E] = modules.kl_distance_matmul(mo, co, cm[s0:s0 + E], cc[s0:s0 + E])
    return res[:, :V]


def reference_model(cfg_kw, B, seed, metric, pad_min=0, cov_qk_bias=0.0):
    """The reference's DisenDistSAModel with the seeded weights of a fixture and that fixture's batch: (cfg, args, model, the
    reference's modules, (input_ids, dec_ids, pos_ids, neg_ids)).  cov_qk_bias is added to every cov_query / cov_key bias (main_hd128)."""
    from tools.gen_golden_wide import _import_from
    from oracle import stosa_oracle as so
    models = _import_from("/root/reference/stosa", "models")
    modules = sys.modules["modules"]
    cfg = so.Cfg(**cfg_kw)
    P = so.init_params(cfg, seed)
    r = np.random.RandomState(seed + 1)
    for k in P:   # biases away from zero so that their gradients are exercised
        if k.endswith(".bias") and "LayerNorm" not in k:
            P[k] = (0.02 * r.standard_normal(P[k].shape)).astype(np.float32)
            if k.endswith(("cov_query.bias", "cov_key.bias")):
                P[k] += np.float32(cov_qk_bias)
    batch = stosa_batch(r, B, cfg.maxlen, cfg.item_size, pad_min)
    a = Args()
    a.item_size, a.hidden_units, a.maxlen, a.num_users, a.dropout, a.attention_dropout = cfg.item_size, cfg.hidden_units, cfg.maxlen, cfg.num_users, 0.0, 0.0
    a.num_heads, a.num_layers, a.hidden_act, a.initializer_range, a.distance_metric, a.kernel_param = cfg.num_heads, cfg.num_layers, "gelu", 0.02, metric, 1.0
    a.cuda_condition, a.pvn_weight = False, cfg.pvn_weight
    m = models.DisenDistSAModel(a)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in P.items()}, strict=True)
    return cfg, a, m, modules, batch


def gen_stosa(tag, cfg_kw, B, seed, lam1, lam2, lr=1e-3, keep_w3=True, compact=False, steps=3, metric="wasserstein", keep_w1=True, thresh=8192,
              pad_min=0, nsample=1024, cov_qk_bias=0.0):
    cfg, a, m, modules, (inp, dec, pos, neg) = reference_model(cfg_kw, B, seed, metric, pad_min, cov_qk_bias)
    t = [torch.from_numpy(x) for x in (inp, dec, pos, neg)]
    uid = torch.zeros(B, dtype=torch.long)
    out = {"seed": seed, "input_ids": inp, "dec_ids": dec, "pos_ids": pos, "neg_ids": neg, "lambda1": np.array(lam1), "lambda2": np.array(lam2),
           "lr": lr, "cfg": np.array([cfg.item_size, cfg.maxlen, cfg.hidden_units, cfg.num_heads, cfg.num_layers, cfg.num_users]),
           "pvn_weight": cfg.pvn_weight}
    if cov_qk_bias:
        out["cov_qk_bias"] = cov_qk_bias
    m.eval()
    with torch.no_grad():
        mo, co, att, margins, enc_in, enc_rec, dec_out = m.finetune(t[0], t[1], uid)
        out["mean_out"], out["cov_out"] = mo.numpy(), co.numpy()
        for i in range(cfg.num_layers):
            out["enc_in_mean_%d" % i], out["enc_in_cov_%d" % i] = enc_in[i][0].numpy(), enc_in[i][1].numpy()
            out["rec_mean_%d" % i], out["rec_cov_%d" % i] = enc_rec[i][0].numpy(), enc_rec[i][1].numpy()
            out["dec_out_mean_%d" % i], out["dec_out_cov_%d" % i] = dec_out[i][0].numpy(), dec_out[i][1].numpy()
        # dist_predict_full (trainer.py:464-479) on the last position
        elu = nn.ELU()
        if metric == "kl":
            out["full_dist"] = kl_predict_full(modules, mo[:, -1, :], co[:, -1, :], m.item_mean_embeddings.weight,
                                               elu(m.item_cov_embeddings.weight) + 1).numpy()
        else:
            out["full_dist"] = modules.wasserstein_distance_matmul(mo[:, -1, :], co[:, -1, :], m.item_mean_embeddings.weight,
                                                                   elu(m.item_cov_embeddings.weight) + 1).numpy()
    m.train()
    opt = torch.optim.Adam(m.parameters(), lr=lr, betas=(0.9, 0.999), weight_decay=0.0)
    wd = modules.kl_distance if metric == "kl" else modules.wasserstein_distance
    for step in range(steps):
        mo, co, att, margins, enc_in, enc_rec, dec_out = m.finetune(t[0], t[1], uid)
        # bpr_optimization (trainer.py:358-391)
        act = nn.ELU()
        pos_mean, neg_mean = m.item_mean_embeddings(t[2]), m.item_mean_embeddings(t[3])
        pos_cov, neg_cov = act(m.item_cov_embeddings(t[2])) + 1, act(m.item_cov_embeddings(t[3])) + 1
        d = cfg.hidden_units
        pos_mean, pos_cov, neg_mean, neg_cov = (x.view(-1, d) for x in (pos_mean, pos_cov, neg_mean, neg_cov))
        sm, sc = mo.view(-1, d), co.view(-1, d)
        pos_logits, neg_logits, pos_vs_neg = wd(sm, sc, pos_mean, pos_cov), wd(sm, sc, neg_mean, neg_cov), wd(pos_mean, pos_cov, neg_mean, neg_cov)
        istarget = (t[2] > 0).view(-1).float()
        loss = torch.sum(-torch.log(torch.sigmoid(neg_logits - pos_logits + 1e-24)) * istarget) / torch.sum(istarget)
        pvn_loss = a.pvn_weight * torch.sum(torch.clamp(pos_logits - pos_vs_neg, 0) * istarget) / torch.sum(istarget)
        auc = torch.sum(((torch.sign(neg_logits - pos_logits) + 1) / 2) * istarget) / torch.sum(istarget)
        if step == 0:
            out["bpr"], out["pvn"], out["auc"] = float(loss), float(pvn_loss), float(auc)
        # iteration (trainer.py:540-559)
        dec_out.reverse()
        for l in range(cfg.num_layers):
            loss = loss + lam1[l] * F.mse_loss(enc_in[l][0], dec_out[l][0])
            loss = loss + lam1[l] * F.mse_loss(enc_in[l][1], dec_out[l][1])
        bs = enc_rec[0][0].shape[0]
        label = torch.tile(torch.arange(a.num_heads), [bs * a.maxlen, 1])
        for l in range(cfg.num_layers):
            loss = loss + lam2[l] * F.nll_loss(enc_rec[l][0].view(bs * a.maxlen, a.num_heads, a.num_heads), label)
            loss = loss + lam2[l] * F.nll_loss(enc_rec[l][1].view(bs * a.maxlen, a.num_heads, a.num_heads), label)
        loss = loss + pvn_loss
        opt.zero_grad()
        loss.backward()
        if step == 0:
            out["loss"] = float(loss.item())
            none = []
            for k, p in m.named_parameters():
                if p.grad is None:
                    none.append(k)
                else:
                    out["grad." + k] = p.grad.numpy().copy()
            out["grad_none"] = np.array(none)
        opt.step()
        if (step == 0 and keep_w1) or (step == 2 and keep_w3):
            for k, p in m.named_parameters():
                out["w%d." % (step + 1) + k] = p.detach().numpy().copy()
    path = os.path.join(OUT, ("stosa_kl_%s.npz" if metric == "kl" else "stosa_%s.npz") % tag)
    if compact:
        from tools.gen_golden_inputs import compact as _compact
        out = _compact(out, k=nsample, thresh=thresh)
    np.savez_compressed(path, **out)
    print("wrote", path, "loss", out["loss"], "none-grads", len(out["grad_none"]), "%.1f KB" % (os.path.getsize(path) / 1024))


def main(metric="wasserstein"):
    if metric == "kl":
        return main_kl()
    gen_stosa("small", dict(item_size=42, maxlen=12, hidden_units=64, num_heads=4, num_layers=1, num_users=4, pvn_weight=0.005), B=4, seed=21,
              lam1=[0.3], lam2=[0.2])
    gen_stosa("l2h2", dict(item_size=33, maxlen=20, hidden_units=64, num_heads=2, num_layers=2, num_users=3, pvn_weight=0.1), B=3, seed=22,
              lam1=[0.25, 0.1], lam2=[0.15, 0.05], keep_w3=False)
    gen_stosa("h1", dict(item_size=28, maxlen=9, hidden_units=64, num_heads=1, num_layers=1, num_users=2, pvn_weight=0.05), B=2, seed=23,
              lam1=[0.1], lam2=[0.05], keep_w3=False)


def main_cfg5():
    """BASELINE configs[4]: STOSA-ADT at the Amazon-Beauty template shape (stosa/templates/Beauty.json: d=64, H=4, 1 layer, L=100,
    pvn_weight 0.005; stosa/data/Beauty.txt has 12,101 items => item_size 12,103; 22,363 users), B=8; get_lambdas("Beauty")[:1]."""
    gen_stosa("cfg5_beauty", dict(item_size=12103, maxlen=100, hidden_units=64, num_heads=4, num_layers=1, num_users=22363, pvn_weight=0.005), B=8,
              seed=33, lam1=[0.0021], lam2=[0.0009], keep_w3=False, compact=True, steps=1)


def main_kl():
    """The four shapes of the Wasserstein fixtures with distance_metric='kl' (compacted)."""
    kw = dict(metric="kl", keep_w3=False, keep_w1=False, compact=True, steps=1, thresh=2048)
    gen_stosa("small", dict(item_size=42, maxlen=12, hidden_units=64, num_heads=4, num_layers=1, num_users=4, pvn_weight=0.005), B=4, seed=21,
              lam1=[0.3], lam2=[0.2], **kw)
    gen_stosa("l2h2", dict(item_size=33, maxlen=20, hidden_units=64, num_heads=2, num_layers=2, num_users=3, pvn_weight=0.1), B=3, seed=22,
              lam1=[0.25, 0.1], lam2=[0.15, 0.05], **kw)
    gen_stosa("h1", dict(item_size=28, maxlen=9, hidden_units=64, num_heads=1, num_layers=1, num_users=2, pvn_weight=0.05), B=2, seed=23,
              lam1=[0.1], lam2=[0.05], **kw)
    gen_stosa("cfg5_beauty", dict(item_size=12103, maxlen=100, hidden_units=64, num_heads=4, num_layers=1, num_users=22363, pvn_weight=0.005), B=8,
              seed=33, lam1=[0.0021], lam2=[0.0009], **kw)


def main_long():
    """stosa_l272.npz and stosa_kl_l272.npz: past the length the whole-(b, h) attention kernels hold in LDS (256; 141 at head size 64), at
    the head size of the Home / Office / Toys templates (d 64, one head).  Row 0 is full length, row 1 has a padded prefix of at least 40
    positions (queries without an attendable key over several 16-row tiles); compacted like the KL fixtures."""
    cfg_kw = dict(item_size=40, maxlen=272, hidden_units=64, num_heads=1, num_layers=1, num_users=2, pvn_weight=0.05)
    kw = dict(keep_w3=False, keep_w1=False, compact=True, steps=1, thresh=2048, pad_min=40)
    for metric in ("wasserstein", "kl"):
        gen_stosa("l272", cfg_kw, B=2, seed=27, lam1=[0.1], lam2=[0.05], metric=metric, **kw)


STOSA_ODD_COMPACT = 320      # samples per compacted tensor of the odd-width fixtures (tests/test_stosa_oddwidth_*.py: K)


def main_odd():
    """stosa_w50_h1 / w100_h2 / w48_h4 / w150_h3.npz: hidden widths the kernels pad (head size 50 -> 64 lanes, 2 x 50 -> 128, 4 x 12 -> 4 x 16,
    3 x 50 -> 192) at the small shapes of main(): dropout 0, three Adam steps, every gen_stosa field.  Compacted
    (every float tensor above 2048 entries: its norm and 320 samples) so that each file stays far below 1 MiB."""
    kw = dict(compact=True, thresh=2048, nsample=STOSA_ODD_COMPACT)
    gen_stosa("w50_h1", dict(item_size=42, maxlen=12, hidden_units=50, num_heads=1, num_layers=1, num_users=4, pvn_weight=0.005), B=4, seed=41,
              lam1=[0.3], lam2=[0.2], **kw)
    gen_stosa("w100_h2", dict(item_size=33, maxlen=20, hidden_units=100, num_heads=2, num_layers=2, num_users=3, pvn_weight=0.1), B=3, seed=42,
              lam1=[0.25, 0.1], lam2=[0.15, 0.05], **kw)
    gen_stosa("w48_h4", dict(item_size=28, maxlen=9, hidden_units=48, num_heads=4, num_layers=1, num_users=2, pvn_weight=0.05), B=3, seed=43,
              lam1=[0.1], lam2=[0.05], **kw)
    gen_stosa("w150_h3", dict(item_size=42, maxlen=12, hidden_units=150, num_heads=3, num_layers=1, num_users=4, pvn_weight=0.005), B=3, seed=44,
              lam1=[0.3], lam2=[0.2], **kw)


def main_kl_odd():
    """stosa_kl_w50_h1 / w100_h2 / w48_h4.npz: main_odd()'s configurations, batch sizes, seeds and lambdas under distance_metric='kl'
    (DESIGN.md section 27), compacted the same way."""
    kw = dict(compact=True, thresh=2048, nsample=STOSA_ODD_COMPACT, metric="kl")
    gen_stosa("w50_h1", dict(item_size=42, maxlen=12, hidden_units=50, num_heads=1, num_layers=1, num_users=4, pvn_weight=0.005), B=4, seed=41,
              lam1=[0.3], lam2=[0.2], **kw)
    gen_stosa("w100_h2", dict(item_size=33, maxlen=20, hidden_units=100, num_heads=2, num_layers=2, num_users=3, pvn_weight=0.1), B=3, seed=42,
              lam1=[0.25, 0.1], lam2=[0.15, 0.05], **kw)
    gen_stosa("w48_h4", dict(item_size=28, maxlen=9, hidden_units=48, num_heads=4, num_layers=1, num_users=2, pvn_weight=0.05), B=3, seed=43,
              lam1=[0.1], lam2=[0.05], **kw)


def main_hd128():
    """stosa_hd128 / stosa_kl_hd128 (d 128, one head), stosa_w100_h1 / stosa_kl_w100_h1 (d 100, one head: 128 lanes) and stosa_hd128_h2.npz
    (d 256, two heads, two layers: the head classifier at 128 lanes and the head offset): head size 128, compacted
    like main_odd().  The weights after the first step are left out, as in main_kl(): they follow from the initial weights and the
    gradient; stosa_hd128_h2 keeps no weights at all (main()'s l2h2 keeps none after step 3 either), which holds every file under 300 KB.
    Under KL at d 128 the reference's own N(0.01, 0.02) initialisation makes the attention's covariances about 2.3 a lane, and its
    kl_distance_matmul takes their PRODUCT over the 128 lanes of a head (stosa/modules.py:53-55): 2.3^128 overflows fp32 and every output is
    NaN.  stosa_kl_hd128 therefore shifts the cov_query / cov_key biases by -0.7 (stored as cov_qk_bias), which keeps the products finite."""
    kw = dict(compact=True, thresh=2048, nsample=STOSA_ODD_COMPACT, keep_w1=False)
    for metric in ("wasserstein", "kl"):
        gen_stosa("hd128", dict(item_size=42, maxlen=12, hidden_units=128, num_heads=1, num_layers=1, num_users=4, pvn_weight=0.005), B=4, seed=51,
                  lam1=[0.3], lam2=[0.2], metric=metric, cov_qk_bias=-0.7 if metric == "kl" else 0.0, **kw)
        gen_stosa("w100_h1", dict(item_size=42, maxlen=12, hidden_units=100, num_heads=1, num_layers=1, num_users=4, pvn_weight=0.005), B=4, seed=52,
                  lam1=[0.3], lam2=[0.2], metric=metric, **kw)
    gen_stosa("hd128_h2", dict(item_size=33, maxlen=20, hidden_units=256, num_heads=2, num_layers=2, num_users=3, pvn_weight=0.1), B=3, seed=53,
              lam1=[0.25, 0.1], lam2=[0.15, 0.05], keep_w3=False, steps=1, **kw)


def main_kl_rowwise():
    """stosa_kl_rowwise.npz: the model, seed and input_ids of stosa_kl_small.npz; rowwise_dist[b][v] = the reference's kl_distance
    (stosa/modules.py:45-50) of user b's last-position (mean, cov) from item v's (mean, ELU(cov) + 1), every row of the item tables --
    the row-wise divergence bpr_optimization trains on, not kl_predict_full's score."""
    cfg_kw = dict(item_size=42, maxlen=12, hidden_units=64, num_heads=4, num_layers=1, num_users=4, pvn_weight=0.005)
    B, seed = 4, 21
    cfg, a, m, modules, (inp, dec, pos, neg) = reference_model(cfg_kw, B, seed, "kl")
    m.eval()
    with torch.no_grad():
        mo, co = m.finetune(torch.from_numpy(inp), torch.from_numpy(dec), torch.zeros(B, dtype=torch.long))[:2]
        sm, sc = mo[:, -1, :], co[:, -1, :]
        Em, Ec = m.item_mean_embeddings.weight, nn.ELU()(m.item_cov_embeddings.weight) + 1
        V = Em.shape[0]
        dist = torch.stack([modules.kl_distance(sm[b:b + 1].expand(V, -1), sc[b:b + 1].expand(V, -1), Em, Ec) for b in range(B)])
    out = {"seed": seed, "input_ids": inp, "pvn_weight": cfg.pvn_weight, "last_mean": sm.numpy(), "last_cov": sc.numpy(), "rowwise_dist": dist.numpy(),
           "cfg": np.array([cfg.item_size, cfg.maxlen, cfg.hidden_units, cfg.num_heads, cfg.num_layers, cfg.num_users])}
    path = os.path.join(OUT, "stosa_kl_rowwise.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, "rowwise_dist", out["rowwise_dist"].shape, "%.1f KB" % (os.path.getsize(path) / 1024))


if __name__ == "__main__":
    import argparse
    sys.path.insert(0, REPO)
    ap = argparse.ArgumentParser()
    ap.add_argument("--metric", default="wasserstein", choices=["wasserstein", "kl", "kl_rowwise", "long", "stosa_odd", "stosa_kl_odd", "stosa_hd128"])
    metric = ap.parse_args().metric
    if metric == "stosa_odd":
        main_odd()
    elif metric == "stosa_kl_odd":
        main_kl_odd()
    elif metric == "stosa_hd128":
        main_hd128()
    else:
        main_kl_rowwise() if metric == "kl_rowwise" else (main_long() if metric == "long" else main(metric))
