#!/usr/bin/env python3
"""Evolutionary search of the per-layer (reconstruction, independence) loss weights of BERT4Rec-ADT on the MI355X path -- the entry
point mirroring the reference's bert4rec/evolution.py: warm up the weight-sharing supernet with one random candidate per epoch
(SearcherEvolution._train_warmup, :253-296), then evolve a population of candidates scored by the validation AUC of the supernet under
each candidate's block choice (get_cand_auc :150-157; random init, top-k, mutation, crossover :170-251; search :298-347).

    python -m adt_amd.bert4rec.evolution --dataset ml-1m --synthetic ml1m-small --warmup_epochs 2 --search_epochs 2 ...

The supernet forward / backward / AdamW run in libadt_hip.so (adt_amd/bert4rec/superbert.py); the population bookkeeping and the batched
candidate evaluation are adt_amd/supersearch.py.  Same flags (bert4rec/options.py) and the same result file.  Extra flags (not in the
reference): --device_batches, --remask_every_epoch, --device_scores and --device_negatives keep the warm-up batches, the evaluation rows,
the scores and the candidate draw on the GPU.
"""
import argparse
import json
import os
import random

import numpy as np
import torch

from .._lib import AdtError
from ..sasrec.utils import metrics_from_hist, metrics_from_ranks
from ..supersearch import EvolutionSearch, cand_to_block, get_shared, result_name
from . import datasets as D
from . import utils as U
from .superbert import SuperBertModel, SuperBertTrainer


def parse_args(argv=None):
    p = argparse.ArgumentParser()       # bert4rec/options.py:7-65
    p.add_argument("--dataset", default="ml-1m")
    p.add_argument("--data_dir", default="data")
    p.add_argument("--synthetic", default=None)
    p.add_argument("--dataset_random_seed", type=int, default=23)
    p.add_argument("--eval_set_size", type=int, default=-1)
    p.add_argument("--batch_size", type=int, default=256)
    p.add_argument("--eval_batch_size", type=int, default=512)
    p.add_argument("--eval_negative_sample_size", type=int, default=100)
    p.add_argument("--device", default="cuda:0")
    p.add_argument("--lr", type=float, default=0.001)
    p.add_argument("--weight_decay", type=float, default=0.001)
    p.add_argument("--clip", type=int, default=5)
    p.add_argument("--dupe_factor", type=int, default=10)
    p.add_argument("--prop_sliding_window", type=float, default=0.1)
    p.add_argument("--type_vocab_size", type=int, default=2)
    p.add_argument("--initializer_range", type=float, default=0.02)
    p.add_argument("--maxlen", type=int, default=200)
    p.add_argument("--hidden_units", type=int, default=64)
    p.add_argument("--inner_units", type=int, default=128)
    p.add_argument("--num_layers", type=int, default=2)
    p.add_argument("--num_heads", type=int, default=2)
    p.add_argument("--dropout", type=float, default=0.2)
    p.add_argument("--attention_dropout", type=float, default=0.2)
    p.add_argument("--mask_prob", type=float, default=0.2)
    p.add_argument("--template", type=lambda s: str(s).lower() in ("1", "true", "yes"), default=False)
    p.add_argument("--override", default=None, help="JSON applied after the template")
    p.add_argument("--warmup_epochs", default=200, type=int)
    p.add_argument("--search_epochs", default=500, type=int)
    p.add_argument("--population_num", type=int, default=100)
    p.add_argument("--select_num", type=int, default=50)
    p.add_argument("--m_prob", type=float, default=0.1)
    p.add_argument("--crossover_num", type=int, default=25)
    p.add_argument("--mutation_num", type=int, default=25)
    p.add_argument("--seed", type=int, default=2022)
    p.add_argument("--scale_factor", type=float, default=0.5)
    p.add_argument("--scale_decay_rate", type=float, default=0.5)
    p.add_argument("--precision", default="bf16", choices=["bf16", "f32"])
    p.add_argument("--out_dir", default="res")
    p.add_argument("--device_batches", action="store_true",
                   help="keep the sequences on the GPU: the warm-up batches are masked and built there (adt_bertbatch_build; no BertTrainDataset "
                        "is constructed, the trailing short batch of an epoch is dropped) and so are the evaluation rows of every candidate "
                        "pass; the masks come from a different random stream, so such a run is not the host run's trajectory")
    p.add_argument("--remask_every_epoch", action="store_true",
                   help="with --device_batches: draw a fresh set of masks every warm-up epoch instead of one per example for the whole run")
    p.add_argument("--device_scores", action="store_true",
                   help="count the ranks of every candidate pass on the GPU (adt_cand_rank_hist) and read one histogram per call of "
                        "evaluate_candidates instead of the ranks of every pass; the same ranks")
    p.add_argument("--device_negatives", action="store_true",
                   help="with --device_batches: draw the evaluation candidates on the GPU (adt_evalcand_draw), once per run, instead of with the "
                        "host sampler.  Same distribution as the numpy sampler's candidates, but a hash stream of its own: different "
                        "candidates and therefore different metrics")
    args = p.parse_args(argv)
    if args.remask_every_epoch and not args.device_batches:
        p.error("--remask_every_epoch needs --device_batches")
    if args.device_negatives and not args.device_batches:
        p.error("--device_negatives needs --device_batches")
    return args


class SearcherEvolution:
    def __init__(self, args):
        self.args = args
        path = os.path.join(args.data_dir, "%s.txt" % args.dataset)
        if not os.path.exists(path) and args.synthetic:
            from ..sasrec import synth
            os.makedirs(args.data_dir, exist_ok=True)
            h, _, _ = synth.generate(args.synthetic, 23)
            synth.write(path, h)
        user_train, user_valid, user_test, usernum, itemnum = self.dataset = D.data_partition(args.dataset, args.data_dir)
        # --device_batches: the sequences resident on the GPU; the host training set is not built at all
        self.train_ds = self.dev_data = None
        if getattr(args, "device_batches", False):
            self.dev_data = D.DeviceBertData(user_train, usernum, itemnum, args.maxlen, args.mask_prob, args.device, args.dupe_factor,
                                             args.prop_sliding_window)
        else:
            self.train_ds = D.BertTrainDataset(user_train, usernum, itemnum, args.maxlen, args.mask_prob, args.dataset_random_seed,
                                               args.dupe_factor, args.prop_sliding_window)
        sampler = D.PopularSampler(user_train, user_valid, user_test, usernum, itemnum, args.eval_negative_sample_size)
        self.val_ds = D.BertEvalDataset(user_train, user_valid, user_test, usernum, itemnum, args.maxlen, sampler, "val", args.eval_set_size)
        self.test_ds = D.BertEvalDataset(user_train, user_valid, user_test, usernum, itemnum, args.maxlen, sampler, "test", args.eval_set_size)
        if self.dev_data is not None and getattr(args, "device_negatives", False):
            # the host sampler is never called; one draw for the whole run, seeds 23 / 24 keep the two sets apart (as bert4rec/main.py)
            self.dev_data.add_eval(self.val_ds, candidates="device"), self.dev_data.add_eval(self.test_ds, candidates="device")
            self.dev_data.draw_eval("val", 23), self.dev_data.draw_eval("test", 24)
        elif self.dev_data is not None:
            self.dev_data.add_eval(self.val_ds), self.dev_data.add_eval(self.test_ds)
        # search space (bert4rec/evolution.py:71-77)
        self.rec_choice = [0, 0.0001, 0.0005, 0.001, 0.005, 0.01]
        self.ind_choice = [0, 0.0001, 0.0005, 0.001, 0.0015, 0.002]
        torch.manual_seed(args.seed)
        self.model = SuperBertModel(usernum, itemnum, self.rec_choice, self.ind_choice, args, allow_lanes=True)
        self.trainer = SuperBertTrainer(self.model, lr=args.lr, betas=(0.9, 0.999), weight_decay=args.weight_decay, clip=args.clip, seed=args.seed)
        self.search_state = EvolutionSearch(args.num_layers, self.evaluate_candidates, "auc", args.select_num, args.population_num, args.m_prob,
                                            args.crossover_num, args.mutation_num, args.scale_factor)
        self.rng = np.random.RandomState(args.seed)
        self.eval_stats = {}

    @property
    def vis_dict(self):
        return self.search_state.vis_dict

    def evaluate_candidates(self, cands, dataset=None, group=16, device_batches=None, device_scores=None):
        """Validation metrics (evaluate_loader, bert4rec/utils.py; ks = [10]) of the supernet under every candidate of `cands`: each
        validation batch is scored for `group` candidates per pass.

        device_batches / device_scores (default: args.device_batches / args.device_scores, both off), independent of
        each other.  device_batches: the batches come from DeviceBertData.eval_batches for the dataset's mode -- rows built on the device,
        candidates a view of the resident table.  device_scores: every pass adds its group's rows to a (len(cands), C) int64 histogram
        (rank_hist_candidates), read once after the last batch and turned into the metrics by metrics_from_hist per candidate."""
        device_batches = bool(getattr(self.args, "device_batches", False)) if device_batches is None else device_batches
        device_scores = bool(getattr(self.args, "device_scores", False)) if device_scores is None else device_scores
        ds = self.val_ds if dataset is None else dataset
        shared = [get_shared(self.rec_choice, self.ind_choice, cand_to_block(self.rec_choice, self.ind_choice, c)[0]) for c in cands]
        if device_batches:
            if self.dev_data is None:
                raise AdtError("evaluate_candidates(device_batches=True) needs the resident data: construct the searcher with args.device_batches")
            batches = self.dev_data.eval_batches(ds.mode, self.args.eval_batch_size)
        else:
            batches = ds.batches(self.args.eval_batch_size)
        ranks = [[] for _ in cands]
        ncand, hist = None, None
        for seq, cand_items in batches:
            ncand = cand_items.shape[1]
            if device_scores:
                if hist is None:
                    hist = torch.zeros(len(cands), ncand, device=self.model.dev, dtype=torch.int64)
                seq, cand_items = self.model.ids(seq), self.model.ids(cand_items)      # host batches: one upload per batch, not per group
            for g0 in range(0, len(cands), group):
                if device_scores:
                    self.model.rank_hist_candidates(seq, cand_items, shared[g0:g0 + group], hist[g0:g0 + group], stats=self.eval_stats)
                    continue
                r = self.model.predict_rank_candidates(seq, cand_items, shared[g0:g0 + group], stats=self.eval_stats).cpu().numpy()
                for k in range(r.shape[0]):
                    ranks[g0 + k].append(r[k])
        if device_scores:
            found = [metrics_from_hist(h, ncand, [10]) for h in hist.cpu().numpy()]
        else:
            found = [metrics_from_ranks(np.concatenate(rk), ncand, [10]) for rk in ranks]
        out = []
        for (ndcg, hr), auc in found:
            out.append({"V_NDCG": float(ndcg[10]), "V_HR": float(hr[10]), "V_AUC": float(auc), "auc": float(auc)})
        return out

    def _train_warmup(self):
        B = self.args.batch_size
        for epoch in range(self.args.warmup_epochs):
            self.trainer.set_choice(self.search_state.sample_random())
            if self.dev_data is not None:
                # as bert4rec/main.py: the permutation BertTrainDataset.epoch_batches would draw, uploaded once; full batches only; the
                # masks of salt 0 for the whole run, or of salt = epoch under --remask_every_epoch
                data = self.dev_data
                data.set_order(self.rng.permutation(len(data)))
                salt = epoch if getattr(self.args, "remask_every_epoch", False) else 0
                for i in range(len(data) // B):
                    self.trainer.step_device(data.train_stage(i * B, B, self.args.dataset_random_seed, salt))
            else:
                for src, dec, lab in self.train_ds.epoch_batches(B, self.rng):
                    self.trainer.step(src, dec, lab)
            print("warmup epoch %d / %d loss %.4f" % (epoch + 1, self.args.warmup_epochs, float(self.trainer.loss())), flush=True)

    def search(self):
        self._train_warmup()
        os.makedirs("./checkpoint", exist_ok=True)
        torch.save(self.model.state_dict(), "./checkpoint/super.pth")
        self.search_state.run(self.args.search_epochs, log=lambda m: print(m, flush=True))
        return self.search_state.write(result_name(self.args.out_dir, self.args), self.rec_choice, self.ind_choice)


def set_rng_seed(seed):
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)


def main(argv=None):
    args = parse_args(argv)
    if args.template:
        args = U.set_template(args)
    if args.override:
        for k, v in json.loads(args.override).items():
            setattr(args, k, v)
    set_rng_seed(args.seed)
    s = SearcherEvolution(args)
    print("results:", s.search())


if __name__ == "__main__":
    main()
