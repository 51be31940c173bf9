"""SearcherEvolution for STOSA-ADT on the MI355X path -- the counterpart of the reference's stosa/searcher.py:23-279: warm up the
weight-sharing supernet with one random candidate per epoch (:235-240), then evolve a population of (reconstruction, independence)
weight candidates scored by the validation MRR of the full-sort ranking under each candidate's block choice (get_cand_MRR :123-129).

The supernet and its warm-up step run in libadt_hip.so (adt_amd/stosa/supernet.py); candidates are scored a chunk at a time -- one
batched pass of the validation set per chunk (adt_amd/supersearch.py), the full sort and the seen-item masking on the device; with
--device_batches the batches are cut there too, and with --device_scores so are the scores.
"""
import os

import numpy as np
import torch

from .. import ops
from .._lib import AdtError
from ..fullrank import fused_ids_or_two_pass
from ..supersearch import EvolutionSearch, cand_to_block, get_shared, result_name
from .datasets import DeviceDisenData, DisenDataset, get_user_seqs
from .supernet import DisenDistSASupernet, SuperStosaTrainer
from .trainer import get_full_sort_score, scores_from_hist


class SearcherEvolution:
    def __init__(self, args):
        self.args = args
        user_seq, max_item, valid_matrix, test_matrix, num_users = get_user_seqs(args.data_file)
        args.item_size, args.num_users, args.mask_id = max_item + 2, num_users, max_item + 1
        self.valid_matrix, self.test_matrix = valid_matrix, test_matrix
        self.train_ds = DisenDataset(args, user_seq, "train", seed=args.seed)
        self.valid_ds = DisenDataset(args, user_seq, "valid", args.eval_set, seed=args.seed + 1)
        self.test_ds = DisenDataset(args, user_seq, "test", args.eval_set, seed=args.seed + 2)
        # search space (stosa/searcher.py:54-55: both grids are the reconstruction grid)
        self.rec_choice = [0, 0.0001, 0.0005, 0.001, 0.005, 0.01]
        self.ind_choice = [0, 0.0001, 0.0005, 0.001, 0.005, 0.01]
        torch.manual_seed(args.seed)
        self.model = DisenDistSASupernet(args, self.rec_choice, self.ind_choice, allow_kl=True, allow_lanes=True)      # 'wasserstein' or 'kl', any width main.py takes
        self.trainer = SuperStosaTrainer(self.model, lr=args.lr, betas=(args.adam_beta1, args.adam_beta2), weight_decay=args.weight_decay,
                                         seed=args.seed)
        self.search_state = EvolutionSearch(args.num_layers, self._evaluate_for_search, "MRR", args.select_num, args.population_num, args.m_prob,
                                            args.crossover_num, args.mutation_num, args.scale_factor)
        self.eval_stats = {}
        # --device_batches: sequences, rating matrices and held-out ids resident on the GPU, for evaluate_candidates only
        self.dev_data = DeviceDisenData(user_seq, args.item_size, args.maxlen, self.model.dev, valid_matrix, test_matrix) \
            if getattr(args, "device_batches", False) else None

    @property
    def vis_dict(self):
        return self.search_state.vis_dict

    def _evaluate_for_search(self, cands):
        return self.evaluate_candidates(cands, fused=bool(getattr(self.args, "fused_eval", False)),
                                        rowwise=bool(getattr(self.args, "rowwise_eval", False)))

    def _stack_csr(self, ip, ix, copies):
        """Host CSR (indptr, indices) of one batch, repeated for `copies` stacked candidates, on the device."""
        ip = np.asarray(ip, np.int64)
        if ix.size == 0:
            return None, None
        ip_all = np.concatenate([ip[:-1] + k * ix.size for k in range(copies)] + [[copies * ix.size]])
        dev = self.model.dev
        assert ip_all.size == copies * (ip.size - 1) + 1
        return (torch.from_numpy(np.ascontiguousarray(ip_all, dtype=np.int32)).to(dev),
                torch.from_numpy(np.ascontiguousarray(np.tile(ix, copies), dtype=np.int32)).to(dev))

    def _seen_csr(self, matrix, users, copies):
        """CSR of the users' seen items, repeated for `copies` stacked candidates, on the device."""
        csr = matrix[users].tocsr()
        return self._stack_csr(csr.indptr, csr.indices, copies)

    @staticmethod
    def _stack_csr_device(indptr, indices, copies):
        """_stack_csr of a device pair (DeviceDisenData.eval_stage), made on the device: the indices repeated, the indptr blocks each
        offset by k * nnz.  nnz is the length of the slice, known on the host: no scipy, no upload, no read-back."""
        nnz = indices.numel()
        if nnz == 0:
            return None, None
        if copies == 1:
            return indptr, indices
        blocks = [indptr[:-1] + k * nnz for k in range(copies)] + [indptr[-1:] + (copies - 1) * nnz]
        return torch.cat(blocks), indices.repeat(copies)

    def _eval_batches(self, ds, matrix, device_batches):
        """One dict per validation batch: inp, the batch's seen CSR as stack(copies) -> device pair, answers_host (B, 1), min_unseen (the
        smallest number of unseen items of a user of the batch, from a host indptr) and, on the device route, answers (device int32)."""
        bs = self.args.eval_batch_size
        if device_batches:
            if self.dev_data is None:
                raise AdtError("evaluate_candidates(device_batches=True) needs the resident data: construct the searcher with args.device_batches")
            for s in range(0, len(ds), bs):
                st = self.dev_data.eval_stage(ds.data_type, s, min(bs, len(ds) - s))
                st["stack"] = lambda copies, st=st: self._stack_csr_device(st["indptr"], st["indices"], copies)
                yield st
            return
        for users, inp, dec, pos, neg, ans in ds.epoch_batches(bs, shuffle=False):
            csr = matrix[users].tocsr()
            most = int(np.diff(csr.indptr).max()) if len(users) else 0
            yield {"inp": inp, "answers_host": np.asarray(ans), "min_unseen": self.args.item_size - most,
                   "stack": lambda copies, csr=csr: self._stack_csr(csr.indptr, csr.indices, copies)}

    def evaluate_candidates(self, cands, dataset=None, matrix=None, group=8, prefix="V", fused=False, device_batches=None, device_scores=None,
                            rowwise=False):
        """Full-sort scores (Trainer.get_full_sort_score, stosa/trainer.py:62-86) of the supernet under every candidate of `cands`:
        every validation batch is ranked for `group` candidates per pass (distances, seen-item masking and top-40 on the device).
        fused (the search passes args.fused_eval; default off): the item image is packed once per call -- the candidates share the item tables --
        and each pass is one adt_full_rank_from call (first_id = 0) on the stacked rows instead of a (group * B, item_size) distance
        matrix; a pass with a user who has fewer than 40 unseen items falls back to the two-pass form.

        device_batches / device_scores (default: args.device_batches / args.device_scores, both off), independent of
        each other and of `fused`.  device_batches: the batches of the first len(dataset) users come from DeviceDisenData.eval_stage for
        the dataset's split ("valid" / "test"; `matrix` is not read: the resident rating matrix of that split is) and the stacked seen
        CSR is made on the device.  device_scores: the id lists stay on the GPU; every pass adds one group per stacked candidate to a
        (len(cands), 41) int64 histogram (ops.hit_hist), the fused / two-pass choice comes from the batch's min_unseen instead of a
        read-back, and one copy after the last batch feeds scores_from_hist per candidate (kept as self.last_hists).

        distance_metric 'kl' (DESIGN.md section 19): the KL item image is packed once per call and every pass is one
        adt_kldist_full_groups call with E = the batch's rows (the trailing batch has its own E); fused=True is an AdtError.

        rowwise=True under 'kl' (nothing changes under Wasserstein): candidates are ranked by the row-wise KL
        divergence the model is trained on, not by kl_predict_full's batch-dependent score.  kl_row_image() is packed once per call and
        every pass is one rank_full_candidates(first_id=0, rowwise=True); no pass falls back -- a row with fewer than 40 unseen items
        keeps its -1 tail, which the metrics count as no hit."""
        device_batches = bool(getattr(self.args, "device_batches", False)) if device_batches is None else device_batches
        device_scores = bool(getattr(self.args, "device_scores", False)) if device_scores is None else device_scores
        kl = self.model.distance_metric == "kl"
        if fused and kl:
            raise AdtError("evaluate_candidates(fused=True): the fused ranking is built for distance_metric='wasserstein' only; 'kl' scores "
                           "through the distance matrix (adt_kldist_full_groups)")
        image = self.model.item_image() if fused else None
        rowwise = bool(rowwise) and kl
        kl_image = self.model.kl_item_image() if kl and not rowwise else None      # the candidates share the item tables: packed once per call
        row_image = self.model.kl_row_image() if rowwise else None
        ds = self.valid_ds if dataset is None else dataset
        matrix = self.valid_matrix if matrix is None else matrix
        dev = self.model.dev
        shared = [get_shared(self.rec_choice, self.ind_choice, cand_to_block(self.rec_choice, self.ind_choice, c)[0]) for c in cands]
        preds = [[] for _ in cands]
        answers = []
        H = torch.zeros(len(cands), 41, device=dev, dtype=torch.int64) if device_scores else None
        for st in self._eval_batches(ds, matrix, device_batches):
            inp = st["inp"]
            B = len(inp)
            if device_scores:
                ans_dev = st["answers"] if "answers" in st else \
                    torch.from_numpy(np.ascontiguousarray(st["answers_host"].reshape(-1), dtype=np.int32)).to(dev)
            else:
                answers.append(st["answers_host"])
            for g0 in range(0, len(cands), group):
                sl = shared[g0:g0 + group]
                indptr, indices = st["stack"](len(sl))

                def two_pass_device():
                    dist = self.model.predict_full_candidates(inp, sl, stats=self.eval_stats, image=kl_image)
                    return ops.topk_masked(dist, 40, indptr, indices)

                def fused_device():
                    return self.model.rank_full_candidates(inp, sl, None, (indptr, indices), 40, image, self.eval_stats, first_id=0)[2]

                def rowwise_device():
                    return self.model.rank_full_candidates(inp, sl, None, (indptr, indices), 40, row_image, self.eval_stats, first_id=0,
                                                           rowwise=True)[2]
                if device_scores:
                    top_idx = rowwise_device() if rowwise else fused_device() if fused and st["min_unseen"] >= 40 else two_pass_device()
                    ops.hit_hist(top_idx, ans_dev, rows_per_group=B, hist=H[g0:g0 + len(sl)])
                    continue
                two_pass = lambda: two_pass_device().cpu().numpy().astype(np.int64)
                if rowwise:
                    top = rowwise_device().cpu().numpy().astype(np.int64)
                else:
                    top = fused_ids_or_two_pass(fused_device(), two_pass)[0] if fused else two_pass()
                for k in range(len(sl)):
                    preds[g0 + k].append(top[k * B:(k + 1) * B])
        if device_scores:
            self.last_hists = H.cpu().numpy()
            scores = [scores_from_hist(h) for h in self.last_hists]
        else:
            answers = np.concatenate(answers)
            scores = [get_full_sort_score(answers, np.concatenate(pk)) for pk in preds]
        return [{prefix + "_NDCG": float(s[5]), prefix + "_HR": float(s[4]), prefix + "_MRR": float(s[-1]), "MRR": float(s[-1])} for s in scores]

    def _train_warmup(self):
        """One random candidate per epoch (stosa/searcher.py:235-240).  Always on host batches, also under --device_batches: the warm-up is
        one pass per epoch, not one per candidate, and SuperStosaTrainer.step stages host arrays."""
        for epoch in range(self.args.warmup_epochs):
            self.trainer.set_choice(self.search_state.sample_random())
            for users, inp, dec, pos, neg, _ in self.train_ds.epoch_batches(self.args.batch_size):
                self.trainer.step(inp, dec, pos, neg)
            print("warmup epoch %d / %d loss %.4f" % (epoch + 1, self.args.warmup_epochs, float(self.trainer.loss())), flush=True)

    def search(self):
        self._train_warmup()
        os.makedirs("./checkpoint", exist_ok=True)
        torch.save(self.model.state_dict(), "./checkpoint/super.pth")
        self.search_state.run(self.args.search_epochs, log=lambda m: print(m, flush=True))
        return self.search_state.write(result_name(getattr(self.args, "out_dir", "res"), self.args), self.rec_choice, self.ind_choice)
