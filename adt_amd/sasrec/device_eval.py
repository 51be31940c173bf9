"""The sampled-negative evaluation of SASRec-ADT kept in HBM: the evaluation users' sequences, their sorted seen
rows, the popularity table, the held-out targets and the (N, 1 + S) candidate table are uploaded once; a batch is two views and one
kernel launch, and the candidates can be drawn on the device (adt_evalcand_draw) instead of by PopularSampler.get_negative_samples.
"""
import numpy as np
import torch

from .. import _lib, ops


def _csr(rows, dtype=np.int32):
    off = np.zeros(len(rows) + 1, np.int64)
    np.cumsum([len(r) for r in rows], out=off[1:])
    items = np.zeros(max(int(off[-1]), 1), dtype)      # never empty: the kernels take its address
    if off[-1]:
        items[:off[-1]] = np.concatenate([np.asarray(r, dtype) for r in rows if len(r)])
    return off, items


class DeviceEvalData:
    """EvalDataset's rows on the device.  The user list follows EvalDataset's rule and order (users with a held-out item of this mode and
    a non-empty training history; eval_set >= 0 draws that many with numpy.random.choice, as EvalDataset does), or is `users` when given.

    Resident: the sequences train + [valid] + [test] as CSR over the evaluation rows, the sorted seen rows (train + valid, plus test in
    test mode) as CSR, `cum` (prefix sums of the item counts over train + valid + test, ids 0 .. itemnum - 1: PopularSampler's table),
    the targets and the candidate table `cand` (N, 1 + S).  draw() fills `cand` on the device; from_dataset() uploads a host
    EvalDataset's frozen candidates instead."""

    def __init__(self, user_train, user_valid, user_test, usernum, itemnum, maxlen, sample_size, mode="val", eval_set=-1, device="cuda",
                 users=None):
        if mode not in ("val", "test"):
            raise ValueError("DeviceEvalData: mode %r (val or test)" % (mode,))
        self.usernum, self.itemnum, self.maxlen, self.sample_size, self.mode = usernum, itemnum, int(maxlen), int(sample_size), mode
        self.device = torch.device(device)
        tgt = user_valid if mode == "val" else user_test
        if users is None:
            pool = range(1, usernum + 1) if eval_set is None or eval_set < 0 else \
                np.random.choice(np.arange(1, usernum + 1), eval_set, replace=False)
            users = [int(u) for u in pool if len(tgt.get(int(u), [])) != 0 and len(user_train.get(int(u), [])) != 0]
        self.users = [int(u) for u in users]
        if not 1 <= self.sample_size <= ops.EVALCAND_MAX_S:
            raise _lib.AdtError("DeviceEvalData: sample_size=%d outside 1..%d" % (self.sample_size, ops.EVALCAND_MAX_S))
        # the popularity table, indexed as the reference indexes it: count[i] for i in range(itemnum), so id 0 (count 0) and id itemnum
        # (outside the range) are never drawn
        acts = [np.asarray(part[u], np.int64) for part in (user_train, user_valid, user_test) for u in range(1, usernum + 1) if len(part.get(u, []))]
        count = np.bincount(np.concatenate(acts) if acts else np.zeros(0, np.int64), minlength=itemnum + 1)
        self.cum_host = np.zeros(itemnum + 1, np.int64)
        np.cumsum(count[:itemnum], out=self.cum_host[1:])
        self.total = int(self.cum_host[-1])
        if not 1 <= self.total < 2 ** 32:
            raise _lib.AdtError("DeviceEvalData: the item counts sum to %d, outside 1 .. 2^32 - 1" % self.total)
        seqs, seen, targets = [], [], []
        for u in self.users:
            va, te = list(user_valid.get(u, [])), list(user_test.get(u, []))
            if mode == "test" and not va:
                raise _lib.AdtError("DeviceEvalData: user %d has a test item and no validation item" % u)
            # exactly one slot each for the validation and the test item, so that cutting 2 (val) / 1 (test) leaves EvalDataset.sequence
            seqs.append(list(user_train[u]) + [va[0] if va else 0] + [te[0] if te else 0])
            targets.append(tgt[u][0])
            seen.append(np.unique(np.asarray(list(user_train[u]) + va + (te if mode == "test" else []), np.int64)))
        # adt_evalcand_draw fills open slots with id 0 where the reference would spin forever: refuse such a user here, once
        nz = count[:itemnum] > 0
        nz[0] = False
        n_drawable = int(nz.sum())
        for u, s in zip(self.users, seen):
            free = n_drawable - int(nz[s[s < itemnum]].sum())
            if free < self.sample_size:
                raise _lib.AdtError("DeviceEvalData: user %d has %d drawable items, sample_size is %d" % (u, free, self.sample_size))
        self.targets_host = np.asarray(targets, np.int32)
        dev = self.device
        self.seq_off, self.seq_items = (torch.from_numpy(x).to(dev) for x in _csr(seqs))
        self.seen_off, self.seen_items = (torch.from_numpy(x).to(dev) for x in _csr(seen))
        self.cum = torch.from_numpy(self.cum_host).to(dev)
        self.targets = torch.from_numpy(self.targets_host).to(dev)
        self.rows = torch.arange(len(self.users), device=dev, dtype=torch.int32)
        self.cand = torch.zeros(len(self.users), 1 + self.sample_size, device=dev, dtype=torch.int32)
        self.cand[:, 0] = self.targets
        self.drawn = False

    def __len__(self):
        return len(self.users)

    @property
    def n_candidates(self):
        return 1 + self.sample_size

    @classmethod
    def from_dataset(cls, eval_ds, device="cuda", upload=True):
        """The device copy of a host EvalDataset: its users, and (upload=True) its frozen candidates, so the ranks are the host path's own."""
        self = cls(eval_ds.user_train, eval_ds.user_val, eval_ds.user_test, eval_ds.usernum, eval_ds.itemnum, eval_ds.maxlen,
                   eval_ds.negative_sampler.sample_size, eval_ds.mode, device=device, users=eval_ds.users)
        if upload:
            if eval_ds._frozen is None:
                raise _lib.AdtError("DeviceEvalData.from_dataset: the EvalDataset redraws its candidates on every access (frozen=False); "
                                    "there is no candidate set to upload")
            if len(self.users):
                self.cand.copy_(torch.from_numpy(np.stack([np.asarray(eval_ds._frozen[u], np.int32) for u in self.users])))
            self.drawn = True
        return self

    def draw(self, seed, salt=0, rows=None, want_filled=False):
        """Fill (rows lo:hi of) the candidate table with adt_evalcand_draw: a hash stream of (seed, salt, row), not numpy's."""
        lo, hi = (0, len(self.users)) if rows is None else rows
        self.drawn = True
        if hi == lo:
            return (self.cand[lo:hi], torch.zeros(0, device=self.device, dtype=torch.int32)) if want_filled else self.cand[lo:hi]
        return ops.evalcand_draw(self.cum, self.total, self.seen_off, self.seen_items, self.targets, self.sample_size, seed, salt, rows=(lo, hi),
                                 out=self.cand[lo:hi], want_filled=want_filled)

    def sequences(self, lo, hi):
        """(hi - lo, L) int32: EvalDataset.sequence of rows lo:hi.  No kernel of its own: with train + [valid] + [test] as the CSR,
        adt_seqbatch_build's input view at cut 2 (val) / 1 (test) is exactly that row (the last L items of s[:-cut], left-padded)."""
        return ops.seqbatch_build(self.seq_off, self.seq_items, self.seen_off, self.seen_items, self.rows, self.maxlen, 2 if self.mode == "val" else 1,
                                  self.itemnum + 1, rows=(lo, hi), want_neg=False, want_inv_count=False, views=False)[0]

    def batch(self, lo, hi):
        """(seq (hi - lo, L), cand (hi - lo, 1 + S)) of rows lo:hi, both on the device; cand is a view of the resident table."""
        if not self.drawn:
            raise _lib.AdtError("DeviceEvalData: no candidates yet (draw() or from_dataset())")
        return self.sequences(lo, hi), self.cand[lo:hi]

    def full_batch(self, lo, hi):
        """What the full-catalogue evaluation of rows lo:hi reads (ops.full_rank_groups): (seq (hi - lo, L), targets, seen_off, seen_items,
        row0 = lo).  The last four name the RESIDENT tensors of the whole set -- the kernel finds the rows from row0 --, so nothing is
        sliced or re-based, and no candidate table is needed: a set that was never drawn serves this."""
        return self.sequences(lo, hi), self.targets, self.seen_off, self.seen_items, lo

    def batches(self, batch_size):
        for lo in range(0, len(self.users), batch_size):
            yield lo, min(lo + batch_size, len(self.users))
