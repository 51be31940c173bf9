"""Host data pipeline of STOSA-ADT -- the counterpart of the reference's stosa/utils.py:get_user_seqs (:132-149),
generate_rating_matrix_{valid,test} (:96-130), neg_sample (:32-36) and stosa/datasets.py:DisenDataset (:202-300): the
same leave-two-out layout (train / valid / test views of one sequence), left padding, negatives outside the user's item
set.  Batches are built with numpy (one vectorised negative draw per batch with rejection) instead of per-sample tensors."""
import numpy as np
from scipy.sparse import csr_matrix


def get_user_seqs(data_file):
    """(user_seq, max_item, valid_rating_matrix, test_rating_matrix, num_users); each line is `user item item ...`."""
    user_seq, max_item = [], 0
    with open(data_file) as f:
        for line in f:
            _, items = line.strip().split(" ", 1)
            items = [int(x) for x in items.split(" ")]
            user_seq.append(items)
            max_item = max(max_item, max(items))
    num_users, num_items = len(user_seq), max_item + 2
    return user_seq, max_item, rating_matrix(user_seq, num_users, num_items, 2), rating_matrix(user_seq, num_users, num_items, 1), num_users


def rating_matrix(user_seq, num_users, num_items, holdout):
    """generate_rating_matrix_valid (holdout 2) / _test (holdout 1): the items a user has seen before the answer."""
    row, col = [], []
    for u, items in enumerate(user_seq):
        seen = items[:-holdout]
        row += [u] * len(seen)
        col += seen
    return csr_matrix((np.ones(len(row)), (np.array(row), np.array(col))), shape=(num_users, num_items))


class DisenDataset:
    def __init__(self, args, user_seq, data_type="train", eval_set=-1, seed=42):
        assert data_type in ("train", "valid", "test")
        self.args, self.user_seq, self.data_type, self.max_len = args, user_seq, data_type, args.maxlen
        self.n = len(user_seq) if eval_set == -1 else min(eval_set, len(user_seq))
        self.sets = [set(s) for s in user_seq]
        self.rng = np.random.RandomState(seed)

    def __len__(self):
        return self.n

    def _views(self, items):
        """datasets.py:230-246."""
        if self.data_type == "train":
            return items[:-3], items[1:-2], items[:-4], [0]
        if self.data_type == "valid":
            return items[:-2], items[1:-1], items[:-3], [items[-2]]
        return items[:-1], items[1:], items[:-2], [items[-1]]

    def batch(self, users):
        L, size = self.max_len, self.args.item_size
        B = len(users)
        inp, dec, pos, neg = (np.zeros((B, L), np.int32) for _ in range(4))
        ans = np.zeros((B, 1), np.int64)
        for r, u in enumerate(users):
            input_ids, target_pos, dec_ids, answer = self._views(self.user_seq[u])
            input_ids, target_pos, dec_ids = input_ids[-L:], target_pos[-L:], dec_ids[-L:]
            n = len(input_ids)
            if n:
                inp[r, L - n:], pos[r, L - n:] = input_ids, target_pos
                tn = self.rng.randint(1, size, size=n)      # neg_sample: uniform in [1, item_size - 1], outside the user's items
                bad = np.array([t in self.sets[u] for t in tn])
                while bad.any():
                    tn[bad] = self.rng.randint(1, size, size=int(bad.sum()))
                    bad = np.array([t in self.sets[u] for t in tn])
                neg[r, L - n:] = tn
            if len(dec_ids):
                dec[r, L - len(dec_ids):] = dec_ids
            ans[r, 0] = answer[0]
        return np.asarray(users, np.int64), inp, dec, pos, neg, ans

    def epoch_batches(self, batch_size, shuffle=True):
        order = self.rng.permutation(self.n) if shuffle else np.arange(self.n)
        for s in range(0, self.n, batch_size):
            yield self.batch(order[s:s + batch_size])


class DeviceDisenData:
    """DisenDataset's batches built on the GPU (adt_seqbatch_build).  Resident on the device as int32 CSR, uploaded
    once: the user sequences, every user's sorted item set (the whole sequence, as DisenDataset.sets), the valid / test rating
    matrices and the held-out ids of both splits; every indptr is kept on the host as well, so a contiguous user range is sliced without
    a device read.  No call below copies ids, CSR rows or normalisers from the host."""
    CUT = {"train": 3, "valid": 2, "test": 1}

    def __init__(self, user_seq, item_size, maxlen, device, valid_matrix, test_matrix):
        import torch
        self.item_size, self.max_len, self.dev, self.n = int(item_size), int(maxlen), torch.device(device), len(user_seq)
        sets = [sorted(set(s)) for s in user_seq]
        assert all(len(s) > 0 and q[0] >= 1 and q[-1] < self.item_size for s, q in zip(user_seq, sets)), "item ids must lie in [1, item_size - 1]"

        def csr(rows):
            off = np.zeros(len(rows) + 1, np.int64)
            np.cumsum([len(r) for r in rows], out=off[1:])
            items = np.fromiter((x for r in rows for x in r), np.int32, count=int(off[-1]))
            return torch.from_numpy(off).to(self.dev), torch.from_numpy(items).to(self.dev)
        self.seq_off, self.seq_items = csr(user_seq)
        self.set_off, self.set_items = csr(sets)
        self.seen, self.answers, self.answers_dev = {}, {}, {}
        for split, matrix in (("valid", valid_matrix), ("test", test_matrix)):
            m = matrix.tocsr()
            assert m.shape[0] == self.n, (m.shape, self.n)
            ip = np.ascontiguousarray(m.indptr, dtype=np.int32)
            self.seen[split] = (ip, torch.from_numpy(ip).to(self.dev), torch.from_numpy(np.ascontiguousarray(m.indices, dtype=np.int32)).to(self.dev))
            c = self.CUT[split]      # the held-out item; 0 for a sequence too short to have one (DisenDataset raises IndexError there)
            self.answers[split] = np.array([[s[-c] if len(s) >= c else 0] for s in user_seq], np.int64)
            self.answers_dev[split] = torch.from_numpy(self.answers[split][:, 0].astype(np.int32)).to(self.dev)
        self._all_users = torch.arange(self.n, device=self.dev, dtype=torch.int32)
        self.order = None

    def __len__(self):
        return self.n

    def set_order(self, order):
        """Upload one epoch's user permutation (the only host -> device copy of an epoch)."""
        import torch
        order = np.ascontiguousarray(order, dtype=np.int32)
        assert order.ndim == 1 and (order.size == 0 or (order.min() >= 0 and order.max() < self.n)), "order holds a user outside 0..n-1"
        self.order = torch.from_numpy(order).to(self.dev)

    def train_stage(self, start, B, seed, step, rows=None):
        """The `stage` dict of TapeTrainer.step_staged for users order[start:start + B] -- under data parallelism rows (lo, hi) of that
        global batch, with the global inv_count and the negatives the whole batch would get."""
        from .. import ops
        assert self.order is not None and 0 <= start and start + B <= self.order.numel(), "set_order first; the batch must lie inside it"
        lo, hi = (0, B) if rows is None else rows
        inp, dec, pos, neg, inv_count = ops.seqbatch_build(self.seq_off, self.seq_items, self.set_off, self.set_items, self.order[start:start + B],
                                                           self.max_len, self.CUT["train"], self.item_size, seed, step, (lo, hi))
        return {"B": hi - lo, "B_global": B, "inp": inp, "dec": dec, "pos": pos, "neg": neg, "inv_count": inv_count}

    def eval_batch(self, split, start, B):
        """(inp device (B, L), (indptr, indices) device int32, answers numpy (B, 1)) of the contiguous users start .. start + B - 1: what
        FusedStosaTrainer.full_sort takes for (DisenDataset.batch's input_ids, matrix[users], answers)."""
        from .. import ops
        assert split in self.seen and 0 <= start and start + B <= self.n, (split, start, B, self.n)
        inp = ops.seqbatch_build(self.seq_off, self.seq_items, self.set_off, self.set_items, self._all_users[start:start + B], self.max_len,
                                 self.CUT[split], self.item_size, want_neg=False, want_inv_count=False, views=False)[0]
        ip, ip_dev, ix_dev = self.seen[split]
        indptr = ip_dev[start:start + B + 1] - int(ip[start])
        return inp, (indptr, ix_dev[int(ip[start]):int(ip[start + B])]), self.answers[split][start:start + B]

    def eval_stage(self, split, start, B):
        """eval_batch as a dict for FusedStosaTrainer.full_sort_scores and the search: inp, indptr, indices (eval_batch's), answers (the
        resident held-out ids, device int32 (B,)), answers_host (eval_batch's numpy (B, 1)) and min_unseen -- the smallest number of items
        a user of the batch has not seen, item_size - max(stored entries per row), a host int from the host indptr: a fused ranking
        (first_id = 0) returns topk ids for every row exactly when min_unseen >= topk."""
        inp, (indptr, indices), ans = self.eval_batch(split, start, B)
        ip = self.seen[split][0]
        most = int(np.diff(ip[start:start + B + 1]).max()) if B > 0 else 0
        return {"inp": inp, "indptr": indptr, "indices": indices, "answers": self.answers_dev[split][start:start + B], "answers_host": ans,
                "min_unseen": self.item_size - most}
