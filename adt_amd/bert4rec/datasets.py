"""Host data pipeline of BERT4Rec-ADT -- the counterpart of the reference's bert4rec/datasets/dataset.py: the same split
(data_partition :16-47), the same masked-sequence generation (BertTrainDataset :49-156: per user `dupe_factor` randomly
masked copies of every sliding window plus one copy with only the last item masked; 80 % [MASK] / 10 % random item / 10 %
kept; the decoder input always ends in [MASK]) and the same evaluation rows (BertEvalDataset :176-222: history + [MASK],
positive + popularity negatives).  Arrays are built once with numpy instead of per-sample LongTensors, and batches are
plain int32 arrays for FusedBertTrainer."""
import random
from collections import Counter, defaultdict

import numpy as np


def data_partition(fname, data_dir="data"):
    """bert4rec/datasets/dataset.py:16-47 (users with < 3 interactions are train-only)."""
    usernum = itemnum = 0
    User = defaultdict(list)
    with open("%s/%s.txt" % (data_dir, fname)) as f:
        for line in f:
            u, i = line.rstrip().split(" ")
            u, i = int(u), int(i)
            usernum, itemnum = max(u, usernum), max(i, itemnum)
            User[u].append(i)
    train, valid, test = {}, {}, {}
    for user, items in User.items():
        if len(items) < 3:
            train[user], valid[user], test[user] = items, [], []
        else:
            train[user], valid[user], test[user] = items[:-2], [items[-2]], [items[-1]]
    return [train, valid, test, usernum, itemnum]


class PopularSampler:
    """bert4rec/datasets/negative_sampler.py PopularSampler: `sample_size` negatives per user drawn by item popularity
    among the items the user has not interacted with."""

    def __init__(self, train, val, test, usernum, itemnum, sample_size, seed=23):
        cnt = Counter()
        for d in (train, val, test):
            for items in d.values():
                cnt.update(items)
        self.items = np.array(sorted(cnt), np.int64)
        p = np.array([cnt[i] for i in self.items], np.float64)
        self.p = p / p.sum()
        self.train, self.val, self.test, self.sample_size = train, val, test, sample_size
        self.rng = np.random.RandomState(seed)
        self._cache = {}

    def get_negative_samples(self, user, mode="val"):
        key = (user, mode)
        if key not in self._cache:      # frozen per (user, mode): two evaluations rank the same candidates
            seen = set(self.train.get(user, [])) | set(self.val.get(user, [])) | set(self.test.get(user, []))
            out = []
            while len(out) < self.sample_size:
                for it in self.rng.choice(self.items, size=2 * self.sample_size, p=self.p):
                    if it not in seen and it not in out:
                        out.append(int(it))
                        if len(out) == self.sample_size:
                            break
            self._cache[key] = out
        return self._cache[key]


def device_candidate_tables(train, val, test, itemnum, users, sample_size):
    """What DeviceBertData.add_eval(candidates="device") uploads for `users`, prepared on the host (no GPU): PopularSampler's table and
    seen sets in the form adt_evalcand_draw reads.  Returns (cum, total, seen_off, seen_items): cum (itemnum + 2,) int64, the exact prefix
    sums of the item counts over train + val + test indexed by item id, cum[0] = 0 and cum[i + 1] - cum[i] = count of id i, so that ids
    1..itemnum are drawable and id 0, [MASK] = itemnum + 1 and the vocabulary tail never are; total = cum[-1]; the sorted, de-duplicated
    train | val | test items of every user as CSR (int64 offsets, int32 ids).  Refused with an AdtError: a sample size outside
    1..EVALCAND_MAX_S, counts that sum to 2^32 or more (the stream maps 32 hash bits onto [0, total)), and a user with fewer than
    sample_size drawable unseen items (the reference's rejection loop would spin forever; the kernel would fill id 0)."""
    from .. import ops
    from .._lib import AdtError
    S = int(sample_size)
    if not 1 <= S <= ops.EVALCAND_MAX_S:
        raise AdtError("DeviceBertData: sample_size=%d outside 1..%d" % (S, ops.EVALCAND_MAX_S))
    acts = [np.asarray(items, np.int64) for d in (train, val, test) for items in d.values() if len(items)]
    acts = np.concatenate(acts) if acts else np.zeros(0, np.int64)
    if acts.size and (acts.min() < 1 or acts.max() > itemnum):
        raise AdtError("DeviceBertData: item ids must lie in [1, %d]" % itemnum)
    count = np.bincount(acts, minlength=itemnum + 1)
    cum = np.zeros(itemnum + 2, np.int64)
    np.cumsum(count, out=cum[1:])
    total = int(cum[-1])
    if not 1 <= total < 2 ** 32:
        raise AdtError("DeviceBertData: the item counts sum to %d, outside 1 .. 2^32 - 1" % total)
    seen = [np.unique(np.asarray(list(train.get(u, [])) + list(val.get(u, [])) + list(test.get(u, [])), np.int64)) for u in users]
    n_drawable = int((count > 0).sum())
    for u, s in zip(users, seen):      # every seen id has a non-zero count: it is one of the counted actions
        if n_drawable - len(s) < S:
            raise AdtError("DeviceBertData: user %d has %d drawable items, sample_size is %d" % (u, n_drawable - len(s), S))
    seen_off = np.zeros(len(seen) + 1, np.int64)
    np.cumsum([len(s) for s in seen], out=seen_off[1:])
    seen_items = np.zeros(max(int(seen_off[-1]), 1), np.int32)      # never empty: the kernel takes its address
    if seen_off[-1]:
        seen_items[:seen_off[-1]] = np.concatenate(seen)
    return cum, total, seen_off, seen_items


class BertTrainDataset:
    def __init__(self, user_train, usernum, itemnum, maxlen, mask_prob, seed, dupe_factor=10, prop_sliding_window=0.5):
        self.itemnum, self.maxlen, self.mask_prob = itemnum, maxlen, mask_prob
        self.mask_token = itemnum + 1
        self.rng = random.Random(seed)
        self.dupe_factor, self.prop_sliding_window = dupe_factor, prop_sliding_window
        src, dec, lab = [], [], []
        for user in range(1, usernum + 1):
            seqs = user_train.get(user, [])
            if len(seqs) < 1:
                continue
            if len(seqs) <= maxlen:
                windows = [seqs]
            else:       # dataset.py:84-94
                step = int(prop_sliding_window * maxlen) if prop_sliding_window != -1 else maxlen
                beg = list(range(len(seqs) - maxlen, 0, -step)) + [0]
                windows = [seqs[i:i + maxlen] for i in beg[::-1]]
            for wdw in windows:
                for _ in range(dupe_factor):
                    t, d, l = self.sample_data(wdw)
                    src.append(t), dec.append(d), lab.append(l)
            t, d, l = self._mask_last(seqs)
            src.append(t), dec.append(d), lab.append(l)
        self.src, self.dec, self.labels = (np.array(x, np.int32) for x in (src, dec, lab))

    def _pad(self, x):
        x = x[-self.maxlen:]
        return [0] * (self.maxlen - len(x)) + x

    def _mask_last(self, seq):
        """dataset.py:100-123."""
        tokens, labels = list(seq), [0] * len(seq)
        labels[-1] = seq[-1]
        tokens[-1] = self.mask_token
        return self._pad(tokens), self._pad(list(tokens)), self._pad(labels)

    def sample_data(self, seq):
        """dataset.py:125-156."""
        tokens, dec_tokens, labels = [], [], []
        for s in seq:
            prob = self.rng.random()
            if prob < self.mask_prob:
                prob /= self.mask_prob
                if prob < 0.8:
                    tok = self.mask_token
                elif prob < 0.9:
                    tok = self.rng.randint(1, self.itemnum)
                else:
                    tok = s
                tokens.append(tok), dec_tokens.append(tok), labels.append(s)
            else:
                tokens.append(s), dec_tokens.append(s), labels.append(0)
        dec_tokens[-1] = self.mask_token
        return self._pad(tokens), self._pad(dec_tokens), self._pad(labels)

    def __len__(self):
        return len(self.src)

    def epoch_batches(self, batch_size, rng, shuffle=True):
        order = rng.permutation(len(self)) if shuffle else np.arange(len(self))
        for s in range(0, len(order), batch_size):
            idx = order[s:s + batch_size]
            yield self.src[idx], self.dec[idx], self.labels[idx]


class DeviceBertData:
    """BertTrainDataset's examples and BertEvalDataset's rows built on the GPU (adt_bertbatch_build / adt_bertbatch_eval; DESIGN.md section
    16).  Resident on the device, uploaded once: the training sequences as CSR over the U users with a non-empty sequence, in user order,
    and the table of the W sliding windows BertTrainDataset cuts (offset into the items, length).  Examples are numbered, not stored:
    with D = dupe_factor, example e < W * D is random copy e % D of window e // D and example W * D + u is the mask-last example of the
    u-th user, so len(self) == len(BertTrainDataset(...)).  The masks are a function of (seed, salt, example, position): one salt keeps
    one mask per example for a whole run (the reference's dupe_factor copies), salt = epoch draws a fresh set every epoch.  Per evaluation
    mode (add_eval) the user list and the (N, 1 + C) candidate table stay resident too: the host sampler's frozen candidates, or, with
    candidates="device", a table that draw_eval fills on the GPU from the resident popularity table and seen rows."""

    def __init__(self, user_train, usernum, itemnum, maxlen, mask_prob, device, dupe_factor=10, prop_sliding_window=0.5):
        import torch
        from .. import ops
        self.itemnum, self.maxlen, self.dupe_factor, self.dev = int(itemnum), int(maxlen), int(dupe_factor), torch.device(device)
        assert self.dupe_factor >= 1 and self.maxlen >= 1 and self.itemnum >= 1, (dupe_factor, maxlen, itemnum)
        self.thr_mask = ops.bertbatch_threshold(mask_prob)
        L = self.maxlen
        step = int(prop_sliding_window * L) if prop_sliding_window != -1 else L
        self.user_index, lens, items, win_start, win_len = {}, [], [], [], []
        at = 0
        for user in range(1, usernum + 1):
            seqs = user_train.get(user, [])
            n = len(seqs)
            if n < 1:
                continue
            self.user_index[user] = len(lens)
            lens.append(n)
            items.append(np.asarray(seqs, np.int32))
            if n <= L:
                win_start.append(at), win_len.append(n)
            else:       # BertTrainDataset.__init__: windows of maxlen items, the last one flush with the end
                for b in (list(range(n - L, 0, -step)) + [0])[::-1]:
                    win_start.append(at + b), win_len.append(L)
            at += n
        self.U, self.W = len(lens), len(win_start)
        seq_off = np.zeros(self.U + 1, np.int64)
        np.cumsum(lens, out=seq_off[1:])
        seq_items = np.concatenate(items) if items else np.zeros(0, np.int32)
        assert seq_items.size == 0 or (seq_items.min() >= 1 and seq_items.max() <= self.itemnum), "item ids must lie in [1, itemnum]"
        assert self.W * self.dupe_factor + self.U < 2 ** 31, "more than 2^31 examples"
        self.seq_off, self.seq_items = torch.from_numpy(seq_off).to(self.dev), torch.from_numpy(seq_items).to(self.dev)
        self.win_start = torch.from_numpy(np.asarray(win_start, np.int64)).to(self.dev)
        self.win_len = torch.from_numpy(np.asarray(win_len, np.int32)).to(self.dev)
        self.order = None
        self._eval = {}
        self._draw = {}       # mode -> the tables draw_eval reads (add_eval(candidates="device") only)

    def __len__(self):
        return self.W * self.dupe_factor + self.U

    def set_order(self, order):
        """Upload one epoch's permutation of example ids (the only host -> device copy of an epoch)."""
        import torch
        from .._lib import AdtError
        order = np.ascontiguousarray(order, dtype=np.int64)
        if order.ndim != 1 or (order.size and (order.min() < 0 or order.max() >= len(self))):
            raise AdtError("DeviceBertData.set_order: an example id outside 0..%d" % (len(self) - 1))
        self.order = torch.from_numpy(order.astype(np.int32)).to(self.dev)

    def train_stage(self, start, B, seed, salt, rows=None):
        """The dict of BertModel.stage for examples order[start:start + B], built on the device (no M_host: the count is not read back) --
        under data parallelism rows (lo, hi) of that global batch, with local `rows` indices, the global inv_count and the masks the whole
        batch would get."""
        from .. import ops
        assert self.order is not None and 0 <= start and start + B <= self.order.numel(), "set_order first; the batch must lie inside it"
        lo, hi = (0, B) if rows is None else rows
        src, dec, _, rows_c, labels_c, M, inv_count = ops.bertbatch_build(
            self.seq_off, self.seq_items, self.win_start, self.win_len, self.order[start:start + B], self.maxlen, self.dupe_factor, self.itemnum,
            self.thr_mask, seed, salt, (lo, hi), want_labels=False)
        return {"B": hi - lo, "B_global": B, "src": src, "dec": dec, "rows": rows_c, "labels": labels_c, "M": M, "inv_count": inv_count}

    def add_eval(self, eval_ds, candidates="host"):
        """Keep a BertEvalDataset's user list and its (N, 1 + C) candidate matrix resident, under eval_ds.mode.  candidates="host": the
        positive, then the sampler's negatives, which it freezes per (user, mode).  candidates="device" (DESIGN.md section 28): the host
        sampler is not called; the targets, the seen rows and the popularity table of device_candidate_tables stay resident beside a
        candidate table that holds the targets only until draw_eval fills it."""
        import torch
        from .._lib import AdtError
        if candidates not in ("host", "device"):
            raise AdtError("DeviceBertData.add_eval: candidates=%r (host or device)" % (candidates,))
        mode = eval_ds.mode
        users = torch.from_numpy(np.array([self.user_index[u] for u in eval_ds.users], np.int32)).to(self.dev)
        self._draw.pop(mode, None)
        if candidates == "host":
            cand = np.array([eval_ds.sample_data(u)[1] for u in eval_ds.users], np.int32).reshape(len(eval_ds.users), -1)
            self._eval[mode] = (users, torch.from_numpy(cand).to(self.dev))
            return
        sp = eval_ds.sampler
        S = int(sp.sample_size)
        cum, total, seen_off, seen_items = device_candidate_tables(sp.train, sp.val, sp.test, self.itemnum, eval_ds.users, S)
        tgt = eval_ds.user_val if mode == "val" else eval_ds.user_test
        targets = torch.from_numpy(np.array([tgt[u][0] for u in eval_ds.users], np.int32)).to(self.dev)
        cand = torch.zeros(len(eval_ds.users), 1 + S, device=self.dev, dtype=torch.int32)
        cand[:, 0] = targets
        self._eval[mode] = (users, cand)
        self._draw[mode] = {"cum": torch.from_numpy(cum).to(self.dev), "total": total, "seen_off": torch.from_numpy(seen_off).to(self.dev),
                            "seen_items": torch.from_numpy(seen_items).to(self.dev), "targets": targets, "S": S, "drawn": False}

    def draw_eval(self, mode, seed, salt=0):
        """Fill the mode's resident (N, 1 + S) candidate table with adt_evalcand_draw: column 0 the target, then the first S distinct
        unseen values of the popularity stream of (seed, salt, row) -- PopularSampler's distribution over a hash stream of its own, not
        numpy's.  Returns the table."""
        from .. import ops
        from .._lib import AdtError
        if mode not in self._draw:
            raise AdtError("DeviceBertData.draw_eval: mode %r was not added with add_eval(candidates=\"device\")" % (mode,))
        t, cand = self._draw[mode], self._eval[mode][1]
        if cand.shape[0]:
            ops.evalcand_draw(t["cum"], t["total"], t["seen_off"], t["seen_items"], t["targets"], t["S"], seed, salt, out=cand)
        t["drawn"] = True
        return cand

    def eval_len(self, mode):
        return self._eval[mode][0].numel()

    def eval_batch(self, mode, start, B):
        """(seq (B, L), candidates (B, 1 + C)), both device int32, of users start .. start + B - 1 of the mode's list: what
        BertEvalDataset.batches yields, for FusedBertTrainer.evaluate."""
        from .. import ops
        from .._lib import AdtError
        users, cand = self._eval[mode]
        if mode in self._draw and not self._draw[mode]["drawn"]:
            raise AdtError("DeviceBertData.eval_batch: mode %r has no candidates yet (draw_eval first)" % (mode,))
        assert 0 <= start and start + B <= users.numel(), (mode, start, B, users.numel())
        return ops.bertbatch_eval(self.seq_off, self.seq_items, users[start:start + B], self.maxlen, self.itemnum), cand[start:start + B]

    def eval_batches(self, mode, batch_size):
        n = self.eval_len(mode)
        return (self.eval_batch(mode, s, min(batch_size, n - s)) for s in range(0, n, batch_size))


class BertEvalDataset:
    def __init__(self, user_train, user_val, user_test, usernum, itemnum, maxlen, negative_sampler, mode="val", eval_set=-1):
        self.user_train, self.user_val, self.user_test = user_train, user_val, user_test
        self.maxlen, self.sampler, self.mode, self.mask_token = maxlen, negative_sampler, mode, itemnum + 1
        pool = random.sample(range(1, usernum + 1), eval_set) if eval_set >= 0 else range(1, usernum + 1)
        tgt = user_val if mode == "val" else user_test
        self.users = [u for u in pool if len(tgt.get(u, [])) != 0 and len(user_train.get(u, [])) != 0]

    def sample_data(self, user):
        """dataset.py:201-215."""
        answer = [(self.user_val if self.mode == "val" else self.user_test)[user][0]]
        cand = answer + self.sampler.get_negative_samples(user, mode=self.mode)
        return self.sequence(user), cand

    def sequence(self, user):
        """The left-padded history with the [MASK] token appended, as fed to the model."""
        seq = (list(self.user_train[user]) + [self.mask_token])[-self.maxlen:]
        return [0] * (self.maxlen - len(seq)) + seq

    def __len__(self):
        return len(self.users)

    def batches(self, batch_size):
        for s in range(0, len(self.users), batch_size):
            rows = [self.sample_data(u) for u in self.users[s:s + batch_size]]
            yield np.array([r[0] for r in rows], np.int32), np.array([r[1] for r in rows], np.int32)
