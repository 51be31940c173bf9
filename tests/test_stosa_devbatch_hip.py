"""GPU: STOSA-ADT batches built on the device (adt_seqbatch_build; adt_amd/stosa/datasets.py:DeviceDisenData) against the host
pipeline they stand in for (DisenDataset.batch), a Python replay of the negative-sampling rule, and the trainer / full-sort / CLI
paths fed from them.  Integer outputs are compared bit for bit; the trainer bounds are those of tests/test_stosa_hip.py for two runs
of one step sequence (the staged tensors are bit-identical, only the order of float atomics differs)."""
import json

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from adt_amd import _lib, ops  # noqa: E402
from adt_amd.stosa.datasets import DeviceDisenData, DisenDataset, rating_matrix  # noqa: E402
from oracle import stosa_oracle as so  # noqa: E402

DEV = "cuda:0"
CUT = {"train": 3, "valid": 2, "test": 1}
MAX_REJECTS = 32


class Args:
    pass


def lengths(L):
    return [1, 2, 3, 4, 5, 6, L - 1, L, L + 1, L + 3, L + 4, 2 * L + 7]


def make_seqs(lens, item_size, seed):
    r = np.random.RandomState(seed)
    return [[int(x) for x in r.randint(1, item_size, size=n)] for n in lens]


def device_data(user_seq, item_size, L):
    n = len(user_seq)
    return DeviceDisenData(user_seq, item_size, L, DEV, rating_matrix(user_seq, n, item_size, 2), rating_matrix(user_seq, n, item_size, 1))


def host_batch(user_seq, item_size, L, data_type, users):
    """DisenDataset.batch row by row.  It cannot form the answer of a sequence shorter than the hold-out (IndexError on items[-2] of a
    one-item sequence in the valid view); there the expected row is the view table's slices themselves and the answer is 0."""
    a = Args()
    a.maxlen, a.item_size = L, item_size
    ds = DisenDataset(a, user_seq, data_type)
    cut = CUT[data_type]
    inp, dec, pos = (np.zeros((len(users), L), np.int32) for _ in range(3))
    ans = np.zeros((len(users), 1), np.int64)
    for r, u in enumerate(users):
        try:
            _, i1, d1, p1, _, a1 = ds.batch([u])
            inp[r], dec[r], pos[r], ans[r] = i1[0], d1[0], p1[0], a1[0]
        except IndexError:
            s = user_seq[u]
            for out, view in ((inp, s[:-cut]), (pos, s[1:len(s) - cut + 1]), (dec, s[:-cut - 1])):
                view = view[-L:]
                if view:
                    out[r, L - len(view):] = view
    return inp, dec, pos, ans


def build_direct(dd, users, cut, seed=0, step=0, rows=None, **kw):
    u = torch.tensor(users, dtype=torch.int32, device=DEV)
    out = ops.seqbatch_build(dd.seq_off, dd.seq_items, dd.set_off, dd.set_items, u, dd.max_len, cut, dd.item_size, seed, step, rows, **kw)
    return [None if t is None else t.cpu().numpy() for t in out]


def replay_neg(user_seq, users, pos, item_size, seed, step, row0=0):
    """The rule of adt_seqbatch.cuh in Python: attempts 0..31 of ops.seqbatch_draw, then the cyclic upward walk from the last proposal,
    0 when nothing is free.  Returns (neg, number of positions that reached the walk)."""
    neg, walked, top = np.zeros_like(pos), 0, item_size - 1
    for r, u in enumerate(users):
        own = set(user_seq[u])
        for t in range(pos.shape[1]):
            if pos[r, t] == 0:
                continue
            for a in range(MAX_REJECTS):
                c = ops.seqbatch_draw(seed, step, row0 + r, t, a, item_size)
                if c not in own:
                    break
            else:
                walked += 1
                x, c = c, 0
                for _ in range(top):
                    x = 1 if x == top else x + 1
                    if x not in own:
                        c = x
                        break
            neg[r, t] = c
    return neg, walked


# ---- layout ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("data_type", ["train", "valid", "test"])
@pytest.mark.parametrize("L", [8, 50])
def test_views_match_host_dataset(L, data_type):
    item_size = 40
    user_seq = make_seqs(lengths(L), item_size, 3)
    dd = device_data(user_seq, item_size, L)
    n = len(user_seq)
    users = [int(x) for x in np.random.RandomState(5).permutation(n)] + [7, 0, 7, 11, 11]       # shuffled, with repeats
    want_inp, want_dec, want_pos, _ = host_batch(user_seq, item_size, L, data_type, users)
    inp, dec, pos, neg, inv = build_direct(dd, users, CUT[data_type], seed=21, step=4)
    assert inp.dtype == np.int32 and inp.shape == (len(users), L)
    assert np.array_equal(inp, want_inp) and np.array_equal(dec, want_dec) and np.array_equal(pos, want_pos)
    assert np.array_equal(neg == 0, pos == 0)
    assert inv[0] == np.float32(1.0 / max(int((want_pos != 0).sum()), 1))
    # the dataset's own entry points: contiguous users for evaluation, the uploaded order for training
    if data_type == "train":
        dd.set_order(users)
        st = dd.train_stage(2, 9, 21, 4)
        w = host_batch(user_seq, item_size, L, "train", users[2:11])
        assert st["B"] == 9 and all(np.array_equal(st[k].cpu().numpy(), x) for k, x in zip(("inp", "dec", "pos"), w))
    else:
        for start, B in ((0, n), (3, 5), (n - 1, 1)):
            e_inp, (indptr, indices), ans = dd.eval_batch(data_type, start, B)
            w = host_batch(user_seq, item_size, L, data_type, list(range(start, start + B)))
            assert np.array_equal(e_inp.cpu().numpy(), w[0]) and np.array_equal(ans, w[3]) and ans.dtype == np.int64
            rows = rating_matrix(user_seq, n, item_size, CUT[data_type])[list(range(start, start + B))]
            assert np.array_equal(indptr.cpu().numpy(), rows.indptr) and np.array_equal(indices.cpu().numpy(), rows.indices)


# ---- negatives -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("item_size", [40, 12103])
def test_negatives_replay(item_size):
    L = 50
    user_seq = make_seqs(lengths(L), item_size, 8)
    dd = device_data(user_seq, item_size, L)
    users = [int(x) for x in np.random.RandomState(6).permutation(len(user_seq))] + [11, 3, 11]
    for cut in (3, 1):
        inp, dec, pos, neg, _ = build_direct(dd, users, cut, seed=77, step=123456)
        for r, u in enumerate(users):
            nz = neg[r][neg[r] != 0]
            assert ((nz >= 1) & (nz <= item_size - 1)).all() and not (set(nz.tolist()) & set(user_seq[u]))
        want, _ = replay_neg(user_seq, users, pos, item_size, 77, 123456)
        assert np.array_equal(neg, want)


def test_guard_walk_and_full_set():
    """A user owning 63 of the 64 ids of item_size 65: every negative is the free id, and the replay shows that the bounded walk -- not
    the rejection loop -- found it for some positions.  A user owning all 64: the call returns and every negative is 0."""
    item_size, L, free = 65, 16, 23
    r = np.random.RandomState(9)
    almost = [int(x) for x in r.permutation([i for i in range(1, item_size) if i != free])]
    full = [int(x) for x in r.permutation(np.arange(1, item_size))]
    user_seq = [almost, full]
    dd = device_data(user_seq, item_size, L)
    inp, dec, pos, neg, _ = build_direct(dd, [0, 1, 0], 3, seed=5, step=2)
    assert (pos != 0).all()
    assert (neg[0] == free).all() and (neg[2] == free).all() and (neg[1] == 0).all()
    want, walked = replay_neg(user_seq, [0, 1, 0], pos, item_size, 5, 2)
    assert np.array_equal(neg, want)
    _, walked_almost = replay_neg(user_seq, [0], pos[:1], item_size, 5, 2)
    assert walked_almost >= 1 and walked >= walked_almost + L


# ---- sharding and determinism --------------------------------------------------------------------------------------------------------
def test_shards_are_slices_of_the_whole():
    item_size, L = 40, 8
    user_seq = make_seqs(lengths(L), item_size, 4)
    dd = device_data(user_seq, item_size, L)
    dd.set_order(np.random.RandomState(2).permutation(12))
    whole = dd.train_stage(0, 12, 31, 7)
    count = int((whole["pos"] != 0).sum())
    assert whole["B"] == 12 and whole["inv_count"].cpu().numpy()[0] == np.float32(1.0 / count)
    for lo, hi in ((0, 5), (5, 12), (0, 12)):
        st = dd.train_stage(0, 12, 31, 7, rows=(lo, hi))
        assert st["B"] == hi - lo and st["B_global"] == 12
        for k in ("inp", "dec", "pos", "neg"):
            assert torch.equal(st[k], whole[k][lo:hi]), (k, lo, hi)
        assert torch.equal(st["inv_count"], whole["inv_count"])


def test_same_seed_and_step_repeat_and_the_step_moves_only_the_negatives():
    item_size, L = 12103, 50
    user_seq = make_seqs(lengths(L), item_size, 4)
    dd = device_data(user_seq, item_size, L)
    dd.set_order(np.arange(12))
    a, b, c = dd.train_stage(0, 12, 31, 7), dd.train_stage(0, 12, 31, 7), dd.train_stage(0, 12, 31, 8)
    for k in ("inp", "dec", "pos", "neg", "inv_count"):
        assert torch.equal(a[k], b[k]), k
    for k in ("inp", "dec", "pos", "inv_count"):
        assert torch.equal(a[k], c[k]), k
    live = a["pos"] != 0
    assert (a["neg"][live] != c["neg"][live]).float().mean() > 0.9


def test_argument_checks():
    dd = device_data(make_seqs([5, 6], 40, 1), 40, 8)
    users = torch.tensor([0, 1], dtype=torch.int32, device=DEV)

    def call(L=8, cut=3, item_size=40, rows=None):
        return ops.seqbatch_build(dd.seq_off, dd.seq_items, dd.set_off, dd.set_items, users, L, cut, item_size, rows=rows)
    for bad in (dict(cut=0), dict(cut=4), dict(L=0), dict(item_size=1), dict(rows=(1, 3))):
        with pytest.raises(_lib.AdtError):
            call(**bad)
    inp, dec, pos, neg, inv = ops.seqbatch_build(dd.seq_off, dd.seq_items, dd.set_off, dd.set_items, users, 8, 1, 40, want_neg=False,
                                                 want_inv_count=False, views=False)
    assert dec is None and pos is None and neg is None and inv is None and inp.shape == (2, 8)


# ---- trainer ---------------------------------------------------------------------------------------------------------------------------
def stosa_model(item_size, L, num_users, seed):
    from adt_amd.stosa.models import DisenDistSAModel
    cfg = so.Cfg(item_size, L, 64, 4, 1, num_users=num_users, pvn_weight=0.005)
    a = Args()
    a.device, a.item_size, a.maxlen, a.hidden_units, a.num_heads, a.num_layers, a.num_users = DEV, item_size, L, 64, 4, 1, num_users
    a.dropout, a.attention_dropout, a.pvn_weight, a.precision, a.distance_metric = 0.0, 0.0, 0.005, "bf16", "wasserstein"
    m = DisenDistSAModel(a)
    m.load_numpy(so.init_params(cfg, seed))
    return m


@pytest.mark.parametrize("use_graph", [False, True])
def test_step_device_matches_step_on_the_same_arrays(use_graph):
    from adt_amd.stosa.trainer import FusedStosaTrainer
    item_size, L, B = 42, 16, 8
    r = np.random.RandomState(12)
    user_seq = make_seqs([int(x) for x in r.randint(4, 31, size=24)], item_size, 13)
    dd = device_data(user_seq, item_size, L)
    dd.set_order(r.permutation(24))
    stages = [dd.train_stage(B * i, B, 9, i) for i in range(3)]
    outs = []
    for device in (True, False):
        m = stosa_model(item_size, L, 24, 2)
        tr = FusedStosaTrainer(m, [0.2], [0.1], use_graph=use_graph, seed=5)
        for st in stages:
            if device:
                tr.step_device(st)
            else:
                tr.step(*(st[k].cpu().numpy() for k in ("inp", "dec", "pos", "neg")))
        torch.cuda.synchronize()
        outs.append((float(tr.loss()), m.flat.cpu().numpy().copy()))
    (loss_d, flat_d), (loss_h, flat_h) = outs
    print("loss %r vs %r; flat rel %g" % (loss_d, loss_h, np.abs(flat_d - flat_h).max() / np.abs(flat_h).max()))
    assert np.isfinite(loss_h) and abs(loss_d - loss_h) < 1e-4 * abs(loss_h)
    assert np.abs(flat_d.astype(np.float64) - flat_h).max() / max(np.abs(flat_h).max(), 1e-6) < 5e-3


# ---- evaluation ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def eval_case():
    from adt_amd.stosa.trainer import FusedStosaTrainer
    item_size, L, n = 62, 16, 40                 # items 1..60, as stosa/datasets.py:get_user_seqs sizes it (max_item + 2)
    r = np.random.RandomState(20)
    user_seq = [[int(x) for x in r.randint(1, 61, size=k)] for k in r.randint(3, 26, size=n)]
    dd = device_data(user_seq, item_size, L)
    tr = FusedStosaTrainer(stosa_model(item_size, L, n, 3), [0.2], [0.1])
    return user_seq, item_size, L, dd, tr


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("split", ["valid", "test"])
def test_full_sort_over_eval_batches(eval_case, split, fused):
    user_seq, item_size, L, dd, tr = eval_case
    n, bs = len(user_seq), 16
    a = Args()
    a.maxlen, a.item_size = L, item_size
    ds = DisenDataset(a, user_seq, split)
    matrix = rating_matrix(user_seq, n, item_size, CUT[split])
    host = [(inp, matrix[users], ans) for users, inp, _, _, _, ans in ds.epoch_batches(bs, shuffle=False)]
    dev = [dd.eval_batch(split, s, min(bs, n - s)) for s in range(0, n, bs)]
    assert all(b[0].is_cuda and b[1][0].is_cuda and b[1][1].is_cuda for b in dev)
    want_pred, want_ans = tr.full_sort(host, fused=fused)
    pred, ans = tr.full_sort(dev, fused=fused)
    assert pred.shape == (n, 40) and np.array_equal(pred, want_pred) and np.array_equal(ans, want_ans)


# ---- command line ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra", [[], ["--fused_eval"]])
def test_cli_device_batches(tmp_path, capsys, extra):
    from adt_amd.stosa.main import _write_synthetic, main
    data = tmp_path / "data"
    data.mkdir()
    _write_synthetic(str(data / "Beauty.txt"), users=96, items=150, seed=3)        # --synthetic 1 keeps a file that is there
    over = {"epochs": 1, "maxlen": 20, "batch_size": 32, "eval_batch_size": 48}     # the Beauty template sets epochs and maxlen itself
    main(["--dataset", "Beauty", "--data_dir", str(data) + "/", "--output_dir", str(tmp_path / "out") + "/", "--device_batches", "--synthetic", "1",
          "--epochs", "1", "--eval_set", "64", "--override", json.dumps(over)] + extra)
    lines = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert len(lines) == 1 and lines[0]["epoch"] == 0 and lines[0]["sequences_per_sec"] > 0
    assert np.isfinite(lines[0]["valid_MRR"]) and 0.0 <= lines[0]["valid_MRR"] <= 1.0 and np.isfinite(lines[0]["rec_cur_loss"])
