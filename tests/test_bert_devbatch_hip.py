"""GPU: BERT4Rec-ADT batches masked and built on the device (adt_bertbatch_build / adt_bertbatch_eval;
adt_amd/bert4rec/datasets.py:DeviceBertData) against a Python replay of the masking rule (ops.bertbatch_token per position), the host
pipeline they stand in for (BertTrainDataset at mask_prob 0, BertModel.stage, BertEvalDataset.batches), and the trainer / evaluation /
CLI paths fed from them.  Integer outputs are compared bit for bit.  The trainer bound is the one tests/test_bert_hip.py:176-178 uses
for two runs of one step sequence (loss 1e-5, weights 5e-4 of the largest weight: the staged tensors are bit-identical, only the order
of the float atomics of the weight gradients differs)."""
import json
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from adt_amd import _lib, ops  # noqa: E402
from adt_amd.bert4rec import datasets as D  # noqa: E402
from oracle import bert_oracle as bo  # noqa: E402

DEV = "cuda:0"
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ITEMS = 60


class Args:
    pass


def make_users(L, itemnum=ITEMS, seed=3):
    """user_train over users 1..9: the lengths at which the window cut changes, and user 4 without a sequence (skipped, as by the host)."""
    r = np.random.RandomState(seed)
    lens = [1, 2, 3, 0, L - 1, L, L + 1, L + 3, 2 * L + 7]
    return {u + 1: [int(x) for x in r.randint(1, itemnum + 1, size=n)] for u, n in enumerate(lens)}, len(lens)


def cut_windows(user_train, usernum, L, prop):
    """The windows and the sequences, in example order (BertTrainDataset.__init__)."""
    wins, seqs = [], []
    for u in range(1, usernum + 1):
        s = user_train.get(u, [])
        if not s:
            continue
        seqs.append(s)
        if len(s) <= L:
            wins.append(s)
        else:
            step = int(prop * L) if prop != -1 else L
            wins += [s[i:i + L] for i in (list(range(len(s) - L, 0, -step)) + [0])[::-1]]
    return wins, seqs


def replay(user_train, usernum, itemnum, L, prop, dupe, mask_prob, seed, salt, examples):
    """The rule of adt_bertbatch.cuh in Python, one ops.bertbatch_token call per position."""
    wins, seqs = cut_windows(user_train, usernum, L, prop)
    thr, mask = ops.bertbatch_threshold(mask_prob), itemnum + 1
    src, dec, lab = (np.zeros((len(examples), L), np.int32) for _ in range(3))
    for r, e in enumerate(examples):
        if e < len(wins) * dupe:
            w = wins[e // dupe]
            out = [ops.bertbatch_token(seed, salt, e, j, thr, itemnum, it) for j, it in enumerate(w)]
            t = [tok for tok, _ in out]
            l = [it if m else 0 for it, (_, m) in zip(w, out)]
            d = t[:-1] + [mask]
        else:
            s = seqs[e - len(wins) * dupe][-L:]
            t = s[:-1] + [mask]
            d, l = list(t), [0] * (len(s) - 1) + [s[-1]]
        src[r, L - len(t):], dec[r, L - len(t):], lab[r, L - len(t):] = t, d, l
    return src, dec, lab


def build(dd, examples, seed=0, salt=0, rows=None, want_labels=True):
    ex = torch.tensor(list(examples), dtype=torch.int32, device=DEV)
    out = ops.bertbatch_build(dd.seq_off, dd.seq_items, dd.win_start, dd.win_len, ex, dd.maxlen, dd.dupe_factor, dd.itemnum, dd.thr_mask,
                              seed, salt, rows, want_labels)
    return [None if t is None else t.cpu().numpy() for t in out]


# ---- 1. replay -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask_prob", [0.2, 0.9])
@pytest.mark.parametrize("L", [7, 50, 200])
def test_all_examples_replay(L, mask_prob):
    user_train, usernum = make_users(L)
    dd = D.DeviceBertData(user_train, usernum, ITEMS, L, mask_prob, DEV, dupe_factor=3, prop_sliding_window=0.5)
    wins, seqs = cut_windows(user_train, usernum, L, 0.5)
    assert dd.W == len(wins) and dd.U == len(seqs) == 8 and len(dd) == 3 * len(wins) + 8
    examples = list(range(len(dd)))
    src, dec, lab, rows, lab_c, M, inv = build(dd, examples, seed=77, salt=4)
    want = replay(user_train, usernum, ITEMS, L, 0.5, 3, mask_prob, 77, 4, examples)
    assert src.dtype == np.int32 and src.shape == (len(dd), L)
    assert np.array_equal(src, want[0]) and np.array_equal(dec, want[1]) and np.array_equal(lab, want[2])
    nz = np.nonzero(want[2].reshape(-1))[0]
    print("L %d mask_prob %g: %d examples, %d of %d positions labelled" % (L, mask_prob, len(dd), nz.size, int((want[0] != 0).sum())))
    assert M[0] == nz.size and np.array_equal(rows[:nz.size], nz) and np.array_equal(lab_c[:nz.size], want[2].reshape(-1)[nz])
    assert not rows[nz.size:].any() and not lab_c[nz.size:].any()
    assert inv[0] == np.float32(1.0 / max(nz.size, 1))
    # another salt is another mask set over the same items; the same salt repeats
    again = build(dd, examples, seed=77, salt=4)
    other = build(dd, examples, seed=77, salt=5)
    assert all(np.array_equal(a, b) for a, b in zip(again, (src, dec, lab, rows, lab_c, M, inv)))
    assert not np.array_equal(other[2], lab) and np.array_equal(other[0] != 0, src != 0)


# ---- 2. the windows of the host dataset -------------------------------------------------------------------------------------------------
def sorted_rows(src, dec, lab):
    return sorted(tuple(int(x) for x in np.concatenate(r)) for r in zip(src, dec, lab))


@pytest.mark.parametrize("prop", [0.5, -1])
@pytest.mark.parametrize("L", [7, 50])
def test_same_examples_as_host_dataset_at_probability_zero(L, prop):
    user_train, usernum = make_users(L, seed=5)
    host = D.BertTrainDataset(user_train, usernum, ITEMS, L, 0.0, 1, dupe_factor=1, prop_sliding_window=prop)
    dd = D.DeviceBertData(user_train, usernum, ITEMS, L, 0.0, DEV, dupe_factor=1, prop_sliding_window=prop)
    assert len(dd) == len(host)
    src, dec, lab = build(dd, range(len(dd)), seed=9)[:3]
    assert sorted_rows(src, dec, lab) == sorted_rows(host.src, host.dec, host.labels)


# ---- 3. compaction = BertModel.stage ---------------------------------------------------------------------------------------------------
def load_small():
    g = np.load(os.path.join(GOLD, "bert_small.npz"))
    V, L, d, H, nl, inner = [int(x) for x in g["cfg"]]
    cfg = bo.Cfg(V, L, d, H, nl, inner)
    return g, cfg, bo.init_params(cfg, int(g["seed"]))


def small_model(cfg, P, dropout=0.0, attention_dropout=0.0):
    from adt_amd.bert4rec.model import BertModel
    a = Args()
    a.device, a.maxlen, a.num_heads, a.num_layers, a.hidden_units, a.inner_units = DEV, cfg.maxlen, cfg.num_heads, cfg.num_layers, cfg.hidden_units, cfg.inner_units
    a.dropout, a.attention_dropout, a.type_vocab_size, a.precision = dropout, attention_dropout, 2, "bf16"
    m = BertModel(1, cfg.item_num, a)
    m.load_numpy(P)
    return m


@pytest.fixture(scope="module")
def model():
    _, cfg, P = load_small()
    return small_model(cfg, P)


def assert_stage_equal(model, st, src, dec, lab, n_valid_global=None):
    want = model.stage(src, dec, lab, n_valid_global)
    assert st["B"] == want["B"]
    for k in ("src", "dec", "rows", "labels", "M", "inv_count"):
        assert st[k].dtype == want[k].dtype and torch.equal(st[k], want[k]), k
    return want["M_host"]


@pytest.mark.parametrize("case", ["masked", "rows_without_label", "no_label"])
def test_stage_equals_host_stage(model, case):
    L, B = 50, 300
    user_train, usernum = make_users(L, seed=7)
    dd = D.DeviceBertData(user_train, usernum, ITEMS, L, 0.2 if case == "masked" else 0.0, DEV, dupe_factor=3, prop_sliding_window=0.5)
    n_random = dd.W * dd.dupe_factor
    r = np.random.RandomState(17)
    order = r.randint(0, n_random if case == "no_label" else len(dd), size=B + 20)      # with repeats: B exceeds the example count
    dd.set_order(order)
    whole = dd.train_stage(10, B, 31, 2)
    src, dec, lab = build(dd, order[10:10 + B], seed=31, salt=2)[:3]
    assert "M_host" not in whole and whole["B_global"] == B
    total = assert_stage_equal(model, whole, src, dec, lab)
    assert total == int((lab != 0).sum())
    if case == "masked":
        assert total > B
    elif case == "rows_without_label":       # a mask-last row has one label, a random row at probability 0 has none
        assert 0 < total < B and total == int((order[10:10 + B] >= n_random).sum())
    else:
        assert total == 0 and whole["M"].item() == 0 and whole["inv_count"].item() == 1.0
    for lo, hi in ((0, 100), (100, 300), (299, 300)):
        st = dd.train_stage(10, B, 31, 2, rows=(lo, hi))
        assert st["B"] == hi - lo and st["B_global"] == B
        assert_stage_equal(model, st, src[lo:hi], dec[lo:hi], lab[lo:hi], n_valid_global=total)
        assert torch.equal(st["inv_count"], whole["inv_count"])


# ---- 5. trainer ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_graph", [False, True])
def test_step_device_matches_step_on_the_same_arrays(use_graph):
    from adt_amd.bert4rec.trainer import FusedBertTrainer
    _, cfg, P = load_small()
    L, B = cfg.maxlen, 4
    user_train, usernum = make_users(L, itemnum=cfg.item_num, seed=12)
    dd = D.DeviceBertData(user_train, usernum, cfg.item_num, L, 0.3, DEV, dupe_factor=2, prop_sliding_window=0.5)
    order = np.random.RandomState(2).permutation(len(dd))
    dd.set_order(order)
    outs = []
    for device in (True, False):
        m = small_model(cfg, P, 0.3, 0.2)
        tr = FusedBertTrainer(m, [0.3, 0.2], [0.2, 0.1], weight_decay=1e-4, use_graph=use_graph, seed=5)
        for i in range(2):
            st = dd.train_stage(B * i, B, 9, 1)
            src, dec, lab = build(dd, order[B * i:B * (i + 1)], seed=9, salt=1)[:3]
            assert np.array_equal(st["src"].cpu().numpy(), src)
            if device:
                tr.step_device(st)
            else:
                tr.step(src, dec, lab)
        torch.cuda.synchronize()
        outs.append((float(tr.loss()), m.flat.cpu().numpy().astype(np.float64)))
    (loss_d, flat_d), (loss_h, flat_h) = outs
    rel = np.abs(flat_d - flat_h).max() / max(np.abs(flat_h).max(), 1e-6)
    print("loss %r vs %r; flat rel %g" % (loss_d, loss_h, rel))
    assert np.isfinite(loss_h) and abs(loss_d - loss_h) < 1e-5 * abs(loss_h)      # tests/test_bert_hip.py:176
    assert rel < 5e-4                                                               # tests/test_bert_hip.py:178


def test_step_device_needs_full_capacity(model):
    from adt_amd.bert4rec.trainer import FusedBertTrainer
    L = model.maxlen
    user_train, usernum = make_users(L, itemnum=model.itemnum, seed=12)
    dd = D.DeviceBertData(user_train, usernum, model.itemnum, L, 0.3, DEV, dupe_factor=2)
    dd.set_order(np.arange(len(dd)))
    tr = FusedBertTrainer(model, [0.3, 0.2], [0.2, 0.1], mcap_frac=0.5)
    with pytest.raises(_lib.AdtError):
        tr.step_device(dd.train_stage(0, 4, 1, 0))


# ---- 6. evaluation ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["val", "test"])
def test_eval_batches_match_host_dataset(model, mode):
    from adt_amd.bert4rec.trainer import FusedBertTrainer
    L, itemnum, usernum, bs = model.maxlen, model.itemnum, 23, 6      # 20 users qualify: three batches of 6 and one of 2
    r = np.random.RandomState(20)
    train, val, test = {}, {}, {}
    for u in range(1, usernum + 1):      # data_partition's split, then main.py's merge of the validation item into the training sequence
        items = [int(x) for x in r.permutation(itemnum)[:r.randint(1, 2 * L)] + 1]
        if u == 6:
            items = []
        if len(items) < 3:
            train[u], val[u], test[u] = items, [], []
        else:
            train[u], val[u], test[u] = items[:-1], [items[-2]], [items[-1]]
    sampler = D.PopularSampler(train, val, test, usernum, itemnum, 8)
    ds = D.BertEvalDataset(train, val, test, usernum, itemnum, L, sampler, mode)
    dd = D.DeviceBertData(train, usernum, itemnum, L, 0.2, DEV)
    dd.add_eval(ds)
    n = len(ds)
    assert n == dd.eval_len(mode) and n % bs != 0 and n > 2 * bs
    host = list(ds.batches(bs))
    dev = [dd.eval_batch(mode, s, min(bs, n - s)) for s in range(0, n, bs)]
    assert len(host) == len(dev) == len(list(dd.eval_batches(mode, bs)))
    for (h_seq, h_cand), (d_seq, d_cand) in zip(host, dev):
        assert d_seq.is_cuda and d_cand.is_cuda and d_seq.dtype == torch.int32 and d_cand.dtype == torch.int32
        assert np.array_equal(d_seq.cpu().numpy(), h_seq) and np.array_equal(d_cand.cpu().numpy(), h_cand)
    users = torch.tensor([dd.user_index[u] for u in ds.users], dtype=torch.int32, device=DEV)
    assert np.array_equal(ops.bertbatch_eval(dd.seq_off, dd.seq_items, users, L, itemnum).cpu().numpy(), np.array([ds.sequence(u) for u in ds.users]))
    tr = FusedBertTrainer(model, [0.3, 0.2], [0.2, 0.1])
    assert tr.evaluate(dev) == tr.evaluate(host)


# ---- 7. command line -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra", [[], ["--remask_every_epoch"]])
def test_cli_device_batches(tmp_path, capsys, extra):
    from adt_amd.bert4rec.main import main
    main(["--dataset", "ml-1m", "--data_dir", str(tmp_path), "--synthetic", "tiny", "--template", "0", "--device_batches", "--num_epochs", "1",
          "--maxlen", "16", "--batch_size", "32", "--eval_batch_size", "24", "--eval_negative_sample_size", "10", "--dupe_factor", "2",
          "--prop_sliding_window", "0.5", "--hidden_units", "64", "--inner_units", "96"] + extra)
    lines = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert len(lines) == 1 and lines[0]["epoch"] == 1 and lines[0]["sequences_per_sec"] > 0
    assert np.isfinite(lines[0]["loss"]) and 0.0 <= lines[0]["valid"]["auc"] <= 1.0


# ---- 8. argument errors ----------------------------------------------------------------------------------------------------------------
def test_argument_checks():
    user_train, usernum = make_users(8)
    dd = D.DeviceBertData(user_train, usernum, ITEMS, 8, 0.2, DEV, dupe_factor=2)
    ex = torch.tensor([0, 1, 2], dtype=torch.int32, device=DEV)

    def call(L=8, dupe=2, itemnum=ITEMS, rows=None):
        return ops.bertbatch_build(dd.seq_off, dd.seq_items, dd.win_start, dd.win_len, ex, L, dupe, itemnum, dd.thr_mask, rows=rows)
    for bad in (dict(L=0), dict(itemnum=0), dict(dupe=0), dict(rows=(1, 4)), dict(rows=(2, 1))):
        with pytest.raises(_lib.AdtError):
            call(**bad)
    lib = _lib.load()
    z = ops._p(torch.zeros(64, dtype=torch.int32, device=DEV))

    def raw(**null):      # the launcher itself: (3, 8) outputs, every pointer valid except the ones named
        p = {k: (None if k in null else z) for k in ("src", "dec", "rows", "labels_c", "M", "work", "examples", "seq_off")}
        return lib.adt_bertbatch_build(ops._p(dd.seq_off) if p["seq_off"] else None, ops._p(dd.seq_items), ops._p(dd.win_start), ops._p(dd.win_len),
                                       ops._p(ex) if p["examples"] else None, 3, 0, 3, 8, dd.W, 2, dd.U, ITEMS, 0, 0, dd.thr_mask, p["src"], p["dec"],
                                       None, p["rows"], p["labels_c"], p["M"], None, p["work"], ops._stream())
    for name in ("src", "dec", "rows", "labels_c", "M", "work", "examples", "seq_off"):
        assert raw(**{name: True}) != 0, name
        assert b"NULL" in lib.adt_last_error()
    assert lib.adt_bertbatch_eval(None, ops._p(dd.seq_items), z, 3, dd.U, 8, ITEMS, z, ops._stream()) != 0
    with pytest.raises(_lib.AdtError):
        ops.bertbatch_eval(dd.seq_off, dd.seq_items, ex, 0, ITEMS)
    # example ids are checked on the host, before the upload
    for bad in ([0, len(dd)], [-1, 0]):
        with pytest.raises(_lib.AdtError):
            dd.set_order(bad)
    dd.set_order([len(dd) - 1, 0])
    # an empty shard and an empty batch are no-ops that still report M = 0
    out = build(dd, [0, 1, 2], rows=(1, 1))
    assert out[0].shape == (0, 8) and out[5][0] == 0
    out = build(dd, [])
    assert out[0].shape == (0, 8) and out[5][0] == 0 and out[6][0] == 1.0
