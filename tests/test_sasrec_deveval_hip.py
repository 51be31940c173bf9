"""GPU: the device-resident sampled evaluation of SASRec-ADT -- adt_evalcand_draw against its Python replay, the
guard, shards and salts, the sequence rows against EvalDataset.sequence, adt_cand_rank_hist against predict_rank (planted exact ties
included), evaluate_device against evaluate_loader on the flagship and the wide model, rank_hist_candidates on a supernet, and
sasrec/main.py with the two flags.  Data sets and replay: tests/sasrec_deveval_cases.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from adt_amd import _lib, ops  # noqa: E402
from adt_amd.sasrec import utils as U  # noqa: E402
from adt_amd.sasrec.device_eval import DeviceEvalData  # noqa: E402

import sasrec_deveval_cases as cases  # noqa: E402

DEV = "cuda:0"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, "tests", "golden")
_DATA = {}


def data_of(max_hist):
    if max_hist not in _DATA:
        _DATA[max_hist] = cases.make_data(max_hist)
    return _DATA[max_hist]


def dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def raw_draw(cum, seen, targets, S, seed, salt, rows=None):
    """adt_evalcand_draw on host arrays: (cand, filled) as numpy."""
    off = np.zeros(len(seen) + 1, np.int64)
    np.cumsum([len(s) for s in seen], out=off[1:])
    items = np.concatenate(seen) if off[-1] else np.zeros(1, np.int64)
    cand, filled = ops.evalcand_draw(dev(cum, np.int64), int(cum[-1]), dev(off, np.int64), dev(items, np.int32), dev(targets, np.int32), S, seed, salt,
                                     rows=rows, want_filled=True)
    return cand.cpu().numpy(), filled.cpu().numpy()


# ---- 1. the sampler ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,max_hist", cases.SAMPLER_CASES)
@pytest.mark.parametrize("mode", ["val", "test"])
def test_draw_equals_the_python_replay(S, max_hist, mode):
    train, valid, test, usernum, itemnum = data_of(max_hist)
    data = DeviceEvalData(train, valid, test, usernum, itemnum, 8, S, mode, device=DEV)
    cand, filled = data.draw(23, 4, want_filled=True)
    cand, filled = cand.cpu().numpy(), filled.cpu().numpy()
    seen = cases.seen_rows(train, valid, test, data.users, mode)
    assert cand.shape == (len(data.users), 1 + S) and (filled == S).all()
    assert np.array_equal(cand[:, 0], data.targets_host)
    for row, s in enumerate(seen):
        want, _, used = cases.replay_row(data.cum_host, s, S, 23, 4, row)
        assert used is not None                       # the sampling path (test_sasrec_deveval_cpu.py checks the margin)
        assert cand[row, 1:].tolist() == want, row
        neg = cand[row, 1:]
        assert len(set(neg.tolist())) == S and not set(neg.tolist()) & set(s.tolist())
        assert neg.min() >= 1 and neg.max() < itemnum and cases.ZERO_ID not in neg
    xs = ops.evalcand_stream(data.cum_host, 23, 4, 0, 0, 64)           # the host stream itself: row 0's first candidate is its first unseen value
    assert cand[0, 1] == next(int(x) for x in xs if int(x) not in set(seen[0].tolist()))
    assert data.cand.data_ptr() == data.batch(0, 3)[1].data_ptr()      # the table is filled in place and batches are views of it


def test_draw_shards_salts_and_repeats():
    S = 64
    train, valid, test, usernum, itemnum = data_of(60)
    data = DeviceEvalData(train, valid, test, usernum, itemnum, 8, S, "val", device=DEV)
    whole = data.draw(23, 1).cpu().numpy().copy()
    assert np.array_equal(data.draw(23, 1).cpu().numpy(), whole)                      # the same (seed, salt) repeats exactly
    other = data.draw(23, 2).cpu().numpy().copy()
    assert np.array_equal(other[:, 0], whole[:, 0]) and (other[:, 1:] != whole[:, 1:]).any(axis=1).all()      # another salt: other negatives, nothing else
    assert (data.draw(24, 1).cpu().numpy()[:, 1:] != whole[:, 1:]).any(axis=1).all()
    N = len(data.users)
    for lo, hi in ((0, 1), (5, 17), (17, N), (N, N)):                                  # a shard draws what the whole call would
        part = ops.evalcand_draw(data.cum, data.total, data.seen_off, data.seen_items, data.targets, S, 23, 1, rows=(lo, hi))
        assert np.array_equal(part.cpu().numpy(), whole[lo:hi]), (lo, hi)
    data.draw(23, 2)
    data.draw(23, 1, rows=(5, 17))                                                     # in place: rows 5..16 alone change
    got = data.cand.cpu().numpy()
    assert np.array_equal(got[5:17], whole[5:17]) and np.array_equal(got[:5], other[:5]) and np.array_equal(got[17:], other[17:])


@pytest.mark.parametrize("S", [5, 64, 100])
def test_guard_fills_from_the_walk(S):
    """4096 stream values go by without a free id (the table makes them about 1e-7 each), so the walk fills the slots: a user with S + 1
    free ids gets S distinct ones of them and a full count, in the replay's order; a user with S - 2 gets those, id 0 in the open slots
    and a short count; DeviceEvalData refuses such a user."""
    cum, gseen, free = cases.guard_table(S + 1)
    cum2, gseen2, free2 = cases.guard_table(S - 2)
    some = np.array([3, 9, 20], np.int64)
    targets = np.array([11, 12, 13], np.int32)
    cand, filled = raw_draw(cum, [some, gseen, some], targets, S, 7, 0)
    want, n, used = cases.replay_row(cum, gseen, S, 7, 0, 1)
    assert used is None and n == S
    assert filled.tolist() == [S, S, S] and cand[1, 1:].tolist() == want
    assert len(set(want)) == S and set(want) <= set(free) and cand[1, 0] == 12
    cand2, filled2 = raw_draw(cum2, [some, gseen2, some], targets, S, 7, 0)
    want2, n2, _ = cases.replay_row(cum2, gseen2, S, 7, 0, 1)
    assert n2 == S - 2 and filled2.tolist() == [S, S - 2, S]
    assert cand2[1, 1:].tolist() == want2 and sorted(cand2[1, 1:S - 1].tolist()) == free2 and (cand2[1, S - 1:] == 0).all()
    # rows next to the guard row are ordinary rows of the same table
    for row in (0, 2):
        assert cand2[row, 1:].tolist() == cases.replay_row(cum2, some, S, 7, 0, row)[0]


def test_device_eval_data_refuses_a_user_without_enough_items():
    train, valid, test, usernum, itemnum = data_of(60)
    with pytest.raises(_lib.AdtError, match="drawable"):
        DeviceEvalData(train, valid, test, usernum, itemnum, 8, 100, "test", device=DEV)


# ---- 2. the sequence rows ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [8, 50])
@pytest.mark.parametrize("mode", ["val", "test"])
def test_sequence_rows_equal_evaldataset(L, mode):
    train, valid, test, usernum, itemnum = data_of(60)
    sampler = U.PopularSampler(train, valid, test, usernum, itemnum, 5)
    ds = U.EvalDataset(train, valid, test, usernum, itemnum, L, sampler, mode, -1, frozen=False)
    data = DeviceEvalData.from_dataset(ds, DEV, upload=False)
    n_train = sorted({len(train[u]) for u in ds.users})
    assert n_train[0] < L and L in n_train and n_train[-1] > L - (mode == "test")      # shorter than, equal to and longer than L
    want = np.stack([ds.sequence(u) for u in ds.users])
    assert np.array_equal(data.sequences(0, len(ds.users)).cpu().numpy(), want)
    assert np.array_equal(data.sequences(7, 19).cpu().numpy(), want[7:19])
    with pytest.raises(_lib.AdtError, match="no candidates"):
        data.batch(0, 4)


# ---- 3. adt_cand_rank_hist --------------------------------------------------------------------------------------------------------------
class Args:
    pass


def flagship(L=8):
    return cases.flagship(DEV, L)


def wide50(L=8):
    from adt_amd.sasrec.model_wide import SASRecADTWide
    a = Args()
    a.device, a.num_heads, a.maxlen, a.num_layers, a.hidden_units, a.dropout, a.precision = DEV, 1, L, 1, 50, 0.0, "f32"
    torch.manual_seed(12)
    return SASRecADTWide(1, cases.ITEMNUM, a).eval()


def duplicate_item_row(m, src, dst):
    """Item dst gets item src's embedding, so the two score exactly alike."""
    if hasattr(m, "R"):
        m.R("item_emb.weight")[dst].copy_(m.R("item_emb.weight")[src])
        m.push()
    else:
        off, n, shape = m._views["item_emb.weight"]
        E = m.flat[off:off + n].view(shape)
        E[dst].copy_(E[src])


@pytest.mark.parametrize("make", (flagship, wide50), ids=("flagship_d64_h2", "wide_d50_h1"))
@pytest.mark.parametrize("C", [1, 6, 101])
def test_cand_rank_hist_equals_predict_rank(make, C):
    m, V, L, B = make(), cases.ITEMNUM, 8, 21
    duplicate_item_row(m, 5, 9)
    r = np.random.RandomState(C)
    seqs = [r.randint(1, V + 1, size=(B, L)).astype(np.int32) for _ in range(3)]
    for s in seqs:
        s[:, :3] = 0
    cand = r.randint(1, V + 1, size=(B, C)).astype(np.int32)
    if C > 3:
        cand[0, 3] = cand[0, 0]              # a candidate equal to the target: an exact tie, not counted
        cand[1, 0], cand[1, 2] = 5, 9        # a duplicated table row: likewise
        cand[2, 0], cand[2, 1], cand[2, 4] = 9, 5, 5
    cand_d = dev(cand, np.int32)
    want = [m.predict_rank(s, cand)[1].cpu().numpy() for s in seqs]
    assert all(w.min() >= 0 and w.max() < C for w in want)
    hist = torch.zeros(1, C, device=DEV, dtype=torch.int64)
    total = np.zeros(C, np.int64)
    feats = []
    for s, w in zip(seqs, want):                                   # accumulating batches equals the sum
        F, E, _, bias = m._full_rank_operands(dev(s, np.int32))
        h, rk = ops.cand_rank_hist(F, F.stride(0), E, cand_d, B, hist=hist, bias=bias, want_rank=True)
        assert h is hist and np.array_equal(rk.cpu().numpy(), w)
        total += np.bincount(w, minlength=C)
        assert np.array_equal(hist.cpu().numpy()[0], total)
        feats.append(F.clone())
    # P = 3 stacked groups over ONE candidate slice equal three separate calls
    stacked = torch.cat(feats, 0)
    h3, rk3 = ops.cand_rank_hist(stacked, stacked.stride(0), E, cand_d, 3 * B, B, want_rank=True)
    assert np.array_equal(rk3.cpu().numpy(), np.concatenate(want))
    assert np.array_equal(h3.cpu().numpy(), np.stack([np.bincount(w, minlength=C) for w in want]))


def test_cand_rank_hist_strides_over_more_rows_than_its_grid():
    """4096 workgroups of 4 waves serve 16,384 rows; beyond that the waves stride.  3 groups of 5,500 rows, d 64, C 5, against
    adt_score_rank's ranks on the same rows."""
    G, B, C, d, V = 3, 5500, 5, 64, 200
    g = torch.Generator().manual_seed(4)
    F = torch.randn(G * B, d, generator=g).to(DEV)
    E = torch.randn(V + 1, d, generator=g).to(DEV)
    bias = torch.randn(V + 1, generator=g).to(DEV)
    cand = torch.randint(0, V + 1, (B, C), generator=g, dtype=torch.int32).to(DEV)
    cand[:, 3] = cand[:, 0]
    want = ops.score_rank_bias(F, d, E, bias, cand.repeat(G, 1), G * B, C)[1].cpu().numpy()
    hist, rk = ops.cand_rank_hist(F, d, E, cand, G * B, B, bias=bias, want_rank=True)
    assert np.array_equal(rk.cpu().numpy(), want) and want.max() <= C - 2
    assert np.array_equal(hist.cpu().numpy(), np.stack([np.bincount(want[i * B:(i + 1) * B], minlength=C) for i in range(G)]))


# ---- 4. ranks and metrics ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("make", (flagship, wide50), ids=("flagship_d64_h2", "wide_d50_h1"))
@pytest.mark.parametrize("mode", ["val", "test"])
def test_evaluate_device_equals_evaluate_loader(make, mode):
    m, S = make(), 64
    train, valid, test, usernum, itemnum = data_of(60)
    sampler = U.PopularSampler(train, valid, test, usernum, itemnum, S)
    ds = U.EvalDataset(train, valid, test, usernum, itemnum, 8, sampler, mode, -1, frozen=True, seed=23)
    data = DeviceEvalData.from_dataset(ds, DEV)
    assert np.array_equal(data.cand.cpu().numpy(), np.stack([ds._frozen[u] for u in ds.users]))
    host_ranks = np.concatenate([m.predict_rank(seq, items)[1].cpu().numpy() for (_, seq, items), _ in ds.batches(16)])
    (nd_h, hr_h), auc_h = U.evaluate_loader(m, ds.batches(16), None, mode, (5, 10))
    ((nd_d, hr_d), auc_d), ranks = U.evaluate_device(m, data, (5, 10), 16, want_ranks=True)
    assert np.array_equal(ranks.cpu().numpy(), host_ranks)
    tol = len(ds.users) * 2.0 ** -52
    for k in (5, 10):
        print(k, nd_d[k], nd_h[k], hr_d[k], hr_h[k])
        assert hr_d[k] == hr_h[k] and abs(nd_d[k] - nd_h[k]) <= tol * abs(nd_h[k])
    print(auc_d, auc_h)
    assert abs(auc_d - auc_h) <= tol * abs(auc_h)
    assert U.evaluate_device(m, data, (5, 10), 512) == ((nd_d, hr_d), auc_d)      # one batch or three: the same histogram


def test_evaluate_device_under_a_process_group(tmp_path):
    """Two gloo ranks sharing the GPU take batches r, r + 2, ... and sum-reduce the int64 histogram: every rank prints exactly the single
    process's metrics (tests/sasrec_deveval_cases.py: dp_main)."""
    script = os.path.join(REPO, "tests", "sasrec_deveval_cases.py")
    env = dict(os.environ, PYTHONPATH=REPO, HSA_ENABLE_IPC_MODE_LEGACY="0")
    outs = []
    for cmd in ([sys.executable, script],
                [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port",
                 str(29700 + os.getpid() % 1000), script]):
        p = subprocess.run(cmd, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
        outs.append([json.loads(l) for l in p.stdout.splitlines() if l.startswith("{")])
    one, two = outs
    assert len(one) == 1 and sorted(r["rank"] for r in two) == [0, 1] and all(r["world"] == 2 for r in two)
    for r in two:
        assert (r["ndcg"], r["hr"], r["auc"]) == (one[0]["ndcg"], one[0]["hr"], one[0]["auc"])
    assert 0.0 < one[0]["auc"] < 1.0


def test_rank_hist_candidates_equals_predict_rank_candidates():
    from adt_amd.sasrec.supersasrec import SuperSASRecModel
    from adt_amd.supersearch import cand_to_block, get_shared
    from oracle import super_oracle as su
    g = np.load(os.path.join(GOLD, "super_c3.npz"))
    V, L, d, H, nl = [int(x) for x in g["cfg"]]
    cfg = su.Cfg(V, L, d, H, nl, g["rec_choice"], g["ind_choice"], 0.0)
    a = Args()
    a.device, a.num_heads, a.maxlen, a.num_layers, a.hidden_units, a.dropout, a.precision = DEV, H, L, nl, d, 0.0, "f32"
    m = SuperSASRecModel(1, V, cfg.rec_choice, cfg.ind_choice, a)
    m.load_numpy(su.init_params(cfg, int(g["seed"])))
    r = np.random.RandomState(7)
    cands = [[float(x) for x in g["cand"]]] + [[float(x) for x in r.rand(2 * nl)] for _ in range(4)]
    shared = [get_shared(g["rec_choice"], g["ind_choice"], cand_to_block(g["rec_choice"], g["ind_choice"], c)[0]) for c in cands]
    items = np.ascontiguousarray(g["items"], dtype=np.int32)
    want = m.predict_rank_candidates(g["seq"], items, shared).cpu().numpy()
    C = items.shape[1]
    hist = torch.zeros(len(cands), C, device=DEV, dtype=torch.int64)
    for _ in range(2):
        assert m.rank_hist_candidates(dev(g["seq"], np.int32), dev(items, np.int32), shared, hist) is hist
    assert np.array_equal(hist.cpu().numpy(), 2 * np.stack([np.bincount(w, minlength=C) for w in want]))
    # groups of candidates into slices of one histogram, as the search does
    hist2 = torch.zeros(len(cands), C, device=DEV, dtype=torch.int64)
    for g0 in range(0, len(cands), 2):
        m.rank_hist_candidates(dev(g["seq"], np.int32), dev(items, np.int32), shared[g0:g0 + 2], hist2[g0:g0 + 2])
    assert np.array_equal(2 * hist2.cpu().numpy(), hist.cpu().numpy())


def test_search_scores_candidates_on_the_device(tmp_path, monkeypatch):
    """sasrec/evolution.py --device_eval: evaluate_candidates over the resident validation set returns the host path's records (the same
    frozen candidates; several batches, chunks of 3 candidates); --device_negatives draws its own and repeats itself."""
    from adt_amd.sasrec import evolution as ev
    monkeypatch.chdir(tmp_path)
    argv = ["--dataset", "tiny", "--data_dir", str(tmp_path), "--synthetic", "tiny", "--maxlen", "20", "--sample_size", "20", "--num_layers", "2",
            "--hidden_units", "64", "--num_heads", "2", "--eval_batch_size", "24", "--precision", "f32"]
    out = {}
    for tag, extra in (("host", []), ("dev", ["--device_eval", "true"]), ("neg", ["--device_negatives", "true"])):
        args = ev.parse_args(argv + extra)
        ev.set_rng_seed(args.seed)
        s = ev.SearcherEvolution(args)
        assert (s.val_dev is not None) == bool(extra) and args.device_eval == bool(extra)
        r = np.random.RandomState(2)
        cands = [[float(x) for x in r.rand(4)] for _ in range(7)]
        out[tag] = s.evaluate_candidates(cands, group=3)
        if tag == "neg":
            assert s.val_ds._frozen is None and s.evaluate_candidates(cands, group=7) == out[tag]
    tol = 64 * 2.0 ** -52
    for a, b, c in zip(out["host"], out["dev"], out["neg"]):
        assert a["V_HR"] == b["V_HR"] and set(a) == set(b) == set(c)
        for key in ("V_NDCG", "V_AUC", "auc"):
            assert abs(a[key] - b[key]) <= tol * abs(a[key]), key
        assert all(0.0 <= c[key] <= 1.0 for key in c)


# ---- 5. command line --------------------------------------------------------------------------------------------------------------------
def run_main(tmp_path, tag, extra):
    cmd = [sys.executable, "-m", "adt_amd.sasrec.main", "--dataset", "ml-1m", "--train_dir", tag, "--data_dir", str(tmp_path / "data"), "--synthetic",
           "tiny", "--no_template", "--hidden_units", "64", "--num_heads", "2", "--maxlen", "20", "--sample_size", "20", "--batch_size", "32",
           "--num_epochs", "2", "--eval_interval", "1"] + extra
    # ADT_ITEM_SORT=1: the bit-reproducible step, so that two runs train the same weights
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""), ADT_ITEM_SORT="1")
    p = subprocess.run(cmd, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    recs = [json.loads(l) for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(recs) == 2, p.stdout[-2000:]
    return recs


METRICS = [(split, key) for split in ("valid", "test") for key in ("ndcg10", "hr10", "auc")]


def test_main_with_device_eval_prints_the_host_metrics(tmp_path):
    host = run_main(tmp_path, "host", [])
    dev_eval = run_main(tmp_path, "deveval", ["--device_eval", "true"])
    tol = 64 * 2.0 ** -52                 # the preset's 64 users
    for a, b in zip(host, dev_eval):      # training untouched, the candidates the same: the host path's own metrics
        assert a["loss"] == b["loss"]
        for split, key in METRICS:
            print(split, key, a[split][key], b[split][key])
            assert abs(a[split][key] - b[split][key]) <= tol * abs(a[split][key]), (split, key)


def test_main_with_device_negatives_repeats_itself(tmp_path):
    both = [run_main(tmp_path, "devneg%d" % i, ["--device_eval", "true", "--device_negatives", "true"]) for i in range(2)]
    for a, b in zip(*both):
        assert a["loss"] == b["loss"]
        for split, key in METRICS:
            assert 0.0 <= a[split][key] <= 1.0 and a[split][key] == b[split][key], (split, key)


def test_main_redraws_on_the_device_or_refuses(tmp_path):
    """--frozen_eval false redraws at every evaluation (salt = evaluation counter) with the device sampler, and is refused without it."""
    for rec in run_main(tmp_path, "redraw", ["--device_negatives", "true", "--frozen_eval", "false"]):
        assert all(0.0 <= rec[split][key] <= 1.0 for split, key in METRICS)
    cmd = [sys.executable, "-m", "adt_amd.sasrec.main", "--dataset", "ml-1m", "--train_dir", "x", "--no_template", "--device_eval", "true", "--frozen_eval", "false"]
    p = subprocess.run(cmd, cwd=str(tmp_path), env=dict(os.environ, PYTHONPATH=REPO), capture_output=True, text=True, timeout=120)
    assert p.returncode != 0 and "--device_negatives" in p.stderr
