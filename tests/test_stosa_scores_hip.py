"""GPU: STOSA-ADT full-sort scores on the device -- adt_hit_hist (adt_amd/csrc/adt_hithist.cuh) through
ops.hit_hist( against the numpy replay of tests/test_stosa_scores_cpu.py, bit for bit; FusedStosaTrainer.full_sort_scores against
full_sort + get_full_sort_score; DeviceDisenData.eval_stage against eval_batch; SearcherEvolution.evaluate_candidates and stosa.main with
--device_batches / --device_scores against the same runs without them.

Histograms are integers and are compared exactly.  Scores: 1e-12 absolute -- both sides are float64 sums of at most N <= 64 terms no
larger than 1, divided by N (tests/test_stosa_scores_cpu.py).

The model-level cases take the `small` and `l2h2` goldens' architectures (maxlen, width, heads, layers, seed) with the item table
widened to 64 rows: their own catalogues have 42 and 33 items, so with topk = 40 every fused batch (l2h2: every list) would come back
short and `fused_fallbacks == 1` over two batches could not hold.  The parameters of those goldens are drawn from (cfg, seed) by
oracle/stosa_oracle.py:init_params, so the wider table is drawn the same way.  The KL golden is used at its own 42 items (two-pass
lists continue into the seen items)."""
import functools
import json
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from adt_amd import _lib, ops  # noqa: E402
from tests.test_stosa_scores_cpu import replay_hit_hist  # noqa: E402

DEV = "cuda:0"
TOL = 1e-12
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


class Args:
    pass


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---- 1. the kernel against the replay ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def list_case(K, rpg, groups):
    """Rows by kind (global row r, kind r % 7): 0 the answer first, 1 last, 2 absent, 3 a -1 tail from K // 2 with the answer before it
    (absent when there is no room), 4 the answer twice, 5 absent with a -1 tail, 6 at a random position.  Every fourth answer is 0; a
    row whose answer is 0 lists id 0 only where its kind places the answer."""
    r = np.random.RandomState(1000 * K + 10 * rpg + groups)
    N = rpg * groups
    ans = r.randint(1, 1000, size=rpg).astype(np.int32)
    ans[3::4] = 0
    top = r.randint(1, 1000, size=(N, K)).astype(np.int32)
    for row in range(N):
        a, kind, t = ans[row % rpg], row % 7, K // 2
        top[row][top[row] == a] = 1000                  # the answer stands only where the kind puts it (answers 1..999, 0: never drawn)
        if kind == 0:
            top[row, 0] = a
        elif kind == 1:
            top[row, K - 1] = a
        elif kind == 3:
            top[row, t:] = -1
            if t > 0:
                top[row, r.randint(t)] = a
        elif kind == 4 and K >= 2:
            p, q = sorted(r.choice(K, 2, replace=False))
            top[row, p] = top[row, q] = a
        elif kind == 5:
            top[row, t:] = -1
        elif kind == 6:
            top[row, r.randint(K)] = a
    hist, pos = replay_hit_hist(top, ans, rpg)
    return top, ans, hist, pos


@pytest.mark.parametrize("K", (1, 5, 40, 63, 64, 65, 128))
def test_hit_hist_matches_replay(K):
    sizes_checked = set()
    for rpg in (1, 63, 64, 65, 257):
        for groups in (1, 3):
            top, ans, r_hist, r_pos = list_case(K, rpg, groups)
            N = rpg * groups
            if rpg >= 63:                                   # the replay itself: every kind stands where list_case put it
                assert r_pos[0] == 0 and r_pos[1] == K - 1 and r_pos[2] == K and r_pos[5] == K
                zero_rows = [row for row in range(N) if ans[row % rpg] == 0]
                assert any(r_pos[row] < K for row in zero_rows) and any(r_pos[row] == K for row in zero_rows)
                sizes_checked.add(rpg)
            wide = np.empty((N, K + 3), np.int32)
            wide[:, :K] = top
            wide[:, K:] = np.tile(ans, groups)[:, None]     # beyond column K: the answer itself -- a read past K would hit
            for t in (dev(top), dev(wide)[:, :K]):
                assert t.stride(0) == (K if t.is_contiguous() else K + 3) or N == 1
                hist, pos = ops.hit_hist(t, dev(ans), rows_per_group=rpg, want_pos=True)
                assert hist.shape == (groups, K + 1) and hist.dtype == torch.int64 and pos.shape == (N,) and pos.dtype == torch.int32
                assert np.array_equal(hist.cpu().numpy(), r_hist), (K, rpg, groups)
                assert np.array_equal(pos.cpu().numpy(), r_pos), (K, rpg, groups)
            # answers as (rows_per_group, 1), rows_per_group from their length, no positions; then a second call accumulates
            if groups == 1:
                h = ops.hit_hist(dev(top), dev(ans[:, None]))
                assert np.array_equal(h.cpu().numpy(), r_hist)
            h = torch.full((groups, K + 1), 7, device=DEV, dtype=torch.int64)
            out = ops.hit_hist(dev(top), dev(ans), rpg, hist=h)
            assert out is h
            ops.hit_hist(dev(top), dev(ans), rpg, hist=h)
            assert np.array_equal(h.cpu().numpy(), 7 + 2 * r_hist), (K, rpg, groups)
    assert sizes_checked == {63, 64, 65, 257}


def test_hit_hist_many_rows_one_group():
    """More rows than 256 blocks x 16 rows: the waves stride over the group (5000 rows, K = 40), most of them misses on one bin."""
    r = np.random.RandomState(3)
    N, K = 5000, 40
    top = r.randint(1, 300, size=(N, K)).astype(np.int32)
    ans = r.randint(0, 3000, size=N).astype(np.int32)
    r_hist, r_pos = replay_hit_hist(top, ans)
    hist, pos = ops.hit_hist(dev(top), dev(ans), want_pos=True)
    assert np.array_equal(hist.cpu().numpy(), r_hist) and np.array_equal(pos.cpu().numpy(), r_pos)
    assert 0 < r_hist[0, K] < N


def test_hit_hist_no_rows_leaves_hist_alone():
    h = torch.arange(41, device=DEV, dtype=torch.int64).view(1, 41).clone()
    out = ops.hit_hist(torch.empty(0, 40, device=DEV, dtype=torch.int32), torch.zeros(5, device=DEV, dtype=torch.int32), hist=h)
    assert out is h and np.array_equal(h.cpu().numpy()[0], np.arange(41))
    fresh = ops.hit_hist(torch.empty(0, 40, device=DEV, dtype=torch.int32), torch.zeros(5, device=DEV, dtype=torch.int32))
    assert fresh.shape == (0, 41)


# ---- 2. argument errors ------------------------------------------------------------------------------------------------------------------
def test_hit_hist_argument_errors():
    ans = torch.zeros(4, device=DEV, dtype=torch.int32)
    for K in (0, 129):
        with pytest.raises(_lib.AdtError):
            ops.hit_hist(torch.zeros(4, K, device=DEV, dtype=torch.int32), ans)
    with pytest.raises(_lib.AdtError):
        ops.hit_hist(torch.zeros(6, 40, device=DEV, dtype=torch.int32), ans)                      # 6 rows, groups of 4
    with pytest.raises(_lib.AdtError):
        ops.hit_hist(torch.zeros(4, 40, device=DEV, dtype=torch.int32), ans, hist=torch.zeros(1, 40, device=DEV, dtype=torch.int64))
    lib = _lib.load()
    top, hist = torch.zeros(8, 40, device=DEV, dtype=torch.int32), torch.zeros(2, 41, device=DEV, dtype=torch.int64)

    def call(ld=40, n_rows=8, K=40, rpg=4, t=top, a=ans, h=hist):
        return lib.adt_hit_hist(ops._p(t), ld, n_rows, K, ops._p(a), rpg, ops._p(h), None, ops._stream())
    assert call() == 0
    for kw in (dict(K=0), dict(K=129, ld=129), dict(ld=39), dict(n_rows=6), dict(rpg=0), dict(n_rows=-4), dict(t=None), dict(a=None), dict(h=None)):
        assert call(**kw) != 0, kw
        with pytest.raises(_lib.AdtError):
            _lib.check(call(**kw), "hit_hist")
    torch.cuda.synchronize()
    assert int(hist.sum()) == 8                              # the one good call counted its rows; no failed call touched hist


# ---- 3. full_sort_scores against full_sort + get_full_sort_score --------------------------------------------------------------------------
def golden_model(tag, metric="wasserstein", item_size=None):
    """The golden's architecture and seed (tests/test_stosa_fullrank_hip.py:load_case), the item table `item_size` rows (docstring)."""
    from oracle import stosa_oracle as so
    from adt_amd.stosa.models import DisenDistSAModel
    g = np.load(os.path.join(GOLD, "stosa_%s.npz" % tag))
    V, L, d, H, nl, nu = [int(x) for x in g["cfg"]]
    V = V if item_size is None else item_size
    cfg = so.Cfg(V, L, d, H, nl, num_users=nu, pvn_weight=float(g["pvn_weight"]))
    P = so.init_params(cfg, int(g["seed"]))
    a = Args()
    a.device, a.item_size, a.maxlen, a.hidden_units, a.num_heads, a.num_layers, a.num_users = DEV, V, L, d, H, nl, nu
    a.dropout, a.attention_dropout, a.pvn_weight, a.precision, a.distance_metric = 0.0, 0.0, cfg.pvn_weight, "f32", metric
    m = DisenDistSAModel(a)
    m.load_numpy(P)
    return m.eval(), cfg


def two_batches(V, L, B=21, seed=5):
    """Two batches in three forms of `seen` (dense, scipy CSR); the second has a user with all but five items seen."""
    import scipy.sparse as sp
    from tests.test_stosa_fullrank_hip import random_batch
    r = np.random.RandomState(seed)
    seqs, dense = random_batch(r, B, L, V)
    seqs2, dense2 = random_batch(r, B, L, V, heavy_row=7)
    ans, ans2 = r.randint(1, V, size=(B, 1)).astype(np.int64), r.randint(1, V, size=(B, 1)).astype(np.int64)
    return [(seqs, dense, ans), (seqs2, sp.csr_matrix(dense2), ans2)], (dense, dense2)


def check_scores_route(tr, batches, fused, want_fallbacks):
    from adt_amd.stosa.trainer import get_full_sort_score
    pred, ans = tr.full_sort(batches, topk=40, fused=fused)
    assert tr.fused_fallbacks == want_fallbacks
    tr.fused_fallbacks = -1
    scores, hist = tr.full_sort_scores(batches, topk=40, fused=fused)
    assert tr.fused_fallbacks == want_fallbacks
    r_hist, _ = replay_hit_hist(pred, ans)
    assert isinstance(hist, np.ndarray) and hist.dtype == np.int64 and hist.shape == (41,)
    assert np.array_equal(hist, r_hist[0]), (hist, r_hist[0])
    err = np.abs(np.array(scores) - np.array(get_full_sort_score(ans, pred))).max()
    print("fused", fused, "hits", int(hist[:40].sum()), "of", int(hist.sum()), "max score difference", err)
    assert len(scores) == 13 and err <= TOL
    return hist


@pytest.mark.parametrize("tag", ("small", "l2h2"))
def test_full_sort_scores_matches_full_sort(tag):
    from adt_amd.stosa.trainer import FusedStosaTrainer
    m, cfg = golden_model(tag, item_size=64)
    V = cfg.item_size
    assert V > 45                                            # room for 40 unseen items in the light batch
    batches, (dense, dense2) = two_batches(V, cfg.maxlen)
    assert V - dense.sum(1).max() >= 40 and V - dense2.sum(1).max() == 5 and V - np.delete(dense2, 7, 0).sum(1).max() >= 40
    tr = FusedStosaTrainer(m, [0.3] * cfg.num_layers, [0.2] * cfg.num_layers)
    h2 = check_scores_route(tr, batches, False, 0)
    hf = check_scores_route(tr, batches, True, 1)
    assert 0 < h2[:40].sum() and h2.sum() == hf.sum() == 42
    # the held-out ids as a device tensor, the seen lists as device pairs with the caller's min_unseen: the same histogram
    devb = []
    for (seqs, seen, ans), dn in zip(batches, (dense, dense2)):
        ip, ix = ops.seen_csr(dn, len(seqs), DEV)
        devb.append((dev(seqs.astype(np.int32)), (ip, ix), dev(ans[:, 0].astype(np.int32)), int(V - dn.sum(1).max())))
    scores, hist = tr.full_sort_scores(devb, topk=40, fused=True)
    assert np.array_equal(hist, hf) and tr.fused_fallbacks == 1
    with pytest.raises(_lib.AdtError, match="min_unseen"):   # a device pair without the count: no silent read-back
        tr.full_sort_scores([b[:3] for b in devb], topk=40, fused=True)
    with pytest.raises(_lib.AdtError):                       # scores_from_hist reports k up to 40
        tr.full_sort_scores(batches, topk=10)


def test_full_sort_scores_kl_two_pass():
    from adt_amd.stosa.trainer import FusedStosaTrainer
    m, cfg = golden_model("kl_small", "kl")
    batches, _ = two_batches(cfg.item_size, cfg.maxlen)
    tr = FusedStosaTrainer(m, [0.3] * cfg.num_layers, [0.2] * cfg.num_layers)
    check_scores_route(tr, batches, False, 0)
    with pytest.raises(_lib.AdtError, match="wasserstein"):
        tr.full_sort_scores(batches, topk=40, fused=True)


# ---- 4. no read-back ---------------------------------------------------------------------------------------------------------------------
class ReadBackGuard:
    """Records every device -> host copy a torch.Tensor method can make: .cpu(), .to(cpu), .item(), .tolist(), .numpy() and the scalar
    conversions, each only when called on a device tensor."""

    def __init__(self, monkeypatch):
        self.copies = []
        for name in ("cpu", "item", "tolist", "numpy", "__bool__", "__int__", "__float__", "__index__"):
            self._wrap(monkeypatch, name)
        orig_to = torch.Tensor.to

        def to(t, *a, **kw):
            tgt = kw.get("device", a[0] if a else None)
            if t.is_cuda and (isinstance(tgt, (str, torch.device)) and torch.device(tgt).type == "cpu"):
                self.copies.append(("to", tuple(t.shape), t.dtype))
            return orig_to(t, *a, **kw)
        monkeypatch.setattr(torch.Tensor, "to", to)

    def _wrap(self, monkeypatch, name):
        orig = getattr(torch.Tensor, name)

        def wrapped(t, *a, **kw):
            if t.is_cuda:
                self.copies.append((name, tuple(t.shape), t.dtype))
            return orig(t, *a, **kw)
        monkeypatch.setattr(torch.Tensor, name, wrapped)


def test_full_sort_scores_copies_only_the_histogram(monkeypatch):
    from adt_amd.stosa.trainer import FusedStosaTrainer
    m, cfg = golden_model("small", item_size=64)
    batches, _ = two_batches(cfg.item_size, cfg.maxlen)      # the second batch falls back: the two-pass ids stay on the device too
    tr = FusedStosaTrainer(m, [0.3], [0.2])
    want = {f: tr.full_sort_scores(batches, topk=40, fused=f)[1] for f in (False, True)}
    with monkeypatch.context() as mp:
        guard = ReadBackGuard(mp)
        for fused in (False, True):
            del guard.copies[:]
            scores, hist = tr.full_sort_scores(batches, topk=40, fused=fused)
            assert guard.copies == [("cpu", (41,), torch.int64)], guard.copies
            assert np.array_equal(hist, want[fused])
        del guard.copies[:]
        tr.full_sort(batches, topk=40, fused=True)           # the guard itself: the id-list route copies every batch back
        assert len(guard.copies) >= 2 and all(c[0] == "cpu" for c in guard.copies), guard.copies


# ---- 5. DeviceDisenData.eval_stage -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", (8, 50))
def test_eval_stage_matches_eval_batch(L):
    from adt_amd.stosa.datasets import rating_matrix
    from tests.test_stosa_devbatch_hip import CUT, device_data, lengths, make_seqs
    item_size = 40
    user_seq = make_seqs(lengths(L), item_size, 77)
    n = len(user_seq)
    dd = device_data(user_seq, item_size, L)
    for split in ("valid", "test"):
        dense = rating_matrix(user_seq, n, item_size, CUT[split]).toarray() != 0
        for start, B in ((0, n), (3, 5), (n - 1, 1)):
            inp, (indptr, indices), ans = dd.eval_batch(split, start, B)
            st = dd.eval_stage(split, start, B)
            assert sorted(st) == ["answers", "answers_host", "indices", "indptr", "inp", "min_unseen"]
            assert torch.equal(st["inp"], inp) and torch.equal(st["indptr"], indptr) and torch.equal(st["indices"], indices)
            assert np.array_equal(st["answers_host"], ans) and st["answers_host"].shape == (B, 1)
            assert st["answers"].is_cuda and st["answers"].dtype == torch.int32 and st["answers"].shape == (B,)
            assert np.array_equal(st["answers"].cpu().numpy(), ans[:, 0])
            assert isinstance(st["min_unseen"], int) and st["min_unseen"] == item_size - int(dense[start:start + B].sum(1).max()), (split, start, B)


# ---- 6. the search -----------------------------------------------------------------------------------------------------------------------
def write_sequences(path, users, items, heavy_user, seed):
    """`user item item ...` lines: 5..15 items per user, except `heavy_user`, who has seen all but 20 of the items."""
    r = np.random.RandomState(seed)
    with open(path, "w") as f:
        for u in range(users):
            seq = r.permutation(items)[:items - 20] + 1 if u == heavy_user else r.randint(1, items + 1, size=r.randint(5, 16))
            f.write("%d %s\n" % (u + 1, " ".join(str(int(x)) for x in seq)))


@pytest.fixture(scope="module")
def searcher(tmp_path_factory):
    """SearcherEvolution with the architecture of the superstosa_c3 golden (maxlen 12, width 64, 4 heads, 1 layer) on a written file of 50
    users and 120 items; user 20 has fewer than 40 unseen items.  Batches of 16: three full ones and one of 2."""
    from adt_amd.stosa import evolution as ev
    g = np.load(os.path.join(GOLD, "superstosa_c3.npz"))
    V, L, d, H, nl, nu = [int(x) for x in g["cfg"]]
    tmp = tmp_path_factory.mktemp("search")
    write_sequences(str(tmp / "Tiny.txt"), 50, 120, 20, 4)
    args = ev.parse_args(["--dataset", "Tiny", "--data_dir", str(tmp) + "/", "--maxlen", str(L), "--hidden_units", str(d), "--num_heads", str(H),
                          "--num_layers", str(nl), "--eval_batch_size", "16", "--precision", "f32", "--device_batches", "--seed", str(int(g["seed"]))])
    args.data_file = os.path.join(args.data_dir, args.dataset + ".txt")
    torch.manual_seed(args.seed)
    np.random.seed(args.seed)
    s = ev.SearcherEvolution(args)
    r = np.random.RandomState(9)
    cands = [[float(x) for x in g["cand"]], [float(x) for x in g["cand2"]], [float(x) for x in r.rand(2 * nl)]]
    return s, cands


@pytest.mark.parametrize("fused", (False, True))
def test_search_flags_agree(searcher, fused, monkeypatch):
    from adt_amd.stosa import searcher as searcher_module
    from adt_amd.stosa.trainer import get_full_sort_score
    s, cands = searcher
    assert s.dev_data is not None and s.args.item_size > 100
    seen = np.diff(s.valid_matrix.tocsr().indptr)
    assert s.args.item_size - seen[20] < 40 and s.args.item_size - np.delete(seen, 20).max() >= 40
    lists = []                                               # the (answers, id lists) the host route scores, one pair per candidate

    def recording(answers, pred):
        lists.append((answers, pred))
        return get_full_sort_score(answers, pred)
    monkeypatch.setattr(searcher_module, "get_full_sort_score", recording)

    def host_hists():
        out = np.stack([replay_hit_hist(pred, answers)[0][0] for answers, pred in lists])
        del lists[:]
        return out
    base = s.evaluate_candidates(cands, group=2, fused=fused, device_batches=False, device_scores=False)
    r_hists = host_hists()
    assert r_hists.shape == (3, 41) and (r_hists.sum(1) == 50).all() and r_hists[:, :40].sum() > 0
    for device_batches in (False, True):
        for device_scores in (False, True):
            if not (device_batches or device_scores):
                continue
            s.last_hists = None
            out = s.evaluate_candidates(cands, group=2, fused=fused, device_batches=device_batches, device_scores=device_scores)
            hists = s.last_hists if device_scores else host_hists()
            assert not lists                                 # --device_scores never calls the Python scoring
            assert np.array_equal(hists, r_hists), (device_batches, device_scores)
            assert len(out) == 3
            for got, want in zip(out, base):
                assert sorted(got) == sorted(want) == ["MRR", "V_HR", "V_MRR", "V_NDCG"]
                assert max(abs(got[k] - want[k]) for k in want) <= TOL, (device_batches, device_scores, got, want)
    # the test split, one pass of all three candidates, both flags on
    base = s.evaluate_candidates(cands, s.test_ds, s.test_matrix, group=8, prefix="T", fused=fused, device_batches=False, device_scores=False)
    out = s.evaluate_candidates(cands, s.test_ds, s.test_matrix, group=8, prefix="T", fused=fused, device_batches=True, device_scores=True)
    assert all(max(abs(a[k] - b[k]) for k in b) <= TOL for a, b in zip(out, base)) and "T_MRR" in out[0]


def test_search_device_batches_need_resident_data(searcher):
    s, cands = searcher
    kept, s.dev_data = s.dev_data, None
    try:
        with pytest.raises(_lib.AdtError):
            s.evaluate_candidates(cands, device_batches=True)
    finally:
        s.dev_data = kept


# ---- 7. command line ---------------------------------------------------------------------------------------------------------------------
def test_cli_device_scores(tmp_path, capsys):
    """The same run with and without --device_scores.  lr = 0 keeps the weights at their seeded initial values through the epoch: the
    training step sums with float atomics, so two trainings differ in their last bits, and only the scoring is compared here."""
    from adt_amd.stosa.main import _write_synthetic, main
    data = tmp_path / "data"
    data.mkdir()
    _write_synthetic(str(data / "Beauty.txt"), users=96, items=150, seed=3)
    over = {"epochs": 1, "maxlen": 20, "batch_size": 32, "eval_batch_size": 48, "lr": 0.0}
    argv = ["--dataset", "Beauty", "--data_dir", str(data) + "/", "--device_batches", "--fused_eval", "--synthetic", "1", "--epochs", "1",
            "--eval_set", "64", "--override", json.dumps(over)]
    outs, lines = [], []
    for i, extra in enumerate(([], ["--device_scores"])):
        outs.append(main(argv + ["--output_dir", str(tmp_path / ("out%d" % i)) + "/"] + extra))
        lines += [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    (v0, t0), (v1, t1) = outs
    assert len(v1) == len(t1) == 13 and len(lines) == 2
    print("valid", v0, "test", t0)
    assert np.abs(np.array(v0) - np.array(v1)).max() <= TOL and np.abs(np.array(t0) - np.array(t1)).max() <= TOL
    assert abs(lines[0]["valid_MRR"] - lines[1]["valid_MRR"]) <= TOL and abs(lines[0]["valid_HIT@10"] - lines[1]["valid_HIT@10"]) <= TOL
    # host batches feed the same scores
    v2, t2 = main([a for a in argv if a != "--device_batches"] + ["--output_dir", str(tmp_path / "out2") + "/", "--device_scores"])
    assert np.abs(np.array(v0) - np.array(v2)).max() <= TOL and np.abs(np.array(t0) - np.array(t2)).max() <= TOL
