"""GPU: the STOSA-ADT evolutionary search under distance_metric='kl' (adt_amd/stosa/searcher.py).

SearcherEvolution.evaluate_candidates scores every group of candidates with one adt_kldist_full_groups call per validation batch, E =
the batch's rows (the trailing batch of 2 has its own E), on an item image packed once per call.  Checked here: the id lists are the
stable argsort of the path's own distance matrices (seen items at 1e24); the matrices equal selecting each candidate alone
(set_choice + predict_full: adt_kldist_full) to 1e-5 of the largest distance -- id lists of the two kernels are NOT compared, fp32
near-ties may swap --; --device_scores / --device_batches give exactly the host-scored metrics (integer histograms, scores to 1e-12
as in tests/test_stosa_scores_hip.py); fused=True is refused; and one whole search writes its result file."""
import json
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from adt_amd import _lib, ops  # noqa: E402
from tests.test_stosa_scores_cpu import replay_hit_hist  # noqa: E402
from tests.test_stosa_scores_hip import write_sequences  # noqa: E402

TOL = 1e-12
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def make_searcher(tmp, extra):
    """SearcherEvolution with the architecture of the superstosa_c3 golden (maxlen 12, width 64, 4 heads, 1 layer) on a written file of 50
    users and 120 items; user 20 has fewer than 40 unseen items.  Batches of 16: three full ones and one of 2."""
    from adt_amd.stosa import evolution as ev
    g = np.load(os.path.join(GOLD, "superstosa_c3.npz"))
    V, L, d, H, nl, nu = [int(x) for x in g["cfg"]]
    write_sequences(str(tmp / "Tiny.txt"), 50, 120, 20, 4)
    args = ev.parse_args(["--dataset", "Tiny", "--data_dir", str(tmp) + "/", "--maxlen", str(L), "--hidden_units", str(d), "--num_heads", str(H),
                          "--num_layers", str(nl), "--eval_batch_size", "16", "--precision", "f32", "--device_batches", "--distance_metric", "kl",
                          "--seed", str(int(g["seed"]))] + extra)
    args.data_file = os.path.join(args.data_dir, args.dataset + ".txt")
    torch.manual_seed(args.seed)
    np.random.seed(args.seed)
    return ev.SearcherEvolution(args), g, nl


@pytest.fixture(scope="module")
def searcher(tmp_path_factory):
    s, g, nl = make_searcher(tmp_path_factory.mktemp("klsearch"), [])
    r = np.random.RandomState(9)
    cands = [[float(x) for x in g["cand"]], [float(x) for x in g["cand2"]]] + [[float(x) for x in r.rand(2 * nl)] for _ in range(3)]
    return s, cands


def test_kl_search_lists_and_distances(searcher, monkeypatch):
    s, cands = searcher
    assert s.model.distance_metric == "kl" and len(cands) == 5
    passes, packs = [], []
    real_predict, real_topk, real_pack = s.model.predict_full_candidates, ops.topk_masked, ops.kldist_pack

    def predict(inp, sl, stats=None, image=None):
        assert image is not None                              # the image of this call, not one packed per pass
        dist = real_predict(inp, sl, stats=stats, image=image)
        passes.append({"inp": inp, "sl": sl, "dist": dist.clone()})
        return dist

    def topk(dist, k, indptr=None, indices=None, want_val=False):
        out = real_topk(dist, k, indptr, indices, want_val)
        passes[-1].update(k=k, indptr=indptr, indices=indices, top=out)
        return out

    def pack(*a):
        packs.append(1)
        return real_pack(*a)
    monkeypatch.setattr(s.model, "predict_full_candidates", predict)
    monkeypatch.setattr(ops, "topk_masked", topk)
    monkeypatch.setattr(ops, "kldist_pack", pack)
    out = s.evaluate_candidates(cands, group=2, device_batches=False, device_scores=False)
    monkeypatch.undo()
    assert len(packs) == 1                                    # packed once per call
    assert len(out) == 5 and all(np.isfinite(v) for o in out for v in o.values())
    assert len(passes) == 4 * 3 and sorted(set(len(p["inp"]) for p in passes)) == [2, 16]      # 4 batches x groups of 2, 2, 1; E = 16 and 2
    worst = 0.0
    for p in passes:
        B, n = len(p["inp"]), len(p["sl"])
        dist = p["dist"].cpu().numpy()
        assert dist.shape == (n * B, s.args.item_size) and p["k"] == 40
        masked = dist.copy()
        if p["indptr"] is not None:
            ip, ix = p["indptr"].cpu().numpy(), p["indices"].cpu().numpy()
            assert ip.size == n * B + 1
            for r in range(n * B):
                masked[r, ix[ip[r]:ip[r + 1]]] = np.float32(1e24)
        assert np.array_equal(p["top"].cpu().numpy(), np.argsort(masked, axis=1, kind="stable")[:, :40])
        for k in range(n):
            s.model.shared = p["sl"][k]
            one = s.model.predict_full(p["inp"]).cpu().numpy()
            e = np.abs(dist[k * B:(k + 1) * B] - one).max() / np.abs(one).max()
            worst = max(worst, e)
            assert e <= 1e-5, (B, k, e)
    print("kl search: grouped against single-candidate distances, worst %.3g of the largest distance" % worst)


def test_kl_search_flags_agree(searcher, monkeypatch):
    from adt_amd.stosa import searcher as searcher_module
    from adt_amd.stosa.trainer import get_full_sort_score
    s, cands = searcher
    lists = []

    def recording(answers, pred):
        lists.append((answers, pred))
        return get_full_sort_score(answers, pred)
    monkeypatch.setattr(searcher_module, "get_full_sort_score", recording)

    def host_hists():
        out = np.stack([replay_hit_hist(pred, answers)[0][0] for answers, pred in lists])
        del lists[:]
        return out
    base = s.evaluate_candidates(cands, group=2, device_batches=False, device_scores=False)
    r_hists = host_hists()
    assert r_hists.shape == (5, 41) and (r_hists.sum(1) == 50).all()
    for device_batches in (False, True):
        for device_scores in (False, True):
            if not (device_batches or device_scores):
                continue
            s.last_hists = None
            out = s.evaluate_candidates(cands, group=2, device_batches=device_batches, device_scores=device_scores)
            hists = s.last_hists if device_scores else host_hists()
            assert not lists
            assert np.array_equal(hists, r_hists), (device_batches, device_scores)
            for got, want in zip(out, base):
                assert sorted(got) == sorted(want) == ["MRR", "V_HR", "V_MRR", "V_NDCG"]
                assert max(abs(got[k] - want[k]) for k in want) <= TOL, (device_batches, device_scores, got, want)


def test_kl_search_fused_raises(searcher):
    s, cands = searcher
    with pytest.raises(_lib.AdtError):
        s.evaluate_candidates(cands, group=2, fused=True)
    with pytest.raises(_lib.AdtError):
        s.evaluate_candidates(cands, group=2, fused=True, device_batches=True, device_scores=True)


def test_kl_search_end_to_end(tmp_path, monkeypatch):
    """One warm-up epoch, one search epoch, a population of 4: the result file, one record per surviving candidate, a finite loss."""
    monkeypatch.chdir(tmp_path)
    s, _, nl = make_searcher(tmp_path, ["--warmup_epochs", "1", "--search_epochs", "1", "--population_num", "4", "--select_num", "2",
                                        "--crossover_num", "1", "--mutation_num", "1", "--batch_size", "16", "--device_scores",
                                        "--out_dir", str(tmp_path / "res")])
    path = s.search()
    assert np.isfinite(float(s.trainer.loss()))
    recs = [json.loads(l) for l in open(path)]
    assert len(recs) == 2 and all(np.isfinite(r["MRR"]) for r in recs)
    assert [r["MRR"] for r in recs] == sorted((r["MRR"] for r in recs), reverse=True)
    assert all(len(json.loads(r["cand"])) == 2 * nl for r in recs)
    assert os.path.exists(tmp_path / "checkpoint" / "super.pth")
