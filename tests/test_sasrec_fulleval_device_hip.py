"""GPU: SASRec-ADT's full-catalogue evaluation on device-resident data -- evaluate_full_device against
evaluate_full on the flagship and the wide model, SuperSASRecModel.rank_full_stats_candidates against single-candidate calls and
against the full score matrix, sasrec/evolution.py --eval_full / --select_by, sasrec/main.py --device_eval_full, and two gloo ranks.
Data sets and models: tests/sasrec_deveval_cases.py; the data-parallel child: tests/sasrec_fulleval_cases.py."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from adt_amd import ops  # noqa: E402
from adt_amd.sasrec import utils as U  # noqa: E402
from adt_amd.sasrec.device_eval import DeviceEvalData  # noqa: E402

import sasrec_deveval_cases as cases  # noqa: E402

DEV = "cuda:0"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


def eval_sets(mode, L=8):
    train, valid, test, usernum, itemnum = cases.make_data(60)
    sampler = U.PopularSampler(train, valid, test, usernum, itemnum, 5)
    ds = U.EvalDataset(train, valid, test, usernum, itemnum, L, sampler, mode, -1, frozen=False)
    return ds, DeviceEvalData.from_dataset(ds, DEV, upload=False)


# ---- 6. device metrics equal host metrics -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("make", (flagship, wide50), ids=("flagship_d64_h2", "wide_d50_h1"))
@pytest.mark.parametrize("mode", ["val", "test"])
def test_evaluate_full_device_equals_evaluate_full(make, mode):
    m = make()
    ds, data = eval_sets(mode)
    assert not data.drawn                                   # no candidate table is needed: never uploaded, never drawn
    host = [m.rank_full(np.stack([ds.sequence(u) for u in ds.users[s:s + 16]]), [U.eval_target(ds, u) for u in ds.users[s:s + 16]],
                        U.eval_seen_csr(ds, ds.users[s:s + 16])) for s in range(0, len(ds.users), 16)]
    host_ranks = np.concatenate([h[0].cpu().numpy() for h in host])
    (nd_h, hr_h), auc_h = U.evaluate_full(m, ds, mode, (5, 10), 16)
    ((nd_d, hr_d), auc_d), ranks = U.evaluate_full_device(m, data, (5, 10), 16, want_ranks=True)
    assert ranks.dtype == torch.int32 and np.array_equal(ranks.cpu().numpy(), host_ranks)
    assert host_ranks.min() >= 0 and len(set(host_ranks.tolist())) > 5
    tol = len(ds.users) * 2.0 ** -52
    for k in (5, 10):
        print(k, nd_d[k], nd_h[k], hr_d[k], hr_h[k])
        assert hr_d[k] == hr_h[k] and abs(nd_d[k] - nd_h[k]) <= tol * abs(nd_h[k])
    print(auc_d, auc_h)
    assert abs(auc_d - auc_h) <= tol * abs(auc_h)
    (nd_1, hr_1), auc_1 = U.evaluate_full_device(m, data, (5, 10), 512)      # one batch or three: the same histogram
    assert (nd_1, hr_1) == (nd_d, hr_d) and abs(auc_1 - auc_d) <= tol * abs(auc_d)


# ---- 7. supernet stats ------------------------------------------------------------------------------------------------------------------
REC, IND = [0, 0.0001, 0.0005, 0.001, 0.005, 0.01], [0, 0.0001, 0.0005, 0.001, 0.0015, 0.002]


def supernet(d, H, lanes, L=8, nl=2):
    from adt_amd.sasrec.supersasrec import SuperSASRecModel
    a = Args()
    a.device, a.num_heads, a.maxlen, a.num_layers, a.hidden_units, a.dropout, a.precision = DEV, H, L, nl, d, 0.0, "f32"
    torch.manual_seed(13)
    return SuperSASRecModel(1, cases.ITEMNUM, REC, IND, a, allow_lanes=lanes).eval()


@pytest.mark.parametrize("d,H,lanes", [(64, 2, False), (50, 1, True)], ids=("tiled_d64_h2", "padded_d50_h1"))
def test_rank_full_stats_candidates(d, H, lanes):
    from adt_amd.supersearch import cand_to_block, get_shared
    m, kh, V = supernet(d, H, lanes), 10, cases.ITEMNUM
    assert (m.lanes is not None) == lanes
    ds, data = eval_sets("val")
    r = np.random.RandomState(3)
    shared = [get_shared(REC, IND, cand_to_block(REC, IND, [float(x) for x in r.rand(4)])[0]) for _ in range(3)]
    lo, hi = 3, 24                                          # 21 users from row 3: tiles straddle both group boundaries
    B = hi - lo
    seq, *full = data.full_batch(lo, hi)
    hist = torch.zeros(3, kh + 1, device=DEV, dtype=torch.int64)
    auc = torch.zeros(3, device=DEV, dtype=torch.float64)
    h, a, ranks = m.rank_full_stats_candidates(seq, full, shared, hist, auc, kh, want_rank=True)
    assert h is hist and a is auc and ranks.shape == (3, B)
    for p in range(3):                                      # per candidate: a single-candidate call
        h1, a1, r1 = m.rank_full_stats_candidates(seq, full, shared[p:p + 1], torch.zeros(1, kh + 1, device=DEV, dtype=torch.int64),
                                                  torch.zeros(1, device=DEV, dtype=torch.float64), kh, want_rank=True)
        assert torch.equal(r1[0], ranks[p]) and torch.equal(h1[0], hist[p])
        assert torch.equal(a1.view(torch.int64)[0], auc.view(torch.int64)[p])
        assert int(h1.sum()) == B
    # the ranks of predict_rank_candidates(seq, None, ...) restricted to the unseen items, from its full score matrix.  The matrix comes
    # from adt_score_rank, whose fp32 sum runs in another order than adt_full_rank's: an item within tol = 2 d 2^-24 sum |F E| of the
    # target (the first-order bound of a length-d fp32 sum, doubled, as in test_fullrank_hip.py) may fall on either side.
    F, _, L = m._candidate_feature_rows(seq, shared)
    E = m.P("item_emb.weight")
    S = ops.score_rank(F[L - 1:], L * m.dp, E, None, 3 * B, V + 1, False)[0].double().cpu().numpy()
    Fl = F[L - 1::L].double().abs().cpu().numpy()
    tol = 2.0 * m.dp * 2.0 ** -24 * (Fl @ E.double().abs().cpu().numpy().T)
    seen = cases.seen_rows(ds.user_train, ds.user_val, ds.user_test, ds.users[lo:hi], "val")
    got, exact = ranks.cpu().numpy(), 0
    for p in range(3):
        for b in range(B):
            t = int(data.targets_host[lo + b])
            other = np.ones(V + 1, bool)
            other[0] = False
            other[seen[b]] = False
            other[t] = False
            s, e = S[p * B + b], tol[p * B + b]
            low, high = int((other & (s > s[t] + e + e[t])).sum()), int((other & (s > s[t] - e - e[t])).sum())
            assert low <= got[p, b] <= high, (p, b, low, got[p, b], high)
            exact += low == high
    assert exact >= 3 * B - 3                               # the margin is used by a stray near tie at the most


# ---- 8. the search ----------------------------------------------------------------------------------------------------------------------
SEARCH = ["--dataset", "tiny", "--synthetic", "tiny", "--maxlen", "20", "--sample_size", "20", "--num_layers", "2", "--hidden_units", "64",
          "--num_heads", "2", "--eval_batch_size", "24", "--batch_size", "32", "--precision", "f32", "--warmup_epochs", "1", "--search_epochs", "1",
          "--population_num", "4", "--select_num", "2", "--crossover_num", "1", "--mutation_num", "1"]


@pytest.mark.parametrize("select_by", ["auc", "ndcg"])
def test_search_scores_candidates_on_the_whole_catalogue(tmp_path, monkeypatch, select_by):
    from adt_amd.sasrec import evolution as ev
    monkeypatch.chdir(tmp_path)
    calls = {"groups": [], "cand": 0}
    real_groups, real_cand = ops.full_rank_groups, ops.cand_rank_hist

    def spy_groups(F, ldf, E, n_items, target, seen_off, seen_items, n_rows, rows_per_group, **kw):
        calls["groups"].append((n_rows, rows_per_group, kw.get("row0", 0)))
        return real_groups(F, ldf, E, n_items, target, seen_off, seen_items, n_rows, rows_per_group, **kw)

    def spy_cand(*a, **kw):
        calls["cand"] += 1
        return real_cand(*a, **kw)
    monkeypatch.setattr(ops, "full_rank_groups", spy_groups)
    monkeypatch.setattr(ops, "cand_rank_hist", spy_cand)
    args = ev.parse_args(SEARCH + ["--data_dir", str(tmp_path), "--out_dir", str(tmp_path / "res"), "--eval_full", "true", "--select_by", select_by])
    ev.set_rng_seed(args.seed)
    s = ev.SearcherEvolution(args)
    assert s.val_dev is not None and not s.val_dev.drawn
    path = s.search()
    infos = [v for v in s.vis_dict.values() if "visited" in v]
    assert len(infos) >= 4
    for info in infos:
        assert all(0.0 <= info[key] <= 1.0 for key in ("V_NDCG", "V_HR", "V_AUC", "auc")) and info["auc"] == info["V_AUC"]
    N = len(s.val_dev)
    sizes = [min(24, N - lo) for lo in range(0, N, 24)]
    assert calls["cand"] == 0 and calls["groups"]
    for n_rows, rpg, row0 in calls["groups"]:               # rows_per_group is the batch, the groups are the candidates of the chunk
        assert rpg == sizes[row0 // 24] and row0 % 24 == 0 and n_rows % rpg == 0
    key = "V_NDCG" if select_by == "ndcg" else "auc"
    assert s.search_state.score_key == key
    top = [s.vis_dict[str(c)][key] for c in s.search_state.top]
    first = sorted((s.vis_dict[str(c)][key] for c in s.search_state.memory[0]), reverse=True)      # the one selection: over the first population
    assert top == first[:2] and len(first) == 4
    recs = [json.loads(l) for l in open(path)]              # the output file: the same records as ever
    assert len(recs) == len(top) and all({"V_NDCG", "V_HR", "V_AUC", "auc", "cand", "rec", "ind"} <= set(rec) for rec in recs)


def test_select_by_ndcg_needs_the_whole_catalogue(capsys):
    from adt_amd.sasrec import evolution as ev
    with pytest.raises(SystemExit) as e:
        ev.parse_args(["--dataset", "tiny", "--select_by", "ndcg"])
    assert e.value.code == 2 and "--eval_full true" in capsys.readouterr().err


# ---- 9. main.py -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra", [["--hidden_units", "64", "--num_heads", "2"], ["--hidden_units", "50", "--num_heads", "1"]], ids=("fused_d64", "wide_d50"))
def test_main_with_device_eval_full(tmp_path, monkeypatch, capsys, extra):
    from adt_amd.sasrec import main as M
    monkeypatch.chdir(tmp_path)
    calls = {"device": 0, "host": 0}
    real = U.evaluate_full_device

    def spy_device(*a, **kw):
        calls["device"] += 1
        return real(*a, **kw)

    def spy_host(*a, **kw):
        calls["host"] += 1
        raise AssertionError("evaluate_full ran under --device_eval_full")
    monkeypatch.setattr(U, "evaluate_full_device", spy_device)
    monkeypatch.setattr(U, "evaluate_full", spy_host)
    M.main(["--dataset", "ml-1m", "--train_dir", "full", "--data_dir", str(tmp_path / "data"), "--synthetic", "tiny", "--no_template", "--maxlen", "20",
            "--sample_size", "20", "--batch_size", "32", "--num_epochs", "1", "--eval_interval", "1", "--device_eval_full", "true"] + extra)
    out = capsys.readouterr().out
    lines = [l for l in out.splitlines() if "full catalogue:" in l]
    assert calls == {"device": 2, "host": 0} and len(lines) == 2, out[-2000:]      # the test set and the validation set; one line per k
    for line in lines:
        nums = [float(x) for x in line.split("full catalogue:")[1].replace(")", " ").replace(",", " ").split() if x[0].isdigit() and "." in x]
        assert len(nums) == 4 and all(math.isfinite(x) and 0.0 <= x <= 1.0 for x in nums), line


# ---- 10. two gloo ranks on one GPU ------------------------------------------------------------------------------------------------------
def test_evaluate_full_device_under_a_process_group(tmp_path):
    """Two gloo ranks sharing the GPU take batches r, r + 2, ... and sum-reduce the int64 histogram and the float64 sum: every rank prints
    the single process's HR and NDCG exactly and its AUC to the order of addition (tests/sasrec_fulleval_cases.py: dp_main)."""
    script = os.path.join(REPO, "tests", "sasrec_fulleval_cases.py")
    env = dict(os.environ, PYTHONPATH=REPO, HSA_ENABLE_IPC_MODE_LEGACY="0")
    outs = []
    for cmd in ([sys.executable, script],
                [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port",
                 str(28700 + os.getpid() % 1000), script]):
        p = subprocess.run(cmd, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
        outs.append([json.loads(l) for l in p.stdout.splitlines() if l.startswith("{")])
    one, two = outs
    assert len(one) == 1 and sorted(r["rank"] for r in two) == [0, 1] and all(r["world"] == 2 for r in two)
    for r in two:
        print(r["auc"], one[0]["auc"])
        assert (r["ndcg"], r["hr"]) == (one[0]["ndcg"], one[0]["hr"])
        assert abs(r["auc"] - one[0]["auc"]) <= one[0]["users"] * 2.0 ** -52 * abs(one[0]["auc"])
    assert 0.0 < one[0]["auc"] < 1.0
