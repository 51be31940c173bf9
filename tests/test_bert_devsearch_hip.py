"""GPU: BERT4Rec-ADT's evaluation and lambda search on device-resident data -- SuperBertModel.rank_hist_candidates,
FusedBertTrainer.evaluate(device_scores=True), DeviceBertData.add_eval(candidates="device") / draw_eval, SuperBertTrainer.step_device,
SearcherEvolution under --device_batches / --device_scores / --device_negatives and both command lines.

Integer outputs (ranks, histograms, candidate tables, HR) are compared exactly: the counting kernel shares its arithmetic with the ranking
kernel (tests/test_sasrec_deveval_hip.py:test_cand_rank_hist_equals_predict_rank).  NDCG and AUC are compared within n * 2^-52 relative,
n the number of users: the two float64 sums differ by their order of addition only.  The trainer bound is the one
tests/test_bert_devbatch_hip.py:test_step_device_matches_step_on_the_same_arrays uses (loss 1e-5, weights 5e-4 of the largest weight)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from adt_amd import _lib, ops  # noqa: E402
from adt_amd.bert4rec import datasets as D  # noqa: E402

import bert_devsearch_cases as cases  # noqa: E402

DEV = "cuda:0"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ITEMNUM, L, S = cases.ITEMNUM, cases.L, cases.S


def dev(a, dtype=np.int32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def close(a, b, n):
    return abs(a - b) <= n * 2.0 ** -52 * abs(b)


# ---- 1. the supernet's scores counted on the device ------------------------------------------------------------------------------------
def test_rank_hist_candidates_equals_predict_rank_candidates():
    """P = 5 candidates in groups of 2 (the last group holds one), batches of 7, 7 and 3 rows into one histogram, C = 17; one candidate
    equal to its row's target: an exact tie, not counted above it."""
    from adt_amd.supersearch import cand_to_block, get_shared
    m = cases.super_model(DEV)
    r = np.random.RandomState(7)
    cands = [[float(x) for x in r.rand(4)] for _ in range(5)]
    shared = [get_shared(cases.REC_CHOICE, cases.IND_CHOICE, cand_to_block(cases.REC_CHOICE, cases.IND_CHOICE, c)[0]) for c in cands]
    C = 1 + S
    hist = torch.zeros(5, C, device=DEV, dtype=torch.int64)
    want = np.zeros((5, C), np.int64)
    for b, B in enumerate((7, 7, 3)):
        seq = r.randint(1, ITEMNUM + 1, size=(B, L)).astype(np.int32)
        seq[:, :2], seq[:, -1] = 0, ITEMNUM + 1
        items = np.stack([r.permutation(ITEMNUM)[:C] + 1 for _ in range(B)]).astype(np.int32)
        items[0, 3] = items[0, 0]
        for g0 in range(0, 5, 2):
            sl = shared[g0:g0 + 2]
            ranks = m.predict_rank_candidates(seq, items, sl).cpu().numpy()
            assert ranks.shape == (len(sl), B) and ranks.min() >= 0 and ranks[:, 0].max() <= C - 2
            want[g0:g0 + 2] += np.stack([np.bincount(rk, minlength=C) for rk in ranks])
            # host arrays on the first batch, device tensors afterwards: `ids` takes both
            a, c = (seq, items) if b == 0 else (dev(seq), dev(items))
            assert m.rank_hist_candidates(a, c, sl, hist[g0:g0 + 2]).data_ptr() == hist[g0:g0 + 2].data_ptr()
        assert np.array_equal(hist.cpu().numpy(), want)
    assert (want.sum(1) == 17).all()                                               # every row counted once per candidate
    with pytest.raises(_lib.AdtError):                                             # two histogram rows for three candidates
        m.rank_hist_candidates(seq, items, shared[:3], hist[:2])


# ---- 2. evaluate(device_scores=True) --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[(64, 2, "bf16"), (50, 1, "f32")], ids=["d64_h2", "d50_h1_padded"])
def trainer(request):
    from adt_amd.bert4rec.trainer import FusedBertTrainer
    d, H, prec = request.param
    m = cases.bert_model(DEV, d, H, prec)
    assert m.dp == 64 and (m.lanes is None) == (d == 64)
    return FusedBertTrainer(m, [0.1, 0.1], [0.1, 0.1])


@pytest.mark.parametrize("mode", ["val", "test"])
def test_evaluate_device_scores_equals_evaluate(trainer, mode):
    train, valid, test, usernum, sampler, ds = cases.eval_sets(mode)
    dd = D.DeviceBertData(train, usernum, ITEMNUM, L, 0.2, DEV)
    dd.add_eval(ds)
    n = len(ds)
    assert n == 38 and dd.eval_len(mode) == n
    (nd_w, hr_w), auc_w = trainer.evaluate(ds.batches(16))
    assert 0.0 < auc_w < 1.0
    got = {"host": trainer.evaluate(ds.batches(16), device_scores=True), "device": trainer.evaluate(dd.eval_batches(mode, 16), device_scores=True)}
    for tag, ((nd, hr), auc) in got.items():
        for k in (5, 10):
            print(mode, tag, k, hr[k], hr_w[k], nd[k], nd_w[k])
            assert hr[k] == hr_w[k] and close(nd[k], nd_w[k], n), (tag, k)
        print(mode, tag, auc, auc_w)
        assert close(auc, auc_w, n) and isinstance(auc, float)
    assert got["host"] == got["device"]
    # one batch or three: the same histogram, so the same tuple; other cut-offs come from the same histogram too
    assert trainer.evaluate(dd.eval_batches(mode, 512), device_scores=True) == got["device"]
    (nd3, hr3), _ = trainer.evaluate(dd.eval_batches(mode, 16), ks=(1, 3), device_scores=True)
    (nd3w, hr3w), _ = trainer.evaluate(dd.eval_batches(mode, 16), ks=(1, 3))
    assert hr3 == hr3w and all(close(nd3[k], nd3w[k], n) for k in (1, 3))


def test_evaluate_device_scores_refuses_a_batch_of_another_candidate_count(trainer):
    train, valid, test, usernum, sampler, ds = cases.eval_sets("val")
    batches = list(ds.batches(16))
    batches[2] = (batches[2][0], batches[2][1][:, :-1])
    with pytest.raises(_lib.AdtError, match="candidates"):
        trainer.evaluate(batches, device_scores=True)
    with pytest.raises(_lib.AdtError):
        trainer.evaluate([], device_scores=True)
    trainer.evaluate(batches[:2], device_scores=True)


# ---- 3. candidates drawn on the device ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["val", "test"])
def test_draw_eval_equals_the_python_replay(mode, monkeypatch):
    train, valid, test, usernum, sampler, ds = cases.eval_sets(mode)
    monkeypatch.setattr(sampler, "get_negative_samples", lambda *a, **k: pytest.fail("the host sampler was called"))
    dd = D.DeviceBertData(train, usernum, ITEMNUM, L, 0.2, DEV)
    dd.add_eval(ds, candidates="device")
    with pytest.raises(_lib.AdtError, match="draw_eval"):
        dd.eval_batch(mode, 0, 4)
    table = dd.draw_eval(mode, 23)
    got = table.cpu().numpy()
    assert got.shape == (len(ds), 1 + S) and got.dtype == np.int32
    cum, total, seen_off, seen_items = D.device_candidate_tables(train, valid, test, ITEMNUM, ds.users, S)
    tgt = valid if mode == "val" else test
    for row, u in enumerate(ds.users):
        seen = seen_items[seen_off[row]:seen_off[row + 1]]
        ids, filled, used = cases.sc.replay_row(cum, seen, S, 23, 0, row)
        assert used is not None and filled == S                      # the sampling path, not the guard
        assert got[row, 0] == tgt[u][0] and got[row, 1:].tolist() == ids, row
        assert len(set(ids)) == S and not set(ids) & (set(train[u]) | set(valid[u]) | set(test[u]))
        assert min(ids) >= 1 and max(ids) <= ITEMNUM and cases.sc.ZERO_ID not in ids
    assert (got[:, 1:] == ITEMNUM).any()      # id itemnum is drawable here (SASRec-ADT's table stops before it)
    # the batches are views of the table, beside the device-built rows
    seq, cand = dd.eval_batch(mode, 5, 7)
    assert np.array_equal(cand.cpu().numpy(), got[5:12]) and np.array_equal(seq.cpu().numpy(), np.array([ds.sequence(u) for u in ds.users[5:12]]))
    # the same arguments repeat; another salt or seed is another table over the same targets
    assert np.array_equal(dd.draw_eval(mode, 23).cpu().numpy(), got)
    for seed, salt in ((23, 1), (24, 0)):
        other = dd.draw_eval(mode, seed, salt).cpu().numpy()
        assert np.array_equal(other[:, 0], got[:, 0]) and not np.array_equal(other, got)
    with pytest.raises(_lib.AdtError):
        dd.draw_eval("valid", 23)
    with pytest.raises(_lib.AdtError):
        dd.add_eval(ds, candidates="gpu")
    # host candidates again under the same mode: no draw is pending
    monkeypatch.undo()
    dd.add_eval(ds)
    assert np.array_equal(dd.eval_batch(mode, 0, 4)[1].cpu().numpy(), next(ds.batches(4))[1])


def test_draw_eval_refuses_a_user_without_enough_items():
    train, valid, test, usernum, sampler, ds = cases.eval_sets("val", sample_size=100)
    dd = D.DeviceBertData(train, usernum, ITEMNUM, L, 0.2, DEV)
    with pytest.raises(_lib.AdtError, match=r"user \d+ has \d+ drawable items"):
        dd.add_eval(ds, candidates="device")
    assert "val" not in dd._eval


# ---- 4. the warm-up step on a device batch -----------------------------------------------------------------------------------------------
def test_super_step_device_matches_step_on_the_same_arrays():
    from adt_amd.bert4rec.superbert import SuperBertTrainer
    train, valid, test, usernum, itemnum = cases.make_data()
    B = 4
    dd = D.DeviceBertData(train, usernum, itemnum, L, 0.3, DEV, dupe_factor=2, prop_sliding_window=0.5)
    order = np.random.RandomState(2).permutation(len(dd))
    dd.set_order(order)
    r = np.random.RandomState(4)
    choices = [[float(x) for x in r.rand(4)] for _ in range(2)]
    outs = []
    for device in (True, False):
        m = cases.super_model(DEV, dropout=0.3, attention_dropout=0.2)
        tr = SuperBertTrainer(m, weight_decay=1e-4, seed=5)
        for i in range(2):
            tr.set_choice(choices[i])
            st = dd.train_stage(B * i, B, 9, 1)
            if device:
                tr.step_device(st)
            else:       # the arrays of the same staged batch, read back
                src, dec, lab = (t.cpu().numpy() for t in ops.bertbatch_build(dd.seq_off, dd.seq_items, dd.win_start, dd.win_len,
                                                                              dd.order[B * i:B * (i + 1)], L, dd.dupe_factor, itemnum,
                                                                              dd.thr_mask, 9, 1)[:3])
                assert np.array_equal(src, st["src"].cpu().numpy()) and np.array_equal(dec, st["dec"].cpu().numpy())
                assert int(st["M"].item()) == np.count_nonzero(lab) > 0
                tr.step(src, dec, lab)
        torch.cuda.synchronize()
        outs.append((float(tr.loss()), m.flat.cpu().numpy().astype(np.float64), dict(tr.steps)))
    (loss_d, flat_d, steps_d), (loss_h, flat_h, steps_h) = outs
    rel = np.abs(flat_d - flat_h).max() / max(np.abs(flat_h).max(), 1e-6)
    print("loss %r vs %r; flat rel %g; %d ranges" % (loss_d, loss_h, rel, len(steps_h)))
    assert np.isfinite(loss_h) and abs(loss_d - loss_h) < 1e-5 * abs(loss_h)
    assert rel < 5e-4
    assert steps_d == steps_h and max(steps_h.values()) == 2           # the shared tensors stepped twice, a candidate layer once or twice


# ---- 5. the searcher ---------------------------------------------------------------------------------------------------------------------
SEARCH = ["--dataset", "tiny", "--synthetic", "tiny", "--maxlen", "12", "--eval_negative_sample_size", "16", "--dupe_factor", "1", "--prop_sliding_window", "0.5", "--num_layers", "2",
          "--hidden_units", "64", "--num_heads", "2", "--batch_size", "16", "--eval_batch_size", "24", "--precision", "f32"]


def test_searcher_on_resident_data_returns_the_host_records(tmp_path, monkeypatch):
    from adt_amd.bert4rec import evolution as ev
    monkeypatch.chdir(tmp_path)
    argv = SEARCH + ["--data_dir", str(tmp_path)]
    args = ev.parse_args(argv)
    ev.set_rng_seed(args.seed)
    plain = ev.SearcherEvolution(args)
    assert plain.dev_data is None and plain.train_ds is not None
    r = np.random.RandomState(2)
    cands = [[float(x) for x in r.rand(4)] for _ in range(5)]
    with pytest.raises(_lib.AdtError, match="resident data"):
        plain.evaluate_candidates(cands, device_batches=True)
    del plain

    def no_host_training_set(*a, **k):
        raise AssertionError("BertTrainDataset was constructed under --device_batches")
    monkeypatch.setattr(D, "BertTrainDataset", no_host_training_set)
    args = ev.parse_args(argv + ["--device_batches"])
    ev.set_rng_seed(args.seed)
    s = ev.SearcherEvolution(args)
    assert s.train_ds is None and len(s.dev_data) > 0 and not args.device_scores
    for ds in (s.val_ds, s.test_ds):
        n = len(ds)
        assert n > 2 * 24                                             # three batches of the 64 users
        host = s.evaluate_candidates(cands, ds, group=2, device_batches=False, device_scores=False)
        assert host == s.evaluate_candidates(cands, ds, group=2, device_scores=False)      # device_batches defaults to the flag: same ranks
        got = s.evaluate_candidates(cands, ds, group=2, device_batches=True, device_scores=True)
        mixed = s.evaluate_candidates(cands, ds, group=2, device_batches=False, device_scores=True)
        assert got == mixed and len(got) == 5
        for a, b in zip(host, got):
            print(ds.mode, a, b)
            assert set(a) == set(b) and a["V_HR"] == b["V_HR"]
            for key in ("V_NDCG", "V_AUC", "auc"):
                assert close(b[key], a[key], n), key
        assert len({h["V_AUC"] for h in host}) > 1
    # a warm-up epoch from the resident data, remasked: finite loss, every full batch stepped
    args.warmup_epochs, args.remask_every_epoch = 2, True
    s._train_warmup()
    assert np.isfinite(float(s.trainer.loss())) and max(s.trainer.steps.values()) == 2 * (len(s.dev_data) // 16)


# ---- 6. command lines --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra", [[], ["--device_batches", "--device_scores", "--device_negatives"]], ids=["host", "device"])
def test_evolution_cli(tmp_path, monkeypatch, extra):
    from adt_amd.bert4rec import evolution as ev
    monkeypatch.chdir(tmp_path)
    if extra:
        monkeypatch.setattr(D.PopularSampler, "get_negative_samples", lambda *a, **k: pytest.fail("the host sampler was called"))
    ev.main(SEARCH + ["--data_dir", str(tmp_path), "--out_dir", str(tmp_path / "res"), "--warmup_epochs", "1", "--search_epochs", "1",
                      "--population_num", "6", "--select_num", "3", "--crossover_num", "2", "--mutation_num", "2"] + extra)
    files = os.listdir(tmp_path / "res")
    assert len(files) == 1
    recs = [json.loads(l) for l in open(tmp_path / "res" / files[0])]
    assert len(recs) == 3
    for rec in recs:
        assert all(np.isfinite(rec[k]) and 0.0 <= rec[k] <= 1.0 for k in ("auc", "V_AUC", "V_HR", "V_NDCG"))


@pytest.mark.parametrize("extra", [["--device_scores"], ["--device_batches", "--device_scores", "--device_negatives"]], ids=["scores", "all"])
def test_main_cli(tmp_path, capsys, monkeypatch, extra):
    from adt_amd.bert4rec.main import main
    if "--device_negatives" in extra:
        monkeypatch.setattr(D.PopularSampler, "get_negative_samples", lambda *a, **k: pytest.fail("the host sampler was called"))
    main(["--dataset", "ml-1m", "--data_dir", str(tmp_path), "--synthetic", "tiny", "--template", "0", "--num_epochs", "1", "--maxlen", "16",
          "--batch_size", "32", "--eval_batch_size", "24", "--eval_negative_sample_size", "10", "--dupe_factor", "2", "--prop_sliding_window", "0.5",
          "--hidden_units", "64", "--inner_units", "96"] + extra)
    lines = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert len(lines) == 1 and lines[0]["epoch"] == 1 and np.isfinite(lines[0]["loss"])
    for split in ("valid", "test"):
        assert all(np.isfinite(lines[0][split][k]) and 0.0 <= lines[0][split][k] <= 1.0 for k in ("ndcg10", "hr10", "auc")), lines[0]
    assert lines[0]["valid"]["auc"] > 0.0


# ---- 7. two ranks ------------------------------------------------------------------------------------------------------------------------
def test_evaluate_device_scores_under_a_process_group(tmp_path):
    """Two gloo ranks sharing the GPU take batches r, r + 2, ... and sum-reduce the int64 histogram: every rank prints exactly the single
    process's metrics (tests/bert_devsearch_cases.py: dp_main).  Each process is started fresh."""
    script = os.path.join(REPO, "tests", "bert_devsearch_cases.py")
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
