"""GPU: the three evolution entry points at the shapes their main.py siblings train and the searches used to refuse (DESIGN.md section
30): one tiny run each through evolution.main() -- two warm-up epochs, a population of 4, one search epoch -- and the result file with
finite scores.  SASRec-ADT at the CLI default width 50 / 1 and at 64 / 2 with maxlen 300 (the streamed attention); BERT4Rec-ADT at
50 / 1 on device-resident batches and scores; STOSA-ADT at 50 / 1 under both metrics on device-resident batches and scores, and at
128 / 1 (one head of 128 lanes) under Wasserstein."""
import glob
import json

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SEARCH = ["--warmup_epochs", "2", "--search_epochs", "1", "--population_num", "4", "--select_num", "2", "--crossover_num", "1", "--mutation_num", "1",
          "--num_layers", "1", "--batch_size", "16", "--eval_batch_size", "32"]


def _records(tmp_path, key):
    files = glob.glob(str(tmp_path / "res" / "*.jsonl"))
    assert len(files) == 1, files
    recs = [json.loads(l) for l in open(files[0])]
    assert 1 <= len(recs) <= 2
    for r in recs:
        assert np.isfinite(r[key]) and 0.0 <= r[key] <= 1.0, r
        assert len(json.loads(r["cand"])) == 2 and len(json.loads(r["rec"])) == 1 and len(json.loads(r["ind"])) == 1
    return recs


@pytest.mark.parametrize("d,H,L,extra", [(50, 1, 50, []), (64, 2, 300, []), (50, 1, 50, ["--device_negatives", "true"])])
def test_sasrec_evolution_lanes(tmp_path, monkeypatch, d, H, L, extra):
    from adt_amd.sasrec import evolution as ev
    monkeypatch.chdir(tmp_path)
    ev.main(["--dataset", "tiny", "--data_dir", str(tmp_path), "--synthetic", "tiny", "--maxlen", str(L), "--sample_size", "20", "--hidden_units", str(d),
             "--num_heads", str(H), "--out_dir", str(tmp_path / "res")] + extra + SEARCH)
    _records(tmp_path, "auc")


def test_bert_evolution_lanes(tmp_path, monkeypatch):
    from adt_amd.bert4rec import evolution as ev
    monkeypatch.chdir(tmp_path)
    ev.main(["--dataset", "tiny", "--data_dir", str(tmp_path), "--synthetic", "tiny", "--maxlen", "20", "--eval_negative_sample_size", "20",
             "--dupe_factor", "1", "--hidden_units", "50", "--num_heads", "1", "--device_batches", "--device_scores",
             "--out_dir", str(tmp_path / "res")] + SEARCH)
    _records(tmp_path, "auc")


@pytest.mark.parametrize("d,metric,device", [(50, "wasserstein", True), (50, "kl", True), (128, "wasserstein", False)])
def test_stosa_evolution_lanes(tmp_path, monkeypatch, d, metric, device):
    from adt_amd.stosa import evolution as ev
    from adt_amd.stosa.main import _write_synthetic
    monkeypatch.chdir(tmp_path)
    _write_synthetic(str(tmp_path / "Tiny.txt"), users=96, items=150, seed=3)        # --synthetic 1 keeps a file that is there
    ev.main(["--dataset", "Tiny", "--data_dir", str(tmp_path) + "/", "--synthetic", "1", "--maxlen", "20", "--hidden_units", str(d), "--num_heads", "1",
             "--distance_metric", metric, "--out_dir", str(tmp_path / "res")] + (["--device_batches", "--device_scores"] if device else []) + SEARCH)
    _records(tmp_path, "MRR")
