"""CPU: the host side of SASRec-ADT's full-catalogue evaluation on the device -- full_metrics_from_hist against
metrics_from_stats(full_rank_stats(...)), the new flags of sasrec/main.py and sasrec/evolution.py, the new C symbols in the header and in
the ctypes table, and the refusals of the two launchers (they fail on their scalars before any pointer is looked at)."""
import ctypes
import os
import re

import numpy as np
import pytest

from adt_amd import _lib
from adt_amd.sasrec import utils as U

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def device_counts(ranks, nel, kh):
    """What adt_full_rank_stats leaves for one group: the histogram clipped at kh and the float64 sum of the AUC terms."""
    ok = ranks >= 0
    hist = np.bincount(np.minimum(ranks[ok], kh), minlength=kh + 1)
    return hist, float(((nel[ok] - ranks[ok]) / np.maximum(nel[ok], 1)).sum())


@pytest.mark.parametrize("N,kh", [(1, 10), (40, 10), (6040, 10), (6040, 128), (500, 5)])
def test_full_metrics_from_hist_equals_metrics_from_stats(N, kh):
    r = np.random.RandomState(N + kh)
    ranks = np.where(r.rand(N) < 0.5, r.randint(0, 12, N), r.randint(0, 3000, N)).astype(np.int64)
    nel = ranks + r.randint(0, 3000, N)
    nel[r.rand(N) < 0.05] = 0
    ranks[nel == 0] = 0
    ks = (5, 10) if kh >= 10 else (1, 5)
    (nd_w, hr_w), auc_w = U.metrics_from_stats(U.full_rank_stats(ranks, nel, ks), ks)
    hist, s = device_counts(ranks, nel, kh)
    (nd, hr), auc = U.full_metrics_from_hist(hist, s, ks)
    tol = N * 2.0 ** -52
    for k in ks:
        assert hr[k] == hr_w[k] and isinstance(hr[k], float)
        assert abs(nd[k] - nd_w[k]) <= tol * abs(nd_w[k])
    assert abs(auc - auc_w) <= tol * abs(auc_w)
    # a (1, kh + 1) row, as it is read back, serves too
    assert U.full_metrics_from_hist(hist[None], s, ks) == ((nd, hr), auc)


def test_full_metrics_from_hist_refuses_k_above_kh():
    hist = np.array([3, 2, 1, 0, 0, 4])      # kh = 5: ranks 0..4, then everything else
    (nd, hr), auc = U.full_metrics_from_hist(hist, 7.5, (5,))
    assert hr[5] == 6 / 10 and auc == 0.75
    with pytest.raises(ValueError, match="kh=5"):
        U.full_metrics_from_hist(hist, 7.5, (5, 10))
    with pytest.raises(ValueError, match="kh=5"):
        U.full_metrics_from_hist(hist, 7.5, (6,))


def test_main_flags():
    from adt_amd.sasrec import main as M
    base = ["--dataset", "ml-1m", "--train_dir", "x", "--no_template"]
    a = M.parse_args(base)
    assert a.device_eval_full is False and a.eval_full is False and a.device_eval is False
    a = M.parse_args(base + ["--eval_full", "true"])
    assert a.eval_full is True and a.device_eval_full is False      # --eval_full alone keeps the host path
    a = M.parse_args(base + ["--device_eval_full", "true"])
    assert a.device_eval_full is True and a.eval_full is True and a.device_eval is False and a.device_negatives is False
    a = M.parse_args(base + ["--device_eval_full", "true", "--device_eval", "true"])
    assert a.device_eval_full and a.eval_full and a.device_eval


def test_evolution_flags(capsys):
    from adt_amd.sasrec import evolution as ev
    a = ev.parse_args(["--dataset", "tiny"])
    assert a.eval_full is False and a.select_by == "auc" and a.device_eval is False
    a = ev.parse_args(["--dataset", "tiny", "--eval_full", "true"])
    assert a.eval_full is True and a.select_by == "auc" and a.device_eval is False
    a = ev.parse_args(["--dataset", "tiny", "--eval_full", "true", "--select_by", "ndcg"])
    assert a.eval_full is True and a.select_by == "ndcg"
    for argv in (["--select_by", "ndcg"], ["--select_by", "ndcg", "--eval_full", "false"], ["--select_by", "ndcg", "--device_eval", "true"]):
        with pytest.raises(SystemExit) as e:
            ev.parse_args(["--dataset", "tiny"] + argv)
        assert e.value.code == 2 and "--eval_full true" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        ev.parse_args(["--dataset", "tiny", "--select_by", "hr"])
    capsys.readouterr()


def test_new_symbols_in_the_header_and_in_signatures():
    src = open(os.path.join(REPO, "include", "adt_hip.h")).read()
    for name, n_args in (("adt_full_rank_groups", 24), ("adt_full_rank_stats", 8)):
        m = re.search(r"\bint %s\(([^;]*)\);" % name, src)
        assert m, name
        assert len(m.group(1).split(",")) == n_args
        res, argtypes = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and len(argtypes) == n_args
        assert hasattr(_lib.load(), name)
    assert _lib.SIGNATURES["adt_full_rank_groups"][1][18] is ctypes.c_int64      # ws_bytes


def test_launchers_reject_bad_arguments_without_a_launch():
    lib = _lib.load()
    fake = ctypes.c_void_p(4096)      # 16-byte aligned and never dereferenced: each call fails on its scalars (or on the NULL) first

    def groups(n_rows=15, R=5, d=64, ldf=64, lde=64, V=120, first_id=1, off=fake, items=fake, n_total=40, row0=0, K=0, splits=0, rank=fake):
        return lib.adt_full_rank_groups(fake, ldf, fake, lde, None, n_rows, R, d, V, first_id, fake, off, items, n_total, row0, K, splits, fake, 1 << 20,
                                        rank, fake, None, None, None)

    def stats(rank=fake, nel=fake, n_rows=10, rpg=5, kh=10, hist=fake, auc=fake):
        return lib.adt_full_rank_stats(rank, nel, n_rows, rpg, kh, hist, auc, None)
    for call, word in ((lambda: groups(R=0), "rows_per_group=0"), (lambda: groups(n_rows=16), "multiple"), (lambda: groups(row0=-1), "outside"),
                       (lambda: groups(row0=36), "outside"), (lambda: groups(n_total=4), "outside"), (lambda: groups(off=None), "go together"),
                       (lambda: groups(items=None), "go together"), (lambda: groups(first_id=2), "first_id"), (lambda: groups(K=129), "K=129"),
                       (lambda: groups(d=50, ldf=52, lde=52), "d=50"), (lambda: groups(ldf=60), "ldf"), (lambda: groups(V=0), "n_items"),
                       (lambda: groups(splits=1025), "splits"), (lambda: groups(rank=None), "missing output"), (lambda: groups(K=5), "missing output"),
                       (lambda: stats(kh=0), "kh=0"), (lambda: stats(kh=1025), "kh=1025"), (lambda: stats(rpg=0), "rows_per_group=0"),
                       (lambda: stats(rpg=3), "multiple"), (lambda: stats(rank=None), "NULL"), (lambda: stats(nel=None), "NULL"),
                       (lambda: stats(hist=None), "NULL"), (lambda: stats(auc=None), "NULL")):
        assert call() != 0
        assert word in lib.adt_last_error().decode(), (word, lib.adt_last_error().decode())
    assert groups(n_rows=0) == 0      # no rows: nothing to do
    assert lib.adt_full_rank_ws_bytes(15, 120, 10, 0) > 0
