"""Ranking a distance_metric='kl' STOSA-ADT model by the row-wise KL divergence, the parts that need no GPU.

The image identity adt_klrow_pack builds on, in float64 numpy: nu[u] - (A[u] . W[v] + bias[v]) is kl_distance (stosa/modules.py:45-50)
of the user's Gaussian from the item's, to 1e-12 relative to the magnitude of the summed terms.  Both command lines take --rowwise_eval with --distance_metric kl only and
still refuse kl with --fused_eval.  The C ABI entry is declared in the header and in SIGNATURES with matching arity, and the fixture
tests/golden/stosa_kl_rowwise.npz belongs to the model of stosa_kl_small.npz."""
import os
import re

import numpy as np
import pytest

pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def elu1_64(x):
    x = np.asarray(x, np.float64)
    return np.where(x > 0, x, np.expm1(np.minimum(x, 0.0))) + 1.0


def kl_direct64(sm, sc, Em, ci):
    """kl_distance of every (user, item) pair, float64: 0.5 (sum cu / ci + sum (mi - mu)^2 / ci - d + sum log ci - sum log cu)."""
    sm, sc, Em, ci = (np.asarray(x, np.float64) for x in (sm, sc, Em, ci))
    trace = sc @ (1.0 / ci).T
    mean = ((Em[None, :, :] - sm[:, None, :]) ** 2 / ci[None, :, :]).sum(-1)
    logdet = np.log(ci).sum(-1)[None, :] - np.log(sc).sum(-1)[:, None]
    return 0.5 * (trace + mean - sm.shape[1] + logdet)


def images64(sm, sc, Em, ci):
    """(A, nu, W, bias) of adt_klrow_pack in float64."""
    sm, sc, Em, ci = (np.asarray(x, np.float64) for x in (sm, sc, Em, ci))
    A = np.concatenate([sm * sm + sc, sm], 1)
    W = np.concatenate([-0.5 / ci, Em / ci], 1)
    bias = -0.5 * (np.log(ci).sum(1) + (Em * Em / ci).sum(1))
    nu = -0.5 * (sm.shape[1] + np.log(sc).sum(1))
    return A, nu, W, bias


@pytest.mark.parametrize("B,V,d", [(5, 203, 20), (21, 1003, 64)])
@pytest.mark.parametrize("scale", (0.02, 0.5, 1.0))
def test_image_identity_float64(B, V, d, scale):
    r = np.random.RandomState(B + V + d)
    Em, Ec, sm = (scale * r.standard_normal(s) for s in ((V, d), (V, d), (B, d)))
    sc = np.exp(scale * r.standard_normal((B, d)))
    ci = elu1_64(Ec)
    want = kl_direct64(sm, sc, Em, ci)
    A, nu, W, bias = images64(sm, sc, Em, ci)
    got = nu[:, None] - (A @ W.T + bias[None, :])
    # relative to the terms that are summed, entry by entry: float64's own forward bound is (2d + 8) 2^-53 T = 1.5e-14 T at d = 64.  At
    # scale 0.02 the divergences are ~1e-2 while nu, bias and A . W are ~d / 2 each, so no float64 sum holds 1e-12 of the RESULT there.
    T = np.abs(A) @ np.abs(W).T + np.abs(bias)[None, :] + np.abs(nu)[:, None]
    err = (np.abs(got - want) / T).max()
    print("identity B=%d V=%d d=%d scale %g: %.3g of T, %.3g of the largest divergence" % (B, V, d, scale, err, np.abs(got - want).max() / np.abs(want).max()))
    assert err <= 1e-12, err
    if scale >= 0.5:          # divergences of the order of T: the same bound against the result itself
        assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    assert (want >= -1e-12 * np.abs(want).max()).all()          # a divergence


@pytest.mark.parametrize("mod", ("main", "evolution"))
def test_parse_args_rowwise_eval(mod, capsys):
    parse_args = getattr(__import__("adt_amd.stosa." + mod, fromlist=["parse_args"]), "parse_args")
    assert not parse_args([]).rowwise_eval
    a = parse_args(["--distance_metric", "kl", "--rowwise_eval"])
    assert a.distance_metric == "kl" and a.rowwise_eval and not a.fused_eval
    assert parse_args(["--distance_metric", "kl", "--rowwise_eval", "--device_batches", "--device_scores"]).device_scores
    for argv, word in ((["--rowwise_eval"], "--rowwise_eval"), (["--distance_metric", "wasserstein", "--rowwise_eval"], "--rowwise_eval"),
                       (["--distance_metric", "kl", "--fused_eval"], "--fused_eval"),
                       (["--distance_metric", "kl", "--rowwise_eval", "--fused_eval"], "--fused_eval")):
        with pytest.raises(SystemExit) as e:
            parse_args(argv)
        assert e.value.code == 2 and word in capsys.readouterr().err, argv
    assert parse_args(["--fused_eval"]).fused_eval          # Wasserstein: as before


@pytest.mark.parametrize("mod", ("main", "evolution"))
def test_help_says_not_the_reference_metrics(mod, capsys):
    parse_args = getattr(__import__("adt_amd.stosa." + mod, fromlist=["parse_args"]), "parse_args")
    with pytest.raises(SystemExit):
        parse_args(["--help"])
    text = " ".join(capsys.readouterr().out.split())
    assert "NOT the reference's kl_predict_full metrics" in text


def test_klrow_pack_declared():
    from adt_amd import _lib
    assert "adt_klrow_pack" in _lib.SIGNATURES
    res, args = _lib.SIGNATURES["adt_klrow_pack"]
    header = open(os.path.join(ROOT, "include", "adt_hip.h")).read()
    decl = re.search(r"\bint\s+adt_klrow_pack\s*\(([^)]*)\)\s*;", header)
    assert decl, "adt_klrow_pack is not declared in include/adt_hip.h"
    params = [p.strip() for p in decl.group(1).split(",")]
    assert len(params) == len(args) == 10
    assert [p.split()[-1].lstrip("*") for p in params] == ["M", "C", "ld", "rows", "d", "items", "img", "ldi", "off", "stream"]


def test_rowwise_fixture_belongs_to_kl_small():
    gold = os.path.join(ROOT, "tests", "golden")
    g, s = np.load(os.path.join(gold, "stosa_kl_rowwise.npz")), np.load(os.path.join(gold, "stosa_kl_small.npz"))
    assert int(g["seed"]) == int(s["seed"]) and np.array_equal(g["cfg"], s["cfg"]) and np.array_equal(g["input_ids"], s["input_ids"])
    V, d, B = int(g["cfg"][0]), int(g["cfg"][2]), len(g["input_ids"])
    assert g["rowwise_dist"].shape == (B, V) and g["last_mean"].shape == g["last_cov"].shape == (B, d)
    assert np.isfinite(g["rowwise_dist"]).all() and (g["last_cov"] > 0).all()
    assert os.path.getsize(os.path.join(gold, "stosa_kl_rowwise.npz")) < 64 * 1024
