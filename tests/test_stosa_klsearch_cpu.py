"""The command line of the STOSA-ADT search (adt_amd/stosa/evolution.py) under distance_metric 'kl': the reference's flag
(stosa/evolution.py:51) is accepted, the fused evaluation -- Wasserstein only -- is refused with it, and an unknown metric stays an
error.  The supernet takes 'kl' only with allow_kl=True (without it the constructor refuses as before:
tests/test_stosa_kl_cpu.py), and a metric that is neither still raises through the base class.  No GPU: only the parser and the
constructor's argument checks run."""
import pytest

pytest.importorskip("torch")


class Args:
    pass


def test_supernet_allow_kl_still_rejects_unknown_metric():
    from adt_amd._lib import AdtError
    from adt_amd.stosa import supernet
    a = Args()
    a.device, a.item_size, a.maxlen, a.hidden_units, a.num_heads, a.num_layers, a.num_users = "cpu", 30, 10, 64, 4, 1, 2
    a.dropout, a.attention_dropout, a.pvn_weight, a.precision, a.distance_metric = 0.0, 0.0, 0.1, "f32", "cosine"
    with pytest.raises(AdtError, match="distance_metric"):
        supernet.DisenDistSASupernet(a, [0.0, 0.5], [0.0, 0.5], allow_kl=True)
    a.distance_metric = "kl"
    with pytest.raises(AdtError, match="allow_kl"):          # opt-in: the plain call refuses 'kl' and says how to ask for it
        supernet.DisenDistSASupernet(a, [0.0, 0.5], [0.0, 0.5])
    assert hasattr(supernet.DisenDistSASupernet, "kl_item_image")


def test_parse_args_accepts_kl():
    from adt_amd.stosa.evolution import parse_args
    assert parse_args([]).distance_metric == "wasserstein"
    a = parse_args(["--distance_metric", "kl", "--device_batches", "--device_scores"])
    assert a.distance_metric == "kl" and a.device_batches and a.device_scores and not a.fused_eval
    assert parse_args(["--distance_metric", "wasserstein", "--fused_eval"]).fused_eval


def test_parse_args_rejects_kl_with_fused_eval(capsys):
    from adt_amd.stosa.evolution import parse_args
    with pytest.raises(SystemExit) as e:
        parse_args(["--distance_metric", "kl", "--fused_eval"])
    assert e.value.code == 2 and "--fused_eval" in capsys.readouterr().err


def test_parse_args_rejects_unknown_metric():
    from adt_amd.stosa.evolution import parse_args
    with pytest.raises(SystemExit) as e:
        parse_args(["--distance_metric", "cosine"])
    assert e.value.code == 2
