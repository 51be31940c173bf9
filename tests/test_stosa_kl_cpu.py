"""distance_metric handling of the STOSA-ADT model, supernet and CLI that needs no GPU: the supernet (whose loss and full-sort paths
are Wasserstein-only) refuses 'kl' at construction, the model refuses unknown metrics, and the CLI offers both metrics."""
import pytest

pytest.importorskip("torch")


class Args:
    pass


def _args(metric):
    a = Args()
    a.device, a.item_size, a.maxlen, a.hidden_units, a.num_heads, a.num_layers, a.num_users = "cpu", 30, 10, 64, 4, 1, 2
    a.dropout, a.attention_dropout, a.pvn_weight, a.precision, a.distance_metric = 0.0, 0.0, 0.1, "f32", metric
    return a


def test_supernet_rejects_kl():
    from adt_amd._lib import AdtError
    from adt_amd.stosa.supernet import DisenDistSASupernet
    with pytest.raises(AdtError, match="wasserstein"):
        DisenDistSASupernet(_args("kl"), [0.0, 0.5], [0.0, 0.5])


def test_model_rejects_unknown_metric():
    from adt_amd._lib import AdtError
    from adt_amd.stosa.models import DisenDistSAModel
    with pytest.raises(AdtError, match="distance_metric"):
        DisenDistSAModel(_args("cosine"))


def test_cli_offers_kl():
    from adt_amd.stosa.main import parse_args
    assert parse_args(["--distance_metric", "kl"]).distance_metric == "kl"
    assert parse_args([]).distance_metric == "wasserstein"
