"""CPU: the padded layout of SASRec-ADT widths that are not multiples of 64 (adt_amd/wide.py:padded_layout, lane_index) and the
unchanged numpy oracle against fixtures recorded from the imported reference at hidden_units 50 (one head; two heads of 25) and
100 (two heads of 50): tools/gen_golden.py oddwidth.  Bounds as tests/test_oracle_golden.py uses for sasrec_d256_h2."""
import numpy as np
import pytest

from oracle import sasrec_oracle as so
from tests.test_oracle_golden import close, load

ODD = ["sasrec_w50_h1", "sasrec_w50_h2", "sasrec_w100_h2"]


def test_padded_layout_table():
    from adt_amd.wide import padded_layout
    want = {(50, 1): (50, 64, 64), (50, 2): (25, 32, 64), (100, 1): (100, 128, 128), (100, 2): (50, 64, 128), (100, 4): (25, 32, 128),
            (200, 2): (100, 128, 256), (64, 2): (32, 32, 64), (128, 2): (64, 64, 128), (192, 3): (64, 64, 192), (256, 2): (128, 128, 256),
            (256, 1): (256, 256, 256), (150, 3): (50, 64, 192), (200, 1): (200, 256, 256)}
    for (d, H), w in want.items():
        assert padded_layout(d, H) == w, (d, H)


@pytest.mark.parametrize("d,H,words", [(50, 5, ("d=50", "H=5", "hd_pad=16", "d_pad=80")), (96, 3, ("d=96", "H=3", "hd_pad=32", "d_pad=96")),
                                       (50, 3, ("d=50", "H=3")), (300, 1, ("d=300", "H=1")), (320, 4, ("d_pad=512",))])
def test_padded_layout_refusals_name_the_shape_and_the_rule(d, H, words):
    from adt_amd._lib import AdtError
    from adt_amd.wide import padded_layout
    with pytest.raises(AdtError) as e:
        padded_layout(d, H)
    msg = str(e.value)
    for w in words + ("hd_pad", "d_pad"):
        assert w in msg, (w, msg)


@pytest.mark.parametrize("d,H", [(50, 1), (50, 2), (100, 2), (100, 4), (200, 2)])
def test_lane_index_round_trips_reference_shapes(d, H):
    """Scatter of reference-shaped parameters into the padded flat layout and back; everything not addressed is a pad lane or an
    alignment gap, and a padded (3 d_pad, d_pad) in_proj weight holds each head's rows and columns at its padded place."""
    from adt_amd.sasrec.model import param_table
    from adt_amd.wide import lane_index, padded_layout
    hd, hd_pad, dp = padded_layout(d, H)
    V, L, nl = 30, 12, 2
    ref, pad = param_table(V, L, d, H, nl), param_table(V, L, dp, H, nl)
    offs, o = {}, 0
    for n, s in pad:
        offs[n] = o
        o += (int(np.prod(s)) + 3) // 4 * 4
    idx = lane_index(ref, pad, offs, d, H)
    assert idx.size == sum(int(np.prod(s)) for _, s in ref) and np.unique(idx).size == idx.size and idx.max() < o
    r = np.random.RandomState(0)
    vals = r.randn(idx.size).astype(np.float32)
    flat = np.zeros(o, np.float32)
    flat[idx] = vals
    assert (flat[idx] == vals).all() and np.count_nonzero(flat) == np.count_nonzero(vals)
    k, name = 0, "encoder.encoder_layers.1.attention_layer.in_proj_weight"
    for n, s in ref:
        if n == name:
            break
        k += int(np.prod(s))
    W = vals[k:k + 3 * d * d].reshape(3 * d, d)
    Wp = flat[offs[name]:offs[name] + 3 * dp * dp].reshape(3, H, hd_pad, H, hd_pad)
    assert (Wp[:, :, :hd, :, :hd].reshape(3 * d, d) == W).all()
    assert np.count_nonzero(Wp) == np.count_nonzero(W)


@pytest.mark.parametrize("name", ODD)
def test_oracle_reproduces_the_odd_width_fixtures(golden_dir, name):
    from tools.gen_golden_inputs import make_batch, sample_idx
    z, cfg = load(golden_dir, name)
    assert cfg.hidden_units % 64 != 0 and cfg.num_layers == 2 and list(z["lam2"])[0] != list(z["lam2"])[1]
    seed, B = int(z["seed"]), int(z["B"])
    P = so.init_params(cfg, seed=seed)
    batch = make_batch(np.random.RandomState(seed + 1), B, cfg.maxlen, cfg.item_num)
    out = so.forward(P, cfg, *batch, training=True)
    close(out[0], z["pos_logits"], 5e-5, what="pos_logits")
    for i in range(cfg.num_layers):
        for nm, t in (("enc_in", out[2][i]), ("dec_out", out[3][i]), ("rec_ind", so.rec_reference_order(out[4][i]))):
            t = t.reshape(-1)
            close(t[sample_idx(t.size, 1024)], z["%s.%d.sample" % (nm, i)], 5e-5, what=nm)
    loss, parts, seeds = so.loss_and_seeds(P, cfg, out, batch[2], list(z["lam1"]), list(z["lam2"]), float(z["wd"]))
    assert abs(loss - float(z["loss"])) < 5e-5
    G = so.backward(P, cfg, out[5], seeds, float(z["wd"]))
    for k, _ in so.param_shapes(cfg):
        if "gnone." + k in z.files:
            assert G[k] is None
            continue
        t = G[k].reshape(-1)
        close(t[sample_idx(t.size)], z["gsample." + k], 1e-7, rtol=1e-3, what="grad sample " + k)
    assert abs(so.grad_norm(G) - float(z["total_norm"])) < 1e-4 * float(z["total_norm"])
    close(so.predict(P, cfg, batch[0], z["cand"]), z["predict_cand"], 2e-5, what="predict")
