"""GPU: the grouped KL full sort on padded rows (adt_amd/csrc/adt_kldist_groups_lanes.cuh through the C ABI).

adt_kldist_pack_lanes / adt_kldist_full_groups_lanes against the float64 restatement of kl_predict_full that
tests/test_stosa_klgroups_hip.py holds the tiled kernels to, applied to the LIVE lanes at the true width d = H * hd, at that test's bounds:
1e-6 for the image and lv, 1e-4 of the largest distance.  The padded inputs carry +0.0 on every pad lane of the state means AND of the
state covariances (log 0 = -inf for a kernel that summed them), and the item tables' pad lanes are +0.0 too (ELU(0) + 1 = 1): every
output must be finite.  Layouts 50/1, 100/2 (two heads of 50 in 64 lanes), 48/4 (four heads of 12 in 16 lanes) and 100/1 in 128 lanes;
E under a 16-user tile, exactly one, across one, and 130 (nine item tiles: wave 0 takes a second pair); V 42 and 301, neither a multiple
of any E; one group and three; state rows that are column views of a wider buffer."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

LANES = [(1, 50, 64), (2, 50, 64), (4, 12, 16), (1, 100, 128)]
CASES = [(ln, E, V, P) for ln in LANES for E in (3, 16, 17, 130) for V in (42, 301) for P in (1, 3)]


def T_(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-6)


def elu1_64(x):
    x = np.asarray(x, np.float64)
    return np.where(x > 0, x, np.expm1(np.minimum(x, 0.0))) + 1.0


def kl_matmul64(m1, c1, m2, c2):
    """kl_distance_matmul (stosa/modules.py:52-70) on (n, d) x (n, d) -> (n, n) in float64, log(prod) as sum(log)."""
    logdet = np.log(c2).sum(-1)[None, :] - np.log(c1).sum(-1)[:, None]
    mean = ((m1 - m2) ** 2) @ (1.0 / c2).T
    trace = (1.0 / c2) @ c1.T
    return (logdet + mean + trace - m1.shape[-1]) / 2


def kl_full_ref(sm, sc, Em, Ec):
    """kl_predict_full (stosa/trainer.py:481-511) of ONE eval batch at the true width: pad the items to a multiple of E = len(sm) with zero
    means and unit covariances, score the E users against every E-item chunk."""
    E, (V, d) = sm.shape[0], Em.shape
    pad = E - V % E
    sm, sc = sm.astype(np.float64), sc.astype(np.float64)
    cm = np.concatenate([Em.astype(np.float64), np.zeros((pad, d))])
    cc = np.concatenate([elu1_64(Ec), np.ones((pad, d))])
    out = np.concatenate([kl_matmul64(sm, sc, cm[s0:s0 + E], cc[s0:s0 + E]) for s0 in range(0, cm.shape[0], E)], 1)
    return out[:, :V]


def live_cols(lanes):
    H, hd, hd_pad = lanes
    return np.concatenate([np.arange(h * hd_pad, h * hd_pad + hd) for h in range(H)])


def pad_rows(x, lanes):
    """(n, H * hd) -> (n, H * hd_pad), +0.0 on the pad lanes."""
    H, hd, hd_pad = lanes
    out = np.zeros((x.shape[0], H * hd_pad), np.float32)
    out[:, live_cols(lanes)] = x
    return out


def inputs(P, E, V, d, seed):
    r = np.random.RandomState(seed)
    Em, Ec = (0.3 * r.standard_normal((V, d))).astype(np.float32), (0.3 * r.standard_normal((V, d))).astype(np.float32)
    sm = (0.3 * r.standard_normal((P * E, d))).astype(np.float32)
    sc = np.exp(0.2 * r.standard_normal((P * E, d))).astype(np.float32)
    return Em, Ec, sm, sc


@pytest.mark.parametrize("lanes", LANES)
@pytest.mark.parametrize("V", [42, 301])
def test_kldist_pack_lanes(lanes, V):
    from adt_amd import ops
    H, hd, hd_pad = lanes
    d, dp, live = H * hd, H * hd_pad, live_cols(lanes)
    Em, Ec, _, _ = inputs(1, 1, V, d, V + d)
    pEm, pEc = T_(pad_rows(Em, lanes)), T_(pad_rows(Ec, lanes))
    img, lv = ops.kldist_pack_lanes(pEm, pEc, lanes)
    img2, lv2 = ops.kldist_pack_lanes(pEm, pEc, lanes)
    assert img.shape == (V, 2 * dp) and lv.shape == (V,)
    assert torch.equal(img, img2) and torch.equal(lv, lv2)
    img, lv = img.cpu().numpy(), lv.cpu().numpy()
    ci = elu1_64(Ec)
    assert np.array_equal(img[:, :dp][:, live], Em)
    e_img, e_lv = rel(img[:, dp:][:, live], 1.0 / ci), rel(lv, np.log(ci).sum(1))
    print("kldist_pack_lanes V=%d %s: rinv %.3g lv %.3g" % (V, lanes, e_img, e_lv))
    assert e_img < 1e-6 and e_lv < 1e-6
    pad = np.setdiff1d(np.arange(dp), live)
    for half in (img[:, :dp], img[:, dp:]):      # +0.0 bit for bit on the pad lanes of both halves
        assert not half[:, pad].view(np.uint32).any()
    # pad lanes of the tables that are NOT zero stay out of the image and of lv all the same
    dirty_m, dirty_c = pEm.clone(), pEc.clone()
    if len(pad):
        dirty_m[:, T_(pad)], dirty_c[:, T_(pad)] = 7.0, -3.0
    img3, lv3 = ops.kldist_pack_lanes(dirty_m, dirty_c, lanes)
    assert torch.equal(img3, img2) and torch.equal(lv3, lv2)


@pytest.mark.parametrize("lanes,E,V,P", CASES)
def test_kldist_full_groups_lanes(lanes, E, V, P):
    from adt_amd import ops
    H, hd, hd_pad = lanes
    d, dp = H * hd, H * hd_pad
    Em, Ec, sm, sc = inputs(P, E, V, d, 1000 * E + V + P + hd)
    psm, psc = pad_rows(sm, lanes), pad_rows(sc, lanes)
    pad = np.setdiff1d(np.arange(dp), live_cols(lanes))
    assert not psc[:, pad].view(np.uint32).any() and not psm[:, pad].view(np.uint32).any()      # +0.0: log would be -inf
    # strided state rows: column views of a wider buffer whose other columns are NaN
    bm, bc = torch.full((P * E, 3 * dp), float("nan"), device="cuda:0"), torch.full((P * E, 3 * dp), float("nan"), device="cuda:0")
    bm[:, dp:2 * dp], bc[:, dp:2 * dp] = T_(psm), T_(psc)
    dsm, dsc = bm[:, dp:2 * dp], bc[:, dp:2 * dp]
    assert dsm.stride(0) == 3 * dp
    img, lv = ops.kldist_pack_lanes(T_(pad_rows(Em, lanes)), T_(pad_rows(Ec, lanes)), lanes)
    got_t = ops.kldist_full_groups_lanes(dsm, dsc, img, lv, E, V, lanes)
    again = ops.kldist_full_groups_lanes(T_(psm), T_(psc), img, lv, E, V, lanes)      # contiguous rows, and a second run: bit for bit
    assert got_t.shape == (P * E, V) and torch.equal(got_t, again)
    got = got_t.cpu().numpy()
    assert np.isfinite(got).all()
    want = np.concatenate([kl_full_ref(sm[g * E:(g + 1) * E], sc[g * E:(g + 1) * E], Em, Ec) for g in range(P)])
    e64 = rel(got, want)
    print("kldist_full_groups_lanes %s E=%d V=%d P=%d: vs float64 %.3g" % (lanes, E, V, P, e64))
    assert e64 < 1e-4


@pytest.mark.parametrize("H,hd", [(1, 64), (4, 16), (2, 64)])
@pytest.mark.parametrize("E,V,P", [(3, 42, 3), (17, 301, 1), (130, 301, 3)])
def test_unpadded_heads_equal_the_tiled_kernel(H, hd, E, V, P):
    """hd == hd_pad: no pad lane, the function of adt_kldist_pack + adt_kldist_full_groups."""
    from adt_amd import ops
    d, lanes = H * hd, (H, hd, hd)
    Em, Ec, sm, sc = inputs(P, E, V, d, E + V + d)
    dEm, dEc, dsm, dsc = T_(Em), T_(Ec), T_(sm), T_(sc)
    img, lv = ops.kldist_pack(dEm, dEc)
    limg, llv = ops.kldist_pack_lanes(dEm, dEc, lanes)
    assert rel(limg.cpu().numpy(), img.cpu().numpy()) < 1e-6 and rel(llv.cpu().numpy(), lv.cpu().numpy()) < 1e-6
    tiled = ops.kldist_full_groups(dsm, dsc, img, lv, E, V).cpu().numpy()
    got = ops.kldist_full_groups_lanes(dsm, dsc, limg, llv, E, V, lanes).cpu().numpy()
    e = rel(got, tiled)
    print("kldist_full_groups_lanes H=%d hd=%d E=%d V=%d P=%d: vs the tiled kernel %.3g" % (H, hd, E, V, P, e))
    assert e < 1e-4


def test_kldist_groups_lanes_launcher_refusals():
    from adt_amd import _lib, ops
    lanes = (1, 50, 64)
    Em, Ec, sm, sc = inputs(2, 4, 20, 50, 3)
    pEm, pEc, dsm, dsc = (T_(pad_rows(x, lanes)) for x in (Em, Ec, sm, sc))
    img, lv = ops.kldist_pack_lanes(pEm, pEc, lanes)
    ops.kldist_full_groups_lanes(dsm, dsc, img, lv, 4, 20, lanes)                       # fine
    with pytest.raises(_lib.AdtError):
        ops.kldist_full_groups_lanes(dsm, dsc, img, lv, 3, 20, lanes)                   # rows = 8 is no multiple of E = 3
    with pytest.raises(_lib.AdtError):
        ops.kldist_full_groups_lanes(dsm, dsc, img, lv, 0, 20, lanes)                   # E < 1
    with pytest.raises(_lib.AdtError):
        ops.kldist_full_groups_lanes(dsm, dsc, img, lv, 4, 20, (2, 50, 64))             # H * hd_pad = 128 != the row of 64
    with pytest.raises(_lib.AdtError):
        ops.kldist_full_groups_lanes(dsm, dsc, img, lv, 4, 20, (1, 50, 48))             # hd_pad no power of two
    with pytest.raises(_lib.AdtError):
        ops.kldist_pack_lanes(pEm, pEc, (2, 50, 64))                                    # H * hd_pad != the row
    with pytest.raises(_lib.AdtError):
        ops.kldist_pack_lanes(pEm, pEc, (1, 65, 64))                                    # hd > hd_pad
    lib = _lib.load()
    dist = torch.empty(8, 20, device="cuda:0")
    args = lambda smp, rows, E, d, ln=(1, 50, 64): (smp, ops._p(dsc), 64, ops._p(img), 128, ops._p(lv), rows, E, 20, d, *ln, ops._p(dist), 20,
                                                    ops._stream())
    assert lib.adt_kldist_full_groups_lanes(*args(ops._p(dsm), 8, 4, 64)) == 0
    assert lib.adt_kldist_full_groups_lanes(*args(None, 8, 4, 64)) != 0 and b"missing" in lib.adt_last_error()      # a NULL operand
    assert lib.adt_kldist_full_groups_lanes(*args(ops._p(dsm), 7, 4, 64)) != 0 and b"multiple of E" in lib.adt_last_error()
    assert lib.adt_kldist_full_groups_lanes(*args(ops._p(dsm), 8, 0, 64)) != 0 and b"E=0" in lib.adt_last_error()
    assert lib.adt_kldist_full_groups_lanes(*args(ops._p(dsm), 8, 4, 128)) != 0 and b"padded row" in lib.adt_last_error()
    assert lib.adt_kldist_full_groups_lanes(*args(ops._p(dsm), 8, 4, 64, (1, 50, 32))) != 0 and b"lanes" in lib.adt_last_error()
    assert lib.adt_kldist_full_groups_lanes(*args(ops._p(dsm.view(-1)[1:]), 4, 4, 64)) != 0 and b"aligned" in lib.adt_last_error()
    short = (ops._p(dsm), ops._p(dsc), 60, ops._p(img), 128, ops._p(lv), 8, 4, 20, 64, 1, 50, 64, ops._p(dist), 20, ops._stream())
    assert lib.adt_kldist_full_groups_lanes(*short) != 0 and b"lds=60" in lib.adt_last_error()              # a row stride under d_pad
    big = (ops._p(dsm), ops._p(dsc), 64, ops._p(img), 128, ops._p(lv), 8, 4, 2 ** 31 - 1, 64, 1, 50, 64, ops._p(dist), 2 ** 31 - 1, ops._stream())
    assert lib.adt_kldist_full_groups_lanes(*big) != 0 and b"index range" in lib.adt_last_error()           # v = cE + j would leave int
    torch.cuda.synchronize()
