"""GPU: the grouped KL full sort on a packed item image (adt_amd/csrc/adt_kldist_groups.cuh through the C ABI).

adt_kldist_pack against float64 (1e-6 relative: one fp32 reciprocal per entry, 64 fp32 logs per sum).  adt_kldist_full_groups on P
stacked groups of E users: against a float64 restatement of the reference's kl_predict_full (stosa/trainer.py:481-511, with
kl_distance_matmul's broadcasts, stosa/modules.py:52-70) applied to each group on its own, at the bound of the existing kldist_full
test (1e-4 of the largest distance); against P separate ops.kldist_full calls -- the only correct route before this kernel -- at
1e-5 of the largest distance (the bound of test_batched_candidates_superstosa: both are fp32 sums of the same 2d + 2 terms, one with
a packed reciprocal where the other divides); and two runs bit for bit.  Inputs have the magnitudes of
test_kl_bpr_and_full_sort_kernels.  Shapes: E dividing V and not, E > V, exactly one 16-user tile with a ragged chunk, a ragged user
tile, several item tiles per wave, state rows that are column views of a wider buffer, and a width that is no multiple of 32."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SHAPES = [(1, 5, 40, 64, False), (3, 4, 40, 64, False), (2, 8, 300, 64, False), (2, 3, 2, 64, False), (4, 16, 37, 32, False),
          (2, 17, 50, 64, False), (3, 5, 40, 64, True), (2, 5, 23, 36, False)]


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
    """kl_predict_full (stosa/trainer.py:481-511) of ONE eval batch: pad the items to a multiple of E = len(sm) with zero means and unit
    covariances, score the E users against every E-item chunk."""
    E, (V, d) = sm.shape[0], Em.shape
    pad = E - V % E
    sm, sc = sm.astype(np.float64), sc.astype(np.float64)
    cm = np.concatenate([Em.astype(np.float64), np.zeros((pad, d))])
    cc = np.concatenate([elu1_64(Ec), np.ones((pad, d))])
    out = np.concatenate([kl_matmul64(sm, sc, cm[s0:s0 + E], cc[s0:s0 + E]) for s0 in range(0, cm.shape[0], E)], 1)
    return out[:, :V]


def inputs(P, E, V, d, seed):
    r = np.random.RandomState(seed)
    Em, Ec = (0.3 * r.standard_normal((V, d))).astype(np.float32), (0.3 * r.standard_normal((V, d))).astype(np.float32)
    sm = (0.3 * r.standard_normal((P * E, d))).astype(np.float32)
    sc = np.exp(0.2 * r.standard_normal((P * E, d))).astype(np.float32)
    return Em, Ec, sm, sc


@pytest.mark.parametrize("V,d", [(40, 64), (37, 32), (300, 64), (2, 68)])
def test_kldist_pack(V, d):
    from adt_amd import ops
    Em, Ec, _, _ = inputs(1, 1, V, d, V + d)
    img, lv = ops.kldist_pack(T_(Em), T_(Ec))
    img2, lv2 = ops.kldist_pack(T_(Em), T_(Ec))
    assert img.shape == (V, 2 * d) and lv.shape == (V,)
    assert torch.equal(img, img2) and torch.equal(lv, lv2)
    img, lv = img.cpu().numpy(), lv.cpu().numpy()
    ci = elu1_64(Ec)
    assert np.array_equal(img[:, :d], Em)
    e_img, e_lv = rel(img[:, d:], 1.0 / ci), rel(lv, np.log(ci).sum(1))
    print("kldist_pack V=%d d=%d: rinv %.3g lv %.3g" % (V, d, e_img, e_lv))
    assert e_img < 1e-6 and e_lv < 1e-6
    # tables that are column views of a wider buffer: the same image
    wide_m, wide_c = torch.zeros(V, 3 * d, device="cuda:0"), torch.zeros(V, 3 * d, device="cuda:0")
    wide_m[:, d:2 * d], wide_c[:, d:2 * d] = T_(Em), T_(Ec)
    img3, lv3 = ops.kldist_pack(wide_m[:, d:2 * d], wide_c[:, d:2 * d])
    assert torch.equal(img3, img2) and torch.equal(lv3, lv2)


@pytest.mark.parametrize("P,E,V,d,views", SHAPES)
def test_kldist_full_groups(P, E, V, d, views):
    from adt_amd import ops
    Em, Ec, sm, sc = inputs(P, E, V, d, 1000 * E + V + P)
    dEm, dEc = T_(Em), T_(Ec)
    if views:
        bm, bc = torch.full((P * E, 3 * d), float("nan"), device="cuda:0"), torch.full((P * E, 3 * d), float("nan"), device="cuda:0")
        bm[:, d:2 * d], bc[:, d:2 * d] = T_(sm), T_(sc)
        dsm, dsc = bm[:, d:2 * d], bc[:, d:2 * d]
        assert dsm.stride(0) == 3 * d
    else:
        dsm, dsc = T_(sm), T_(sc)
    img, lv = ops.kldist_pack(dEm, dEc)
    got_t = ops.kldist_full_groups(dsm, dsc, img, lv, E, V)
    again = ops.kldist_full_groups(dsm, dsc, img, lv, E, V)
    assert got_t.shape == (P * E, V) and torch.equal(got_t, again)
    got = got_t.cpu().numpy()
    assert np.isfinite(got).all()
    want = np.concatenate([kl_full_ref(sm[g * E:(g + 1) * E], sc[g * E:(g + 1) * E], Em, Ec) for g in range(P)])
    loop = torch.cat([ops.kldist_full(T_(sm[g * E:(g + 1) * E]), T_(sc[g * E:(g + 1) * E]), dEm, dEc, V) for g in range(P)]).cpu().numpy()
    e64, eloop = rel(got, want), np.abs(got - loop).max() / np.abs(loop).max()
    print("kldist_full_groups P=%d E=%d V=%d d=%d: vs float64 %.3g, vs the loop of kldist_full %.3g" % (P, E, V, d, e64, eloop))
    assert e64 < 1e-4
    assert eloop <= 1e-5
    if P > 1:      # the group rule itself: chunking the stack by P * E is a different function
        mixed = kl_full_ref(sm, sc, Em, Ec)
        assert rel(mixed[E:], want[E:]) > 1e-3


def test_kldist_full_groups_past_2_31_entries():
    """rows * V = 32,800 * 65,537 > 2^31 entries (8.6 GB; d = 4 keeps the arithmetic small): the output is indexed in size_t.  The last
    group, whose rows lie wholly past entry 2^31, and the first one against adt_kldist_full on those 16 rows alone."""
    from adt_amd import ops
    P, E, V, d = 2050, 16, 65537, 4
    assert (P - 1) * E * V > 2 ** 31
    Em, Ec, sm, sc = inputs(P, E, V, d, 11)
    dEm, dEc, dsm, dsc = T_(Em), T_(Ec), T_(sm), T_(sc)
    img, lv = ops.kldist_pack(dEm, dEc)
    dist = ops.kldist_full_groups(dsm, dsc, img, lv, E, V)
    assert dist.shape == (P * E, V)
    for g in (0, P // 2, P - 1):
        one = ops.kldist_full(dsm[g * E:(g + 1) * E], dsc[g * E:(g + 1) * E], dEm, dEc, V)
        e = float((dist[g * E:(g + 1) * E] - one).abs().max() / one.abs().max())
        assert e <= 1e-5, (g, e)
    del dist
    torch.cuda.empty_cache()


def test_kldist_groups_launcher_refusals():
    from adt_amd import _lib, ops
    Em, Ec, sm, sc = inputs(2, 4, 20, 64, 3)
    img, lv = ops.kldist_pack(T_(Em), T_(Ec))
    dsm, dsc = T_(sm), T_(sc)
    ops.kldist_full_groups(dsm, dsc, img, lv, 4, 20)                       # fine
    with pytest.raises(_lib.AdtError):
        ops.kldist_full_groups(dsm, dsc, img, lv, 3, 20)                   # rows = 8 is no multiple of E = 3
    with pytest.raises(_lib.AdtError):
        ops.kldist_full_groups(dsm, dsc, img, lv, 0, 20)                   # E < 1
    with pytest.raises(_lib.AdtError):                                     # d % 4 != 0
        ops.kldist_full_groups(dsm[:, :62], dsc[:, :62], img[:, :124], lv, 4, 20)
    with pytest.raises(_lib.AdtError):
        ops.kldist_pack(T_(Em)[:, :62], T_(Ec)[:, :62])                    # d % 4 != 0
    lib = _lib.load()
    dist = torch.empty(8, 20, device="cuda:0")
    args = lambda smp, rows, E, d: (smp, ops._p(dsc), 64, ops._p(img), 128, ops._p(lv), rows, E, 20, d, ops._p(dist), 20, ops._stream())
    assert lib.adt_kldist_full_groups(*args(ops._p(dsm), 8, 4, 64)) == 0
    assert lib.adt_kldist_full_groups(*args(None, 8, 4, 64)) != 0 and b"missing" in lib.adt_last_error()      # a NULL operand
    assert lib.adt_kldist_full_groups(*args(ops._p(dsm), 7, 4, 64)) != 0 and b"multiple of E" in lib.adt_last_error()
    assert lib.adt_kldist_full_groups(*args(ops._p(dsm), 8, 4, 62)) != 0 and b"multiple of 4" in lib.adt_last_error()
    assert lib.adt_kldist_full_groups(*args(ops._p(dsm.view(-1)[1:]), 4, 4, 64)) != 0 and b"aligned" in lib.adt_last_error()
    big = (ops._p(dsm), ops._p(dsc), 64, ops._p(img), 128, ops._p(lv), 8, 4, 2 ** 31 - 1, 64, ops._p(dist), 2 ** 31 - 1, ops._stream())
    assert lib.adt_kldist_full_groups(*big) != 0 and b"index range" in lib.adt_last_error()              # v = cE + j would leave int
    torch.cuda.synchronize()
