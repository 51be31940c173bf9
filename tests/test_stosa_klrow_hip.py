"""GPU: full-catalogue ranking of a distance_metric='kl' STOSA-ADT model by the ROW-WISE KL divergence --
adt_klrow_pack (adt_amd/csrc/adt_klrow_pack.cuh), DistRankMixin.rank_full / recommend(rowwise=True), kl_row_image(),
DisenDistSASupernet.rank_full_candidates(rowwise=True), FusedStosaTrainer.full_sort*(rowwise=True) and
SearcherEvolution.evaluate_candidates(rowwise=True).

    KL[u][v] = 0.5 (sum cu / ci + sum (mi - mu)^2 / ci - d + sum log ci - sum log cu) = nu[u] - (A[u] . W[v] + bias[v])

Bounds (none of them measured on the code under test).
  Pack: 1e-6, the bound tests/test_stosa_klgroups_hip.py asks of adt_kldist_pack on the same input magnitudes -- image entries against
  the largest magnitude of their column block ([0, d) and [d, 2d)), `off` against the sum of its terms' magnitudes, row by row.
  Ranking: a returned divergence lies within bound = (2d + 8) 2^-23 T of the float64 formula on the same fp32 inputs, T = sum_c |A_c W_c|
  + |bias| + |nu| in float64: the forward bound of a 2d-term fp32 accumulation plus the operands' roundings.  `the bound` of a row is
  the largest over its items.  A rank lies between the count of eligible items closer than the target by more than the bound and the
  count closer or within it.  Id lists are compared exactly on rows whose first K + 1 float64 places are more than two bounds apart;
  on the others (at most 10 % of the rows, a cap the float64 reference is asserted to meet before anything is compared): every id
  eligible, none twice, distances ascending within the bound, none farther than the float64 K-th place plus the bound.
  Model level: section 19's bounds for full-sort distances against the reference, 5e-4 (fp32) and 6e-2 (bf16) of the tensor's magnitude."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from adt_amd import _lib, ops  # noqa: E402
from tests.test_stosa_klrow_cpu import elu1_64, images64, kl_direct64  # noqa: E402

DEV = "cuda:0"
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return None if t is None else t.cpu().numpy()


# ---- 1. the pack ---------------------------------------------------------------------------------------------------------------------------
def pack_strided(M, C, items, pad=4):
    """adt_klrow_pack through the C ABI with ld = d + pad and ldi = 2d + pad: the pad columns of the inputs hold NaN, those of the image a
    sentinel that must survive.  Returns (img (rows, 2d) view, off) on the device."""
    rows, d = M.shape
    bm, bc = (torch.full((rows, d + pad), float("nan"), device=DEV) for _ in range(2))
    bm[:, :d], bc[:, :d] = dev(M), dev(C)
    img = torch.full((rows, 2 * d + pad), -7.0, device=DEV)
    off = torch.empty(rows, device=DEV)
    _lib.check(_lib.load().adt_klrow_pack(ops._p(bm), ops._p(bc), d + pad, rows, d, int(items), ops._p(img), 2 * d + pad, ops._p(off), ops._stream()),
               "klrow_pack")
    assert bool((img[:, 2 * d:] == -7.0).all())
    return img[:, :2 * d], off


def pack_inputs(rows, d, seed):
    """The magnitudes of tests/test_stosa_klgroups_hip.py: tables 0.3 N(0, 1), user covariances exp(0.2 N(0, 1))."""
    r = np.random.RandomState(seed)
    M, Ec = (0.3 * r.standard_normal((rows, d))).astype(np.float32), (0.3 * r.standard_normal((rows, d))).astype(np.float32)
    return M, Ec, np.exp(0.2 * r.standard_normal((rows, d))).astype(np.float32)


@pytest.mark.parametrize("items", (1, 0))
@pytest.mark.parametrize("rows,d", [(37, 4), (37, 20), (37, 64), (37, 68), (65557, 4)])
def test_klrow_pack_against_float64(rows, d, items):
    M, Ec, sc = pack_inputs(rows, d, 7 * rows + d)
    C = Ec if items else sc
    img_t, off_t = pack_strided(M, C, items)
    img2, off2 = pack_strided(M, C, items)
    assert torch.equal(img_t, img2) and torch.equal(off_t, off2)                      # two runs, bit for bit
    img, off = host(img_t).astype(np.float64), host(off_t).astype(np.float64)
    M64 = M.astype(np.float64)
    if items:
        c = elu1_64(C)
        lo, hi = -0.5 / c, M64 / c
        want_off = -0.5 * (np.log(c).sum(1) + (M64 * M64 / c).sum(1))
        mag = 0.5 * (np.abs(np.log(c)).sum(1) + (M64 * M64 / c).sum(1))
    else:
        c = C.astype(np.float64)
        lo, hi = M64 * M64 + c, M64
        want_off = -0.5 * (d + np.log(c).sum(1))
        mag = 0.5 * (d + np.abs(np.log(c)).sum(1))
    e_lo = np.abs(img[:, :d] - lo).max() / np.abs(lo).max()
    e_hi = np.abs(img[:, d:] - hi).max() / np.abs(hi).max()
    e_off = (np.abs(off - want_off) / mag).max()
    print("klrow_pack rows=%d d=%d items=%d: image %.3g / %.3g, off %.3g" % (rows, d, items, e_lo, e_hi, e_off))
    assert np.isfinite(img).all() and np.isfinite(off).all()
    assert e_lo < 1e-6 and e_hi < 1e-6 and e_off < 1e-6
    if rows == 37:                                                                     # ops.klrow_pack (ld = d, ldi = 2d): the same bits
        img3, off3 = ops.klrow_pack(dev(M), dev(C), bool(items))
        assert img3.shape == (rows, 2 * d) and off3.shape == (rows,)
        assert torch.equal(img3, img_t) and torch.equal(off3, off_t)


def test_klrow_pack_refusals():
    lib = _lib.load()
    M, C = torch.zeros(4, 72, device=DEV), torch.ones(4, 72, device=DEV)
    img, off = torch.empty(4, 136, device=DEV), torch.empty(4, device=DEV)
    P = ops._p

    def call(m=M, c=C, ld=72, rows=4, d=64, items=1, im=img, ldi=136, of=off):
        return lib.adt_klrow_pack(None if m is None else P(m), None if c is None else P(c), ld, rows, d, items, None if im is None else P(im), ldi,
                                  None if of is None else P(of), ops._stream())
    assert call() == 0 and call(items=0) == 0
    assert call(rows=0) == 0 and call(rows=-3) == 0 and call(rows=0, m=None, c=None, im=None, of=None) == 0      # nothing to do
    bad = {"d = 0": dict(d=0), "d = -4": dict(d=-4), "d % 4": dict(d=62), "ld < d": dict(ld=60), "ldi < 2d": dict(ldi=124),
           "ld % 4": dict(ld=70), "ldi % 4": dict(ldi=134), "M off a 16-byte boundary": dict(m=M.view(-1)[1:]),
           "C off a 16-byte boundary": dict(c=C.view(-1)[1:]), "img off a 16-byte boundary": dict(im=img.view(-1)[1:]),
           "M NULL": dict(m=None), "C NULL": dict(c=None), "img NULL": dict(im=None), "off NULL": dict(of=None),
           "items = 2": dict(items=2), "items = -1": dict(items=-1)}
    for what, kw in bad.items():
        with pytest.raises(_lib.AdtError):
            _lib.check(call(**kw), what)
    with pytest.raises(_lib.AdtError):
        ops.klrow_pack(M[:, :62], C[:, :62], True)
    assert call() == 0                                                                 # and the library still works
    torch.cuda.synchronize()


# ---- 2. ranking against float64 ------------------------------------------------------------------------------------------------------------
def eligibility(B, V, target, seen, first_id):
    """(B, V) bool: ids first_id .. V - 1 that the dense `seen` does not list; the target stays eligible."""
    elig = np.zeros((B, V), bool)
    elig[:, first_id:] = seen[:, first_id:] == 0
    if target is not None:
        elig[np.arange(B), target] = True
    return elig


def rank_case(B, V, d, seed):
    """Tables and states 0.5 N(0, 1), user covariances exp(0.5 N(0, 1)); ~10 % of the items seen, row 1 nothing, row 2 all but 4 ids
    (a -1 tail at K = 10); targets in 1 .. V - 1, row 3 lists its own target.  D, bound: the float64 formula on these fp32 inputs and
    (2d + 8) 2^-23 T."""
    r = np.random.RandomState(seed)
    Em, Ec, sm = ((0.5 * r.standard_normal(s)).astype(np.float32) for s in ((V, d), (V, d), (B, d)))
    sc = np.exp(0.5 * r.standard_normal((B, d))).astype(np.float32)
    seen = (r.rand(B, V) < 0.1).astype(np.int8)
    seen[1] = 0
    seen[2] = 1
    seen[2, r.choice(np.arange(1, V), 4, replace=False)] = 0
    target = r.randint(1, V, B).astype(np.int32)
    seen[3, target[3]] = 1
    ci = elu1_64(Ec)
    D = kl_direct64(sm, sc, Em, ci)
    A, nu, W, bias = images64(sm, sc, Em, ci)
    T = np.abs(A) @ np.abs(W).T + np.abs(bias)[None, :] + np.abs(nu)[:, None]
    return dict(Em=Em, Ec=Ec, sm=sm, sc=sc, seen=seen, target=target, D=D, bound=(2 * d + 8) * 2.0 ** -23 * T)


def ref_lists(D, elig):
    """Per row: the float64 order of the eligible ids (distance ascending, ties to the smaller id)."""
    return [np.flatnonzero(e)[np.lexsort((np.flatnonzero(e), Db[e]))] for Db, e in zip(D, elig)]


def separated(D, order, K, tb):
    """True when the first K + 1 places of the float64 order are more than two bounds apart."""
    o = D[order[:K + 1]]
    return bool((np.diff(o) > 2 * tb).all())


def check_ranking(c, K, first_id, rank, n_elig, ti, td, what):
    """The rules of the module docstring.  Returns (rows under the weaker rule, the largest |error| / bound seen)."""
    D, bound, seen, target = c["D"], c["bound"], c["seen"], c["target"]
    B, V = D.shape
    elig = eligibility(B, V, target, seen, first_id)
    orders = ref_lists(D, elig)
    tbs = bound.max(1)
    weak_ref = sum(not separated(D[b], orders[b], K, tbs[b]) for b in range(B))
    assert weak_ref <= 0.1 * B, (what, "the float64 reference itself has %d of %d rows with near-ties: choose another seed" % (weak_ref, B))
    weaker, worst = 0, 0.0
    ids = np.arange(V)
    for b in range(B):
        tb, t, order = tbs[b], int(target[b]), orders[b]
        other = elig[b] & (ids != t)
        assert n_elig[b] == other.sum(), (what, b)
        lo, hi = int((other & (D[b] < D[b, t] - tb)).sum()), int((other & (D[b] <= D[b, t] + tb)).sum())
        assert lo <= rank[b] <= hi, (what, b, lo, int(rank[b]), hi)
        n = min(K, len(order))
        got, gd = ti[b, :n].astype(np.int64), td[b, :n].astype(np.float64)
        assert (ti[b, n:] == -1).all() and np.isposinf(td[b, n:]).all(), (what, b)      # the tail of a short row
        assert (got >= first_id).all() and (got < V).all(), (what, b)
        err = np.abs(gd - D[b, got]) / bound[b, got]
        worst = max(worst, float(err.max()))
        assert (err <= 1.0).all(), (what, b, float(err.max()))
        if separated(D[b], order, K, tb):
            assert np.array_equal(got, order[:n]), (what, b)
        else:
            weaker += 1
            assert elig[b, got].all() and len(set(got.tolist())) == n, (what, b)
            assert (np.diff(D[b, got]) >= -tb).all(), (what, b)
            assert (D[b, got] <= D[b, order[n - 1]] + tb).all(), (what, b)
    assert weaker <= 0.1 * B, (what, weaker)
    return weaker, worst


@pytest.mark.parametrize("first_id", (0, 1))
@pytest.mark.parametrize("B,V,d,seed", [(5, 203, 64, 3), (21, 203, 20, 4)])
def test_rowwise_ranking_against_float64(B, V, d, seed, first_id):
    K = 10
    c = rank_case(B, V, d, seed)
    W, bias = ops.klrow_pack(dev(c["Em"]), dev(c["Ec"]), True)
    A, nu = ops.klrow_pack(dev(c["sm"]), dev(c["sc"]), False)
    indptr, indices = ops.seen_csr(c["seen"], B, DEV)
    rank, n_elig, ti, tv = ops.full_rank(A, A.stride(0), W, V - 1, dev(c["target"]), bias, indptr, indices, K, first_id=first_id)
    from adt_amd.fullrank import kl_dist_from_scores
    td = kl_dist_from_scores(nu, ti, tv)
    weaker, worst = check_ranking(c, K, first_id, host(rank), host(n_elig), host(ti), host(td), "B=%d d=%d first_id=%d" % (B, d, first_id))
    print("rowwise ranking B=%d V=%d d=%d first_id=%d: largest error %.3g of the bound, %d of %d rows under the weaker rule"
          % (B, V, d, first_id, worst, weaker, B))


# ---- 3. model level, on the golden's model ---------------------------------------------------------------------------------------------------
class Args:
    pass


def golden_model(prec, metric="kl", tag="kl_rowwise"):
    """The model of tests/golden/stosa_kl_rowwise.npz (that of stosa_kl_small.npz: seeded weights, biases moved off zero)."""
    from adt_amd.stosa.models import DisenDistSAModel
    from oracle import stosa_oracle as so
    g = np.load(os.path.join(GOLD, "stosa_%s.npz" % tag))
    V, L, d, H, nl, nu = [int(x) for x in g["cfg"]]
    cfg = so.Cfg(V, L, d, H, nl, num_users=nu, pvn_weight=float(g["pvn_weight"]))
    P = so.init_params(cfg, int(g["seed"]))
    r = np.random.RandomState(int(g["seed"]) + 1)
    for k in P:
        if k.endswith(".bias") and "LayerNorm" not in k:
            P[k] = (0.02 * r.standard_normal(P[k].shape)).astype(np.float32)
    a = Args()
    a.device, a.item_size, a.maxlen, a.hidden_units, a.num_heads, a.num_layers, a.num_users = DEV, V, L, d, H, nl, nu
    a.dropout, a.attention_dropout, a.pvn_weight, a.precision, a.distance_metric = 0.0, 0.0, cfg.pvn_weight, prec, metric
    m = DisenDistSAModel(a)
    m.load_numpy(P)
    return m.eval(), g


@pytest.mark.parametrize("prec", ("f32", "bf16"))
def test_model_rowwise_against_golden(prec):
    m, g = golden_model(prec)
    want = g["rowwise_dist"].astype(np.float64)
    B, V = want.shape
    tol = (5e-4 if prec == "f32" else 6e-2) * np.abs(want).max()
    sm, sc = m._last_state(g["input_ids"])
    e_state = max(np.abs(host(sm) - g["last_mean"]).max() / np.abs(g["last_mean"]).max(), np.abs(host(sc) - g["last_cov"]).max() / np.abs(g["last_cov"]).max())
    worst = 0.0
    for topk in (V - 1, V):                    # first_id = 0: V ids compete; V - 1 leaves out the farthest one only
        rank, n_elig, ti, td = m.rank_full(g["input_ids"], None, None, topk=topk, rowwise=True, first_id=0)
        ti, td = host(ti).astype(np.int64), host(td).astype(np.float64)
        assert ti.shape == (B, topk) and (host(rank) == -1).all() and (host(n_elig) == V).all()
        for b in range(B):
            assert len(set(ti[b].tolist())) == topk and ti[b].min() >= 0 and ti[b].max() < V, b
            assert (np.diff(td[b]) >= 0).all(), b
            got = np.full(V, np.nan)
            got[ti[b]] = td[b]                                                         # scattered back by id
            err = np.abs(got[ti[b]] - want[b, ti[b]]).max()
            worst = max(worst, err)
            assert err <= tol, (prec, b, err, tol)
            missing = np.setdiff1d(np.arange(V), ti[b])
            assert len(missing) == V - topk and (want[b, missing] >= want[b, ti[b]].max() - 2 * tol).all(), b
    print("model rowwise %s: distances %.3g of the tensor's magnitude (last states %.3g)" % (prec, worst / np.abs(want).max(), e_state))
    # recommend: never item 0, never a seen item; the same with a pre-packed image
    seen = (np.random.RandomState(2).rand(B, V) < 0.3).astype(np.int8)
    seen[0] = 1
    seen[0, [0, 5, 9]] = 0                     # two items left (0 does not count): a -1 tail
    image = m.kl_row_image()
    assert image[0].shape == (V, 2 * m.hidden_units) and image[1].shape == (V,)
    for img in (None, image):
        ids, dist = m.recommend(g["input_ids"], 10, seen=seen, image=img, rowwise=True)
        ids, dist = host(ids), host(dist)
        for b in range(B):
            real = ids[b][ids[b] >= 0]
            assert (real >= 1).all() and (seen[b, real] == 0).all() and len(set(real.tolist())) == len(real), b
            assert np.isposinf(dist[b][ids[b] < 0]).all() and np.isfinite(dist[b][ids[b] >= 0]).all(), b
            assert np.abs(dist[b][ids[b] >= 0] - want[b, real]).max() <= tol, b
        assert sorted(ids[0][ids[0] >= 0].tolist()) == [5, 9] and (ids[0][2:] == -1).all()
        assert (ids[1:] >= 1).all()


def test_rowwise_batch_independence():
    """Fixed state rows ranked as one batch of 21, as 16 + 5 and in reversed order: ids and distances bit-equal per user.  ops.kldist_full
    -- kl_predict_full -- on the same splits is a different function of the same rows: the reason this entry point exists."""
    m, g = golden_model("f32")
    V, d, B, K = m.item_size, m.hidden_units, 21, 10
    r = np.random.RandomState(11)
    sm = dev((0.5 * r.standard_normal((B, d))).astype(np.float32))
    sc = dev(np.exp(0.5 * r.standard_normal((B, d))).astype(np.float32))
    seen = (r.rand(B, V) < 0.2).astype(np.int8)
    target = r.randint(1, V, B).astype(np.int32)
    image = m.kl_row_image()

    def run(rows):
        out = m._rank_states(sm[rows].contiguous(), sc[rows].contiguous(), target[rows], seen[rows], K, image, 0, rowwise=True)
        return [host(x) for x in out]
    whole = run(np.arange(B))
    parts = [run(np.arange(0, 16)), run(np.arange(16, B))]
    split = [np.concatenate([p[i] for p in parts]) for i in range(4)]
    rev = [x[::-1] for x in run(np.arange(B)[::-1].copy())]
    for other in (split, rev):
        for x, y in zip(whole, other):
            assert x.dtype == y.dtype and np.array_equal(x.view(np.int32), y.view(np.int32))
    assert np.isfinite(whole[3]).all() and (whole[2] >= 0).all()
    Em, Ec, _ = m._dist_tables()
    full = host(ops.kldist_full(sm, sc, Em, Ec, V))
    two = np.concatenate([host(ops.kldist_full(sm[:16].contiguous(), sc[:16].contiguous(), Em, Ec, V)),
                          host(ops.kldist_full(sm[16:].contiguous(), sc[16:].contiguous(), Em, Ec, V))])
    assert np.abs(full - two).max() > 1e-3 * np.abs(full).max()


# ---- 4. trainer ---------------------------------------------------------------------------------------------------------------------------
def test_full_sort_rowwise():
    """full_sort / full_sort_scores(rowwise=True) on a KL model: the ids of rank_full(first_id=0, rowwise=True) batch by batch, -1 tails
    kept (no two-pass fallback), the image packed once, the histogram that of the host lists; the metrics do not move with the batch
    size; fused=True still raises."""
    from adt_amd.stosa.trainer import FusedStosaTrainer, get_full_sort_score
    m, g = golden_model("f32")
    V, L, nl, K = m.item_size, m.maxlen, m.num_layers, 40
    r = np.random.RandomState(3)
    N = 21
    seqs = r.randint(1, V - 1, size=(N, L)).astype(np.int32)
    seqs[:, :3] = 0
    seen = (r.rand(N, V) < 0.1).astype(np.int8)
    ans = r.randint(1, V, size=(N, 1))
    seen[np.arange(N), ans[:, 0]] = 0                                  # a held-out item is never in the seen list
    seen[7] = 1
    seen[7, [ans[7, 0], 0]] = 0                                        # user 7: two unseen ids, 38 places of -1
    tr = FusedStosaTrainer(m, [0.3] * nl, [0.2] * nl)
    packs = []
    real = m.kl_row_image
    m.kl_row_image = lambda: packs.append(1) or real()

    def batches(bs):
        return [(seqs[s:s + bs], seen[s:s + bs], ans[s:s + bs]) for s in range(0, N, bs)]
    pred, answers = tr.full_sort(batches(16), topk=K, rowwise=True)
    assert len(packs) == 1 and tr.fused_fallbacks == 0
    assert pred.shape == (N, K) and pred.dtype == np.int64 and np.array_equal(answers, ans)
    image = real()
    for s in (0, 16):
        want = host(m.rank_full(seqs[s:s + 16], None, seen[s:s + 16], K, image, first_id=0, rowwise=True)[2])
        assert np.array_equal(pred[s:s + 16], want)
    assert (pred[7, 2:] == -1).all() and sorted(pred[7, :2].tolist()) == sorted([0, int(ans[7, 0])])
    for b in range(N):
        real_ids = pred[b][pred[b] >= 0]
        assert (seen[b, real_ids] == 0).all() and len(set(real_ids.tolist())) == len(real_ids)
    pred5, _ = tr.full_sort(batches(5), topk=K, rowwise=True)          # another batch size: the same lists
    assert np.array_equal(pred5, pred)
    scores, hist = tr.full_sort_scores(batches(16), topk=K, rowwise=True)
    assert len(packs) == 3 and hist.sum() == N
    want_scores = get_full_sort_score(ans, pred)
    assert np.abs(np.asarray(scores) - np.asarray(want_scores)).max() <= 1e-12
    del m.kl_row_image
    with pytest.raises(_lib.AdtError, match="wasserstein"):
        tr.full_sort(batches(16), topk=K, fused=True, rowwise=True)
    with pytest.raises(_lib.AdtError, match="wasserstein"):
        tr.full_sort_scores(batches(16), topk=K, fused=True, rowwise=True)


# ---- 5. supernet and search ------------------------------------------------------------------------------------------------------------------
def test_supernet_rank_full_candidates_rowwise():
    from adt_amd.supersearch import cand_to_block, get_shared
    from tests.test_superstosa_kl_hip import build_stosa
    g = np.load(os.path.join(GOLD, "superstosa_kl_c3.npz"))
    m = build_stosa(g, "f32").eval()
    V, L, nl = m.item_size, m.maxlen, m.num_layers
    rc, ic = g["rec_choice"], g["ind_choice"]
    r = np.random.RandomState(9)
    cands = [[float(x) for x in g["cand"]], [float(x) for x in g["cand2"]]] + [[float(x) for x in r.rand(2 * nl)] for _ in range(2)]
    blocks = [cand_to_block(rc, ic, c)[0] for c in cands]
    shared = [get_shared(rc, ic, b) for b in blocks]
    P_, B, K = len(cands), 9, 10
    seqs = r.randint(1, V - 1, size=(B, L)).astype(np.int32)
    seqs[:, :3] = 0
    seen = (r.rand(B, V) < 0.1).astype(np.int8)
    target = r.randint(1, V, B).astype(np.int32)
    image = m.kl_row_image()                                           # one image for all four: the candidates share the item tables
    rank, nel, ti, td = m.rank_full_candidates(seqs, shared, target, np.tile(seen, (P_, 1)), K, image, first_id=0, rowwise=True)
    assert rank.shape == (P_ * B,) and ti.shape == td.shape == (P_ * B, K) and bool(torch.isfinite(td).all())
    again = m.rank_full_candidates(seqs, shared, target, np.tile(seen, (P_, 1)), K, None, first_id=0, rowwise=True)      # packed inside
    assert torch.equal(again[2], ti) and torch.equal(again[3], td)
    for p in range(P_):
        m.set_choice(blocks[p])
        one = m.rank_full(seqs, target, seen, K, image, first_id=0, rowwise=True)
        assert torch.equal(ti[p * B:(p + 1) * B], one[2]), p
        assert torch.equal(nel[p * B:(p + 1) * B], one[1]), p
    with pytest.raises(_lib.AdtError):                                 # opt-in only
        m.rank_full_candidates(seqs, shared, target, None, K)
    with pytest.raises(_lib.AdtError):
        m.item_image()


def test_search_rowwise(tmp_path):
    from tests.test_stosa_klsearch_hip import make_searcher
    s, g, nl = make_searcher(tmp_path, [])
    r = np.random.RandomState(9)
    cands = [[float(x) for x in g["cand"]], [float(x) for x in g["cand2"]]] + [[float(x) for x in r.rand(2 * nl)] for _ in range(2)]
    base = s.evaluate_candidates(cands, group=2, device_batches=False, device_scores=False, rowwise=True)
    assert len(base) == 4 and all(np.isfinite(v) for o in base for v in o.values())
    for device_batches, device_scores in ((False, True), (True, False), (True, True)):
        out = s.evaluate_candidates(cands, group=2, device_batches=device_batches, device_scores=device_scores, rowwise=True)
        for got, want in zip(out, base):
            assert sorted(got) == sorted(want) == ["MRR", "V_HR", "V_MRR", "V_NDCG"]
            assert max(abs(got[k] - want[k]) for k in want) <= 1e-12, (device_batches, device_scores, got, want)
        if device_scores:
            assert s.last_hists.shape == (4, 41) and (s.last_hists.sum(1) == 50).all()
    one = s.evaluate_candidates(cands, group=4, rowwise=True)          # the grouping changes nothing either
    assert all(max(abs(a[k] - b[k]) for k in a) <= 1e-12 for a, b in zip(one, base))
    with pytest.raises(_lib.AdtError):
        s.evaluate_candidates(cands, group=2, fused=True, rowwise=True)
    from adt_amd.stosa import evolution as ev
    assert ev.parse_args(["--distance_metric", "kl", "--rowwise_eval"]).rowwise_eval


# ---- 6. opt-in only ------------------------------------------------------------------------------------------------------------------------
def test_wasserstein_rowwise_is_the_default_call():
    m, g = golden_model("f32", "wasserstein", "small")
    V = m.item_size
    seen = (np.random.RandomState(4).rand(len(g["input_ids"]), V) < 0.2).astype(np.int8)
    target = g["pos_ids"][:, -1].astype(np.int32)
    a = m.rank_full(g["input_ids"], target, seen, 10)
    b = m.rank_full(g["input_ids"], target, seen, 10, rowwise=True)
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    ra, rb = m.recommend(g["input_ids"], 10, seen), m.recommend(g["input_ids"], 10, seen, rowwise=True)
    assert torch.equal(ra[0], rb[0]) and torch.equal(ra[1].view(torch.int32), rb[1].view(torch.int32))
    with pytest.raises(_lib.AdtError, match="kl"):
        m.kl_row_image()


def test_kl_defaults_still_raise():
    from adt_amd.stosa.trainer import FusedStosaTrainer
    m, g = golden_model("f32")
    nl = m.num_layers
    with pytest.raises(_lib.AdtError, match="wasserstein"):
        m.rank_full(g["input_ids"], None, None, 5)
    with pytest.raises(_lib.AdtError, match="wasserstein"):
        m.recommend(g["input_ids"], 5)
    with pytest.raises(_lib.AdtError, match="wasserstein"):
        m.item_image()
    tr = FusedStosaTrainer(m, [0.3] * nl, [0.2] * nl)
    with pytest.raises(_lib.AdtError, match="wasserstein"):
        tr.full_sort([(g["input_ids"], None, np.ones((len(g["input_ids"]), 1), np.int64))], topk=5, fused=True)
