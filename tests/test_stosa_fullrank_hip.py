"""GPU: fused full-catalogue ranking for STOSA-ADT (Wasserstein) -- adt_wdist_pack (adt_amd/csrc/adt_wdist_pack.cuh), the first_id
argument of adt_full_rank_from (adt_fullrank.cuh), DistRankMixin (adt_amd/fullrank.py) on DisenDistSAModel / DisenDistSASupernet and
FusedStosaTrainer.full_sort(fused=True) -- against numpy references that live in this file (helpers after tests/test_fullrank_hip.py).

Tolerances (derived, not tuned).  u = 2^-24, the unit roundoff of fp32; first-order bounds, doubled, as in tests/test_fullrank_hip.py.

  Pack, covariance c.  elu = 0: c is the input, exact (eps_c = 0).  elu = 1, x > 0: c = fl(x + 1), one rounding, relative eps_c = u.
  elu = 1, x <= 0: c = fl(fl(expf(x) - 1) + 1) with expf within 1 ulp (relative 2u, and expf(x) <= 1), then two roundings of results
  of magnitude <= 1: absolute error <= 2u + u + u = 4u, relative eps_c = 4u / c (c >= e^-3 on the inputs used here).
  Pack, element.  sqrtf within 1 ulp (relative 2u) of sqrt(c (1 + eps_c)) = sqrt(c) (1 + eps_c / 2):
      elem_tol = 2 * sqrt(c) * (eps_c / 2 + 2u).
  Pack, norm.  nrm = nrm_scale * (sum M^2 + sum c): 2d terms, each product M^2 rounded once (u M^2), each c off by eps_c c, a sum of
  length 2d (at most 2d roundings of partial sums <= the total, whatever the order) and the final multiply:
      nrm_tol = 2 * |nrm_scale| * ((2d + 2) u (sum M^2 + sum c) + sum eps_c c).
  Ranking.  s = A . W + bias is one fp32 accumulation over the 2d + 1 terms (the first-order bound of the existing file, doubled)
  of operands that carry the pack tolerances, and dist = fl(na - 2 s) adds one rounding:
      s_tol = 2 (2d + 1) u (|A| . |W| + |bias|) + |A| . W_tol + A_tol . |W| + bias_tol
      dist_tol = na_tol + 2 s_tol + 2u (|na| + 2 |s|).
  Model level: the reference distances are fp32 themselves (k_wdist_full: the same 2d products and norm terms, summed in fp32 from
  the same rounded operands), so they carry the same first-order bound: tol = 2 dist_tol.
A rank must lie between count(D < Dt - tol) and count(D < Dt + tol); a returned distance within tol of its id's reference distance; the
K-th returned item within 2 tol of the true K-th distance (check_bracket, on scores S = -D)."""
import functools
import os

import numpy as np
import pytest
import torch

from adt_amd import _lib, ops

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U = 2.0 ** -24
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# ---- numpy reference (after tests/test_fullrank_hip.py, with first_id) -----------------------------------------------------------------
def eligibility(B, n_items, target, indptr, indices, first_id=1):
    elig = np.zeros((B, n_items + 1), bool)
    elig[:, first_id:] = True
    if indptr is not None:
        for b in range(B):
            ids = indices[indptr[b]:indptr[b + 1]]
            ids = ids[(ids >= first_id) & (ids <= n_items)]
            elig[b, ids] = False
    for b in range(B):
        if 1 <= target[b] <= n_items:
            elig[b, target[b]] = True
    return elig


def ref_rank_topk(S, elig, target, k):
    """S: (B, n_items + 1) scores (int64 or float64).  rank / n_elig / top ids / top scores (float64; -1 / -inf tail)."""
    B, n1 = S.shape
    ids = np.arange(n1)
    rank, nel = np.zeros(B, np.int64), np.zeros(B, np.int64)
    top_idx, top_val = np.full((B, k), -1, np.int64), np.full((B, k), -np.inf)
    for b in range(B):
        t = target[b] if 1 <= target[b] < n1 else 0
        other = elig[b] & (ids != t) if t else elig[b]
        nel[b] = other.sum()
        rank[b] = (other & (S[b] > S[b, t])).sum() if t else -1
        cand = ids[elig[b]]
        order = cand[np.lexsort((cand, -S[b, cand]))][:k]      # score descending, ties to the smaller id
        top_idx[b, :len(order)] = order
        top_val[b, :len(order)] = S[b, order]
    return rank, nel, top_idx, top_val


def make_csr(r, B, n_items, target):
    """Seen lists with every edge the kernel has to handle: an empty row, a row listing the target, id 0, an id above n_items, a
    duplicate, rows that leave 5 / 1 / 0 eligible items (the -1 tail at every K >= 1)."""
    rows = []
    for b in range(B):
        t = int(target[b])
        kind = b % 8 if B > 1 else 3
        if kind == 0:
            ids = []
        elif kind == 1:
            ids = [t, 1, n_items] + list(r.randint(1, n_items + 1, 9))
        elif kind == 2:
            ids = [0, n_items + 1, n_items + 7, 3, 3, 3, 0] + list(r.randint(0, n_items + 3, 20))
        elif kind == 3:      # all but five items seen (the target listed too, ids out of range and duplicates mixed in)
            keep = set(r.choice(np.arange(1, n_items + 1), 5, replace=False).tolist())
            ids = [i for i in range(1, n_items + 1) if i not in keep] + [0, n_items + 2, 2, 2]
            r.shuffle(ids)
        elif kind == 4:      # everything seen: only the target is left (and item 0 where it competes)
            ids = list(range(1, n_items + 1))
        else:
            ids = list(r.randint(1, n_items + 1, r.randint(0, 60)))
        rows.append(ids)
    indptr = np.zeros(B + 1, np.int32)
    np.cumsum([len(x) for x in rows], out=indptr[1:])
    return indptr, np.asarray([i for x in rows for i in x], np.int32)


def check_bracket(S, tol, elig, target, k, rank, ti, tv, first_id, what=""):
    """check_bracket of tests/test_fullrank_hip.py (ids >= first_id instead of >= 1).  S: reference scores (B, n + 1) float64, larger
    is better (here: minus the distance), tol the same shape; tv the returned scores."""
    B, n1 = S.shape
    ids = np.arange(n1)
    for b in range(B):
        t = int(target[b]) if target is not None else 0
        if t:
            other = elig[b] & (ids != t)
            lo = int((other & (S[b] > S[b, t] + tol[b])).sum())
            hi = int((other & (S[b] > S[b, t] - tol[b])).sum())
            assert lo <= rank[b] <= hi, (what, b, lo, int(rank[b]), hi)
        if k:
            got = ti[b]
            assert (got >= first_id).all() and len(set(got.tolist())) == k and elig[b, got].all(), (what, b)
            if tv is not None:
                assert (np.abs(tv[b] - S[b, got]) <= tol[b, got]).all(), (what, b, np.abs(tv[b] - S[b, got]).max())
                assert (np.diff(tv[b]) <= 0).all(), (what, b)
            kth = np.sort(S[b, elig[b]])[-k]
            assert S[b, got[-1]] >= kth - 2 * tol[b, got[-1]], (what, b)


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return None if t is None else t.cpu().numpy()


# ---- float64 pack reference and the tolerances of the docstring ---------------------------------------------------------------------------
def pack_ref(M, C, elu, scale):
    """float64 (img, nrm, elem_tol (rows, d) of the covariance half, nrm_tol (rows,)) from fp32 inputs."""
    M64, C64 = M.astype(np.float64), C.astype(np.float64)
    if elu:
        c = np.where(C64 > 0, C64 + 1.0, np.exp(np.minimum(C64, 0.0)))
        eps = np.where(C64 > 0, U, 4.0 * U / c)
    else:
        c, eps = C64, np.zeros_like(C64)
    root = np.sqrt(np.maximum(c, 1e-24))
    d = M.shape[1]
    tot = (M64 ** 2).sum(1) + c.sum(1)
    img = np.concatenate([M64, root], 1)
    elem_tol = 2.0 * root * (eps / 2.0 + 2.0 * U)
    nrm_tol = 2.0 * abs(scale) * ((2 * d + 2) * U * tot + (eps * c).sum(1))
    return img, scale * tot, elem_tol, nrm_tol


def dist_ref(sm, sc, Em, Ec):
    """Reference distances (B, V) in float64 from the tables, and dist_tol of the docstring."""
    A, na, tA, tna = pack_ref(sm, sc, 0, 1.0)
    W, bias, tW, tb = pack_ref(Em, Ec, 1, -0.5)
    d = sm.shape[1]
    D = ((A[:, None, :] - W[None, :, :]) ** 2).sum(2) if A.shape[0] * W.shape[0] * 2 * d < 5e7 else None
    s = A @ W.T + bias
    if D is None:
        D = na[:, None] - 2.0 * s
    absA, absW = np.abs(A), np.abs(W)
    tA_full = np.concatenate([np.zeros_like(tA), tA], 1)      # the mean half is copied bit for bit
    tW_full = np.concatenate([np.zeros_like(tW), tW], 1)
    s_tol = 2.0 * (2 * d + 1) * U * (absA @ absW.T + np.abs(bias)) + absA @ tW_full.T + tA_full @ absW.T + tb
    tol = tna[:, None] + 2.0 * s_tol + 2.0 * U * (np.abs(na)[:, None] + 2.0 * np.abs(s))
    return D, tol


# ---- 1. first_id, exact ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def first_id_case(n_items, d=64, B=37):
    """int_case of tests/test_fullrank_hip.py with table row 0 the best item of users 0 and 5 (both have no 0 in their seen lists; rows
    b % 8 in (2, 3) list it).  References at K = 128 for first_id 0 and 1."""
    r = np.random.RandomState(7000 + n_items)
    E = r.randint(-3, 4, size=(n_items + 1, d)).astype(np.float32)
    F = r.randint(-3, 4, size=(B, d)).astype(np.float32)
    F[5] = F[0]
    E[0] = 3.0 * np.sign(F[0] + 0.5)       # 3 sum |F[0]|: no row scores higher, and the tie rule prefers id 0
    target = r.randint(1, n_items + 1, B).astype(np.int32)
    target[6] = 0
    target[12] = 0
    for b in range(B):
        if target[b]:
            E[r.randint(1, n_items + 1, 2)] = E[target[b]]
    indptr, indices = make_csr(r, B, n_items, target)
    S = F.astype(np.int64) @ E.astype(np.int64).T
    refs = {f: ref_rank_topk(S, eligibility(B, n_items, target, indptr, indices, f), target, 128) for f in (0, 1)}
    return dict(F=F, E=E, target=target, indptr=indptr, indices=indices, n_items=n_items, refs=refs, S=S)


def run_fr(c, k, splits=0, **kw):
    F, E = dev(c["F"]), dev(c["E"])
    out = ops.full_rank(F, F.stride(0), E, c["n_items"], dev(c["target"]), None, dev(c["indptr"]), dev(c["indices"]), k, splits, **kw)
    torch.cuda.synchronize()
    return out


def check_exact(ref, out, k):
    rank, nel, ti, tv = out
    r_rank, r_nel, r_ti, r_tv = ref
    print("rank mismatches", int((host(rank) != r_rank).sum()), "n_elig mismatches", int((host(nel) != r_nel).sum()))
    assert np.array_equal(host(rank), r_rank)
    assert np.array_equal(host(nel), r_nel)
    if k == 0:
        assert ti is None and tv is None
        return
    assert np.array_equal(host(ti), r_ti[:, :k])
    assert np.array_equal(host(tv).astype(np.float64), r_tv[:, :k])


@pytest.mark.parametrize("n_items", (20, 5003))
def test_first_id_exact(n_items):
    c = first_id_case(n_items)
    r0, r1 = c["refs"][0], c["refs"][1]
    assert r0[2][0, 0] == 0 and r0[2][5, 0] == 0                          # the reference itself: item 0 heads users 0 and 5 ...
    assert r0[1][0] == r1[1][0] + 1 and r0[1][2] == r1[1][2]              # ... is counted for user 0 and not for user 2, who lists it
    assert r0[0][0] == r1[0][0] + 1                                       # ... and outranks user 0's target
    assert not (r0[2][2] == 0).any() and not (r0[2][3] == 0).any()
    for k in (0, 1, 40, 128):
        out0 = run_fr(c, k, first_id=0)
        check_exact(r0, out0, k)
        out1 = run_fr(c, k, first_id=1)
        check_exact(r1, out1, k)
        base = run_fr(c, k)
        for a, b in zip(out1, base):
            assert (a is None and b is None) or torch.equal(a, b), k
    for k in (10, 128):                                                   # splits 0 / 1 / 7: bit-identical at first_id = 0
        base = run_fr(c, k, 0, first_id=0)
        for splits in (1, 7):
            for a, b in zip(base, run_fr(c, k, splits, first_id=0)):
                assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (k, splits)
    with pytest.raises(_lib.AdtError):
        run_fr(c, 1, first_id=2)
    with pytest.raises(_lib.AdtError):
        run_fr(c, 1, first_id=-1)


# ---- 2. pack -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("elu", (0, 1))
@pytest.mark.parametrize("rows", (1, 37, 1000))
@pytest.mark.parametrize("d", (16, 52, 64))
def test_pack_against_float64(d, rows, elu):
    r = np.random.RandomState(100 * d + rows + elu)
    ld = d + 12                                                 # a row stride larger than d, junk beyond column d: never read
    M = r.uniform(-2, 2, size=(rows, ld)).astype(np.float32)
    C = (r.uniform(-3, 3, size=(rows, ld)) if elu else r.uniform(0.05, 4, size=(rows, ld))).astype(np.float32)
    M[:, d:] = 1e30
    C[:, d:] = np.nan
    scale = -0.5 if elu else 1.0
    Md, Cd = dev(M), dev(C)
    img, nrm = ops.wdist_pack(Md[:, :d], Cd[:, :d], elu, scale)
    img2, nrm2 = ops.wdist_pack(Md[:, :d], Cd[:, :d], elu, scale)
    torch.cuda.synchronize()
    assert img.shape == (rows, 2 * d) and nrm.shape == (rows,)
    assert torch.equal(img.view(torch.int32), img2.view(torch.int32)) and torch.equal(nrm.view(torch.int32), nrm2.view(torch.int32))
    img, nrm = host(img), host(nrm)
    assert np.array_equal(img[:, :d].view(np.int32), M[:, :d].view(np.int32))        # the mean half: bit-equal copies
    r_img, r_nrm, e_tol, n_tol = pack_ref(M[:, :d], C[:, :d], elu, scale)
    e_err, n_err = np.abs(img[:, d:] - r_img[:, d:]), np.abs(nrm - r_nrm)
    print("d", d, "rows", rows, "elu", elu, "max element err / tol", float((e_err / e_tol).max()), "max norm err / tol", float((n_err / n_tol).max()))
    assert np.isfinite(img).all() and np.isfinite(nrm).all()
    assert (e_err <= e_tol).all() and (n_err <= n_tol).all()


def test_pack_clamp_value():
    """A covariance of exactly 0 (elu = 0) is clamped to 1e-24 before the root: the image holds 1e-12 (relative u / 2 from the
    rounding of the fp32 constant 1e-24f, halved by the root, plus 2u from sqrtf: under 3u, doubled)."""
    d = 16
    M = np.ones((2, d), np.float32)
    C = np.full((2, d), 0.25, np.float32)
    C[1] = 0.0
    img, nrm = ops.wdist_pack(dev(M), dev(C), 0, 1.0)
    img, nrm = host(img).astype(np.float64), host(nrm).astype(np.float64)
    assert np.array_equal(img[0, d:], np.full(d, 0.5))
    assert (np.abs(img[1, d:] - 1e-12) <= 2.0 * 3.0 * U * 1e-12).all(), img[1, d:]
    assert nrm[0] == d + 0.25 * d and nrm[1] == d          # the norm sums the covariance BEFORE clamp and root


# ---- 3. exact Wasserstein ranking ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def wdist_int_case(n_items, B, d):
    """Integer means in [-3, 3], state covariances in {1, 4, 9}, raw item covariances in {0, 3, 8, 15} (ELU + 1 in {1, 4, 9, 16}): every
    root, product and half-integer bias is exact in fp32.  The reference works on doubled scores 2 s = 2 A . W - nb (integers)."""
    r = np.random.RandomState(31 * n_items + 7 * d + B)
    Em = r.randint(-3, 4, size=(n_items + 1, d)).astype(np.float32)
    Ec = r.choice([0.0, 3.0, 8.0, 15.0], size=(n_items + 1, d)).astype(np.float32)
    Em[0], Ec[0] = 0.0, 0.0                                 # the padding row: zero mean, unit covariance
    sm = r.randint(-3, 4, size=(B, d)).astype(np.float32)
    sc = r.choice([1.0, 4.0, 9.0], size=(B, d)).astype(np.float32)
    target = r.randint(1, n_items + 1, B).astype(np.int32)
    if B > 12:
        target[6] = 0
        target[12] = 0
    for b in range(B):                                      # copies of the target's rows elsewhere: real ties
        if target[b]:
            for j in r.randint(1, n_items + 1, 2):
                Em[j], Ec[j] = Em[target[b]], Ec[target[b]]
    indptr, indices = make_csr(r, B, n_items, target)
    A = np.concatenate([sm, np.sqrt(sc)], 1).astype(np.int64)
    W = np.concatenate([Em, np.sqrt(np.where(Ec > 0, Ec + 1, 1.0))], 1).astype(np.int64)
    na, nb = (A ** 2).sum(1), (W ** 2).sum(1)
    S2 = 2 * (A @ W.T) - nb
    assert n_items > 1000 or np.array_equal(na[:, None] - S2, ((A[:, None, :] - W[None, :, :]) ** 2).sum(2))      # the algebra itself
    refs = {f: ref_rank_topk(S2, eligibility(B, n_items, target, indptr, indices, f), target, 128) for f in (0, 1)}
    return dict(Em=Em, Ec=Ec, sm=sm, sc=sc, target=target, indptr=indptr, indices=indices, n_items=n_items, na=na, refs=refs)


@pytest.mark.parametrize("B", (1, 37))
@pytest.mark.parametrize("d", (16, 52, 64))
@pytest.mark.parametrize("n_items", (20, 1000, 5003))
def test_exact_wasserstein_ranking(n_items, d, B):
    c = wdist_int_case(n_items, B, d)
    W, bias = ops.wdist_pack(dev(c["Em"]), dev(c["Ec"]), True, -0.5)
    A, na = ops.wdist_pack(dev(c["sm"]), dev(c["sc"]), False, 1.0)
    assert np.array_equal(host(na).astype(np.int64), c["na"])
    from adt_amd.fullrank import dist_from_scores
    for first_id in (0, 1):
        r_rank, r_nel, r_ti, r_s2 = c["refs"][first_id]
        for k in (0, 1, 40, 128):
            rank, nel, ti, tv = ops.full_rank(A, A.stride(0), W, n_items, dev(c["target"]), bias, dev(c["indptr"]), dev(c["indices"]), k,
                                              first_id=first_id)
            assert np.array_equal(host(rank), r_rank) and np.array_equal(host(nel), r_nel), (first_id, k)
            if k == 0:
                assert ti is None
                continue
            assert np.array_equal(host(ti), r_ti[:, :k]), (first_id, k)
            want = c["na"][:, None].astype(np.float64) - r_s2[:, :k]          # -(-inf) = +inf where the id is -1
            got = host(dist_from_scores(na, ti, tv)).astype(np.float64)
            assert np.array_equal(got, want), (first_id, k)
            assert np.isposinf(got[r_ti[:, :k] < 0]).all()


# ---- 4. real-valued against float64 --------------------------------------------------------------------------------------------------------
def test_real_distances_against_float64():
    from adt_amd.fullrank import dist_from_scores
    n_items, B, d, k = 5003, 37, 64, 40
    r = np.random.RandomState(64)
    Em, Ec = r.randn(n_items + 1, d).astype(np.float32), r.uniform(-3, 3, size=(n_items + 1, d)).astype(np.float32)
    sm, sc = r.randn(B, d).astype(np.float32), r.uniform(0.05, 4, size=(B, d)).astype(np.float32)
    target = r.randint(1, n_items + 1, B).astype(np.int32)
    rows = [list(r.randint(0, n_items + 1, r.randint(0, 80))) for _ in range(B)]
    indptr = np.zeros(B + 1, np.int32)
    np.cumsum([len(x) for x in rows], out=indptr[1:])
    indices = np.asarray([i for x in rows for i in x], np.int32)
    D, tol = dist_ref(sm, sc, Em, Ec)
    print("dist_tol: max", float(tol.max()), "relative to the distance", float((tol / D).max()))
    W, bias = ops.wdist_pack(dev(Em), dev(Ec), True, -0.5)
    A, na = ops.wdist_pack(dev(sm), dev(sc), False, 1.0)
    ids = np.arange(n_items + 1)
    for first_id in (0, 1):
        elig = eligibility(B, n_items, target, indptr, indices, first_id)
        rank, nel, ti, tv = ops.full_rank(A, A.stride(0), W, n_items, dev(target), bias, dev(indptr), dev(indices), k, first_id=first_id)
        td = host(dist_from_scores(na, ti, tv)).astype(np.float64)
        assert np.array_equal(host(nel), [(elig[b] & (ids != target[b])).sum() for b in range(B)])
        ti = host(ti)
        print("first_id", first_id, "max |dist - float64| / tol over the returned items",
              float(np.max(np.abs(td - np.take_along_axis(D, ti, 1)) / np.take_along_axis(tol, ti, 1))))
        check_bracket(-D, tol, elig, target, k, host(rank), ti, -td, first_id, "first_id=%d" % first_id)


# ---- 5. model level ------------------------------------------------------------------------------------------------------------------------
class Args:
    pass


def load_case(tag):
    from oracle import stosa_oracle as so
    g = np.load(os.path.join(GOLD, "stosa_%s.npz" % tag))
    V, L, d, H, nl, nu = [int(x) for x in g["cfg"]]
    cfg = so.Cfg(V, L, d, H, nl, num_users=nu, pvn_weight=float(g["pvn_weight"]))
    P = so.init_params(cfg, int(g["seed"]))
    r = np.random.RandomState(int(g["seed"]) + 1)
    for k in P:
        if k.endswith(".bias") and "LayerNorm" not in k:
            P[k] = (0.02 * r.standard_normal(P[k].shape)).astype(np.float32)
    return g, cfg, P


def build(cfg, P, metric="wasserstein"):
    from adt_amd.stosa.models import DisenDistSAModel
    a = Args()
    a.device, a.item_size, a.maxlen, a.hidden_units, a.num_heads, a.num_layers, a.num_users = DEV, cfg.item_size, cfg.maxlen, cfg.hidden_units, cfg.num_heads, cfg.num_layers, cfg.num_users
    a.dropout, a.attention_dropout, a.pvn_weight, a.precision, a.distance_metric = 0.0, 0.0, cfg.pvn_weight, "f32", metric
    m = DisenDistSAModel(a)
    m.load_numpy(P)
    return m.eval()


def random_batch(r, B, L, V, heavy_row=None):
    """(input_ids (B, L), dense seen (B, V)): ~10 % of the items seen; heavy_row: all but five items seen, item 0 included."""
    seqs = r.randint(1, V - 1, size=(B, L)).astype(np.int32)
    seqs[:, :3] = 0
    seen = (r.rand(B, V) < 0.1).astype(np.int8)
    seen[1] = 0
    if heavy_row is not None:
        seen[heavy_row] = 1
        seen[heavy_row, r.choice(np.arange(1, V), 5, replace=False)] = 0
    return seqs, seen


def model_tol(m, states, V):
    sm, sc = (host(x) for x in states)
    Em, Ec, n_items = m._dist_tables()
    assert n_items == V - 1
    _, tol = dist_ref(sm, sc, host(Em)[:V], host(Ec)[:V])
    return 2.0 * tol                    # the reference is fp32 too (docstring)


def check_id_lists(got, want, D, tol, seen, k, what):
    """Rule of full_sort(fused=True) against full_sort(): per row, equal id SETS where the reference's k-th and (k + 1)-th distances
    (seen items pushed away) differ by more than 2 tol; otherwise the bracket rule.  Returns the number of rows under the weaker rule."""
    weaker = 0
    for b in range(len(got)):
        Db = np.where(seen[b] > 0, np.inf, D[b])
        order = np.sort(Db)
        t = tol[b].max()
        if order[k] - order[k - 1] > 2 * t:
            assert set(got[b].tolist()) == set(want[b].tolist()), (what, b)
        else:
            weaker += 1
            assert len(set(got[b].tolist())) == k and (seen[b, got[b]] == 0).all() and (got[b] >= 0).all(), (what, b)
            assert (Db[got[b]] <= order[k - 1] + 2 * t).all(), (what, b)
    return weaker


@pytest.mark.parametrize("tag", ("small", "l2h2"))
def test_model_rank_full_recommend_and_full_sort(tag):
    import scipy.sparse as sp
    from adt_amd.stosa.trainer import FusedStosaTrainer
    g, cfg, P = load_case(tag)
    m = build(cfg, P)
    V, L, B, k = cfg.item_size, cfg.maxlen, 21, 10
    r = np.random.RandomState(5)
    seqs, dense = random_batch(r, B, L, V)
    target = r.randint(1, V, B).astype(np.int32)
    dense[4, target[4]] = 1
    D = host(m.predict_full(seqs)).astype(np.float64)
    tol = model_tol(m, m._last_state(seqs), V)
    print(tag, "tol max", float(tol.max()), "distance spread", float(D.max() - D.min()))
    r_ip, r_ix = ops.seen_csr_host(dense, B)
    ids = np.arange(V)
    image = m.item_image()
    for first_id in (1, 0):
        elig = eligibility(B, V - 1, target, r_ip, r_ix, first_id)
        for seen, img in ((sp.csr_matrix(dense), None), (dense, image)):
            rank, nel, ti, td = m.rank_full(seqs, target, seen, topk=k, image=img, first_id=first_id)
            assert np.array_equal(host(nel), [(elig[b] & (ids != target[b])).sum() for b in range(B)])
            check_bracket(-D, tol, elig, target, k, host(rank), host(ti), -host(td).astype(np.float64), first_id, "%s first_id=%d" % (tag, first_id))
    rec_ids, rec_d = m.recommend(seqs, k, seen=dense, image=image)
    elig_nt = eligibility(B, V - 1, np.zeros(B, np.int32), r_ip, r_ix, 1)
    check_bracket(-D, tol, elig_nt, None, k, None, host(rec_ids), -host(rec_d).astype(np.float64), 1, tag + " recommend")
    assert (host(rec_ids) >= 1).all()                      # the padding item is never recommended
    rank0, nel0, ti0, td0 = m.rank_full(seqs, target)      # nothing seen, no selection
    assert ti0 is None and td0 is None and np.array_equal(host(nel0), np.full(B, V - 2))
    check_bracket(-D, tol, eligibility(B, V - 1, target, None, None, 1), target, 0, host(rank0), None, None, 1, tag + " unmasked")

    # full_sort(fused=True) against full_sort() on the same batches; the second batch has a user with all but 5 items seen
    seqs2, dense2 = random_batch(r, B, L, V, heavy_row=7)
    batches = [(seqs, dense, target[:, None]), (seqs2, sp.csr_matrix(dense2), target[:, None])]
    tr = FusedStosaTrainer(m, [0.3] * cfg.num_layers, [0.2] * cfg.num_layers)
    want, ans_w = tr.full_sort(batches, topk=k)
    got, ans_g = tr.full_sort(batches, topk=k, fused=True)
    assert np.array_equal(ans_w, ans_g) and got.shape == want.shape == (2 * B, k) and got.dtype == want.dtype
    assert tr.fused_fallbacks == 1
    assert np.array_equal(got[B:], want[B:])               # the fallback batch: the two-pass result itself
    weaker = check_id_lists(got[:B], want[:B], D, tol, dense, k, tag)
    print(tag, "full_sort rows under the weaker rule:", weaker, "of", B)


def test_kl_model_raises():
    from oracle import stosa_oracle as so
    from adt_amd.stosa.trainer import FusedStosaTrainer
    g = np.load(os.path.join(GOLD, "stosa_kl_small.npz"))
    V, L, d, H, nl, nu = [int(x) for x in g["cfg"]]
    cfg = so.Cfg(V, L, d, H, nl, num_users=nu, pvn_weight=float(g["pvn_weight"]))
    m = build(cfg, so.init_params(cfg, int(g["seed"])), "kl")
    with pytest.raises(_lib.AdtError, match="wasserstein"):
        m.rank_full(g["input_ids"], None, None, 5)
    with pytest.raises(_lib.AdtError, match="wasserstein"):
        m.item_image()
    with pytest.raises(_lib.AdtError, match="wasserstein"):
        m.recommend(g["input_ids"], 5)
    tr = FusedStosaTrainer(m, [0.3] * nl, [0.2] * nl)
    with pytest.raises(_lib.AdtError, match="wasserstein"):
        tr.full_sort([(g["input_ids"], None, g["pos_ids"][:, -1:])], topk=5, fused=True)
    pred, _ = tr.full_sort([(g["input_ids"], None, g["pos_ids"][:, -1:])], topk=5)      # the two-pass path still serves KL
    assert pred.shape == (len(g["input_ids"]), 5)


# ---- 6. supernet ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ("c3", "l2"))
def test_supernet_rank_full_candidates(tag):
    from adt_amd.stosa.supernet import DisenDistSASupernet
    from adt_amd.supersearch import cand_to_block, get_shared
    from tools.gen_golden_inputs import seeded_params
    g = np.load(os.path.join(GOLD, "superstosa_%s.npz" % tag))
    V, L, d, H, nl, nu = [int(x) for x in g["cfg"]]
    a = Args()
    a.device, a.item_size, a.maxlen, a.hidden_units, a.num_heads, a.num_layers, a.num_users = DEV, V, L, d, H, nl, nu
    a.dropout, a.attention_dropout, a.pvn_weight, a.precision, a.distance_metric = 0.0, 0.0, float(g["pvn_weight"]), "f32", "wasserstein"
    m = DisenDistSASupernet(a, g["rec_choice"], g["ind_choice"])
    m.load_numpy(seeded_params({k: tuple(v.shape) for k, v in m.state_dict().items()}, int(g["seed"])))      # as tests/test_superwide_hip.py
    m.eval()
    rc, ic = g["rec_choice"], g["ind_choice"]
    r = np.random.RandomState(9)
    cands = [[float(x) for x in g["cand"]], [float(x) for x in g["cand2"]], [float(x) for x in r.rand(2 * nl)]]
    shared = [get_shared(rc, ic, cand_to_block(rc, ic, c)[0]) for c in cands]
    P_, B, k = len(cands), 9, 10
    seqs, dense = random_batch(r, B, L, V)
    target = r.randint(1, V, B).astype(np.int32)
    seen_all = np.tile(dense, (P_, 1))
    image = m.item_image()
    rank, nel, ti, td = m.rank_full_candidates(seqs, shared, target, seen_all, k, image, first_id=0)
    assert rank.shape == (P_ * B,) and ti.shape == (P_ * B, k)
    for p in range(P_):                                    # bit-equal to the single-candidate calls
        one = m.rank_full_candidates(seqs, shared[p:p + 1], target, dense, k, image, first_id=0)
        for x, y in zip((rank, nel, ti, td), one):
            assert torch.equal(x[p * B:(p + 1) * B].view(torch.int32), y.view(torch.int32)), p
    D = host(m.predict_full_candidates(seqs, shared)).astype(np.float64)
    tol = model_tol(m, m._last_state_candidates(seqs, shared), V)
    ip, ix = ops.seen_csr(seen_all, P_ * B, DEV)
    want = host(ops.topk_masked(m.predict_full_candidates(seqs, shared), k, ip, ix)).astype(np.int64)
    weaker = check_id_lists(host(ti).astype(np.int64), want, D, tol, seen_all, k, tag)
    print(tag, "candidate rows under the weaker rule:", weaker, "of", P_ * B)
    r_ip, r_ix = ops.seen_csr_host(seen_all, P_ * B)
    tgt_all = np.tile(target, P_)
    elig = eligibility(P_ * B, V - 1, tgt_all, r_ip, r_ix, 0)
    check_bracket(-D, tol, elig, tgt_all, k, host(rank), host(ti), -host(td).astype(np.float64), 0, tag)


# ---- 7. argument errors ----------------------------------------------------------------------------------------------------------------------
def test_pack_argument_errors():
    M = torch.zeros(4, 64, device=DEV)
    C = torch.ones(4, 64, device=DEV)
    ops.wdist_pack(M, C, True, -0.5)                                        # fine
    ops.wdist_pack(M[:, :60], C[:, :60], False, 1.0)                        # ld > d is fine
    with pytest.raises(_lib.AdtError):
        ops.wdist_pack(M[:, :62], C[:, :62], True, -0.5)                    # d not a multiple of 4
    flat_m, flat_c = torch.zeros(4 * 64 + 4, device=DEV), torch.ones(4 * 64 + 4, device=DEV)
    with pytest.raises(_lib.AdtError):
        ops.wdist_pack(flat_m[1:257].view(4, 64), flat_c[1:257].view(4, 64), True, -0.5)      # bases 4 bytes off a 16-byte boundary
    lib = _lib.load()
    img, nrm = torch.empty(4, 128, device=DEV), torch.empty(4, device=DEV)
    args = lambda ldi, ip=None: (ops._p(M), ops._p(C), 64, 4, 64, 1, ops._p(img) if ip is None else ip, ldi, ops._p(nrm), -0.5, ops._stream())
    assert lib.adt_wdist_pack(*args(128)) == 0
    assert lib.adt_wdist_pack(*args(124)) != 0 and b"ldi" in lib.adt_last_error()            # ldi < 2d
    assert lib.adt_wdist_pack(*args(128, ops._p(img.view(-1)[1:]))) != 0                      # misaligned image
    torch.cuda.synchronize()
