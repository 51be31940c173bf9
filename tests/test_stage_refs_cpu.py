"""The float64 references of oracle/stage_refs.py and the comparisons of tests/test_direct_kernels_hip.py, checked without a GPU:
the optimiser reference against torch.optim itself, and every comparison against a float32 numpy emulation of the kernel (accepted) and
against deliberately wrong variants of it (each rejected at the tolerance the GPU test asserts)."""
import numpy as np
import pytest
import torch

from oracle import rng
from oracle import stage_refs as sr

import test_direct_kernels_hip as gk

F = np.float32
OPT = gk.OPT


# ---- adam_range_ref is torch.optim.Adam / AdamW behind clip_grad_norm_ ------------------------------------------------------------------
@pytest.mark.parametrize("name", ["adam", "adamw"])
def test_adam_range_ref_is_torch_optim(name):
    case = gk.ADAM_CASE if name == "adam" else gk.ADAMW_CASE
    lr, b1, b2, eps, clip = (sr.f32(x) for x in (case["lr"], OPT["b1"], OPT["b2"], OPT["eps"], OPT["clip"]))
    P0, Gs = gk.optimiser_inputs(3001, seed=5)
    p = torch.nn.Parameter(torch.from_numpy(P0.astype(np.float64)))
    if name == "adam":
        opt = torch.optim.Adam([p], lr=lr, betas=(b1, b2), eps=eps, weight_decay=sr.f32(case["l2"]), foreach=False)
    else:
        opt = torch.optim.AdamW([p], lr=lr, betas=(b1, b2), eps=eps, weight_decay=sr.f32(case["wd"]), foreach=False)
    P, M, V = P0.astype(np.float64), np.zeros(3001), np.zeros(3001)
    clipped = []
    for t, g in enumerate(Gs, 1):
        g = g.astype(np.float64)
        p.grad = torch.from_numpy(g.copy())
        gn2 = float((g ** 2).sum())
        clipped.append(np.sqrt(gn2) > clip)
        torch.nn.utils.clip_grad_norm_([p], clip)
        opt.step()
        P, M, V = sr.adam_range_ref(P, g, M, V, gn2, case["l2"], case["wd"], clip, lr, b1, b2, eps, t)
        st = opt.state[p]
        for got, want in ((P, p.detach().numpy()), (M, st["exp_avg"].numpy()), (V, st["exp_avg_sq"].numpy())):
            assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max(), (name, t)
    assert clipped == [False, True, False]


# ---- the optimiser comparison rejects wrong optimisers ------------------------------------------------------------------------------------
ADAM_MUTANTS = ["bc_at_t_minus_1", "no_bc2", "no_clip", "l2_before_clip", "eps_inside_sqrt", "eps_over_sqrt_bc2"]
ADAMW_MUTANTS = ["decay_as_coupled_l2", "decay_after_update"]


def emulate_adam_range(P, G, M, V, gn2, l2, wd, clip, lr, b1, b2, eps, t, mutant=None):
    """adt_adam_range / adt_adamw_range in float32 numpy (unfused), or one of the wrong variants."""
    l2, wd, clip, lr, b1, b2, eps, t, one = F(l2), F(wd), F(clip), F(lr), F(b1), F(b2), F(eps), F(t), F(1)
    P, G, M, V = (np.asarray(a, F) for a in (P, G, M, V))
    coef = one if mutant == "no_clip" else min(one, clip / (np.sqrt(F(gn2)) + F(1e-6)))
    tb = t - one if mutant == "bc_at_t_minus_1" else t
    bc1, bc2 = one - b1 ** tb, one - b2 ** tb
    if mutant == "no_bc2":
        bc2 = one
    if mutant == "decay_as_coupled_l2":
        l2, wd = wd, F(0)
    g = (G + l2 * P) * coef if mutant == "l2_before_clip" else G * coef + l2 * P
    m = b1 * M + (one - b1) * g
    v = b2 * V + (one - b2) * g * g
    rs2 = one / np.sqrt(bc2)
    if mutant == "eps_inside_sqrt":
        den = np.sqrt(v + eps) * rs2
    elif mutant == "eps_over_sqrt_bc2":
        den = (np.sqrt(v) + eps) * rs2
    else:
        den = np.sqrt(v) * rs2 + eps
    upd = (lr / bc1) * m / den
    if mutant == "decay_after_update":
        p1 = (P - upd) * (one - lr * wd)
    else:
        p1 = P * (one - lr * wd) - upd
    assert p1.dtype == F and m.dtype == F and v.dtype == F
    return p1, m, v


@pytest.mark.parametrize("name", ["adam", "adamw"])
def test_update_err_rejects_wrong_optimisers(name):
    """Three steps of the GPU test's data (smaller, the clip lowered with it so that every step clips as it does there).  Per step the
    float32 emulation must pass the GPU test's tolerances and every wrong variant must miss the update tolerance in at least one step."""
    case, tol, mutants = (gk.ADAM_CASE, gk.ADAM_UPDATE_TOL, ADAM_MUTANTS) if name == "adam" else (gk.ADAMW_CASE, gk.ADAMW_UPDATE_TOL, ADAMW_MUTANTS)
    n, clip = 30001, 1.0
    P0, Gs = gk.optimiser_inputs(n, seed=6)
    assert np.abs(P0).max() <= 4.5
    P, M, V = P0, np.zeros(n, F), np.zeros(n, F)
    args = lambda gn2, t: (gn2, case["l2"], case["wd"], clip, case["lr"], OPT["b1"], OPT["b2"], OPT["eps"], t)
    worst = {m: 0.0 for m in mutants}
    for t, G in enumerate(Gs, 1):
        gn2 = float((G.astype(np.float64) ** 2).sum())
        assert np.sqrt(gn2) > clip
        Pr, Mr, Vr = sr.adam_range_ref(P, G, M, V, *args(gn2, t))
        P1, M1, V1 = emulate_adam_range(P, G, M, V, *args(gn2, t))
        u = sr.update_err(P, P1, Pr, case["lr"])
        mt, vt = gk.moment_terms(P, G, M, V, gn2, case["l2"], case["wd"], clip, case["lr"], OPT["b1"], OPT["b2"])
        print("%s step %d: emulation update err %.3e lr, M' %.2f and V' %.2f units of 2**-24" % (name, t, u, gk.moments_close(M1, mt, 1), gk.moments_close(V1, vt, 1)))
        assert u <= tol and gk.moments_close(M1, mt, gk.M_ULPS) <= 1.0 and gk.moments_close(V1, vt, gk.V_ULPS) <= 1.0
        # the moments are compared at all: a wrong b2 or a missing (1 - b2) is 2 % of V', five orders above the bound
        assert gk.moments_close((V1 * F(1.02)).astype(F), vt, gk.V_ULPS) > 1e3 and gk.moments_close((M1 * F(0.999)).astype(F), mt, gk.M_ULPS) > 1.0 or not M1.any()
        for m in mutants:
            if m == "bc_at_t_minus_1" and t == 1:
                continue                       # 1 - b ** 0 = 0: not finite, which update_err refuses outright
            with np.errstate(all="ignore"):
                Pm, _, _ = emulate_adam_range(P, G, M, V, *args(gn2, t), mutant=m)
            worst[m] = max(worst[m], sr.update_err(P, Pm, Pr, case["lr"]))
        P, M, V = P1, M1, V1
    print(name, "tolerance %.3e lr; wrong variants:" % tol, {m: "%.3e" % w for m, w in worst.items()})
    for m, w in worst.items():
        assert w > tol, "%s: update error %.3e lr passes the tolerance %.3e lr" % (m, w, tol)
    with np.errstate(all="ignore"), pytest.raises(AssertionError):
        sr.update_err(P0, emulate_adam_range(P0, Gs[0], M * 0, V * 0, *args(1.0, 1), mutant="bc_at_t_minus_1")[0], P0, case["lr"])


def test_update_err_and_ulp_close_units():
    P0 = np.array([4.0, 0.5, -1e-3], F)
    step = np.array([1e-3, -1e-3, 1e-3])
    ref = P0.astype(np.float64) - step
    assert sr.update_err(P0, ref.astype(F), ref, 1e-3) == 0.0                       # the store's own rounding is not an error
    off = (ref - np.array([0.0, 0.0, 1e-5])).astype(F)
    assert 0.9e-2 < sr.update_err(P0, off, ref, 1e-3) < 1.1e-2                       # 1 % of lr on the smallest parameter is seen as such
    a, b, c = F(1.2345678), F(-0.37), F(0.7654321)
    exact = float(a) * float(b) + float(c)
    terms = [np.array([float(a) * float(b)]), np.array([float(c)])]
    assert sr.ulp_close(np.array([F(a * b) + c], F), terms) and sr.ulp_close(np.array([exact], F), terms)      # unfused and fused both pass
    bad = np.array([exact * (1 + 1e-6)], F)
    assert not sr.ulp_close(bad, terms)
    assert sr.sum_excess(np.array([1.0], F), [np.array([0.0])], 1.0) == np.inf and sr.sum_excess(np.array([0.0], F), [np.array([0.0])], 1.0) == 0.0


# ---- log_softmax ------------------------------------------------------------------------------------------------------------------------------
def lsm_f32(X, shift=True):
    m = X.max(1, keepdims=True) if shift else np.zeros((X.shape[0], 1), F)
    with np.errstate(all="ignore"):
        return ((X - m) - np.log(np.exp(X - m).sum(1, keepdims=True, dtype=F))).astype(F)


@pytest.mark.parametrize("H", [1, 2, 5, 8])
def test_log_softmax_comparison_rejects_wrong_kernels(H):
    X = gk.lsm_rows(1000, H)
    Y = lsm_f32(X)
    excess, abs_small = gk.lsm_fwd_errors(X, Y)
    assert excess <= gk.LSM_FN_TOL and abs_small <= gk.LSM_ABS_TOL, (excess, abs_small)
    # no max shift: the rows at +-1e4 overflow / underflow
    excess, abs_small = gk.lsm_fwd_errors(X, lsm_f32(X, shift=False))
    assert not (excess <= gk.LSM_FN_TOL and abs_small <= gk.LSM_ABS_TOL)
    big = np.abs(X).max(1) > 100
    Yb = Y.copy()
    Yb[big] = lsm_f32(X, shift=False)[big]
    assert not gk.lsm_fwd_errors(X, Yb)[0] <= gk.LSM_FN_TOL, "the large-magnitude rows alone must give it away"
    # backward: softmax * dY instead of softmax * sum(dY)
    dY, old = gk.lsm_bwd_inputs(1000, H, Y)
    sm = np.exp(Y)
    for o in (None, old):
        base = F(0) if o is None else o
        good = (base + (dY - sm * dY.sum(1, keepdims=True, dtype=F))).astype(F)
        assert max(gk.lsm_bwd_ratios(X, Y, dY, o, good)) <= 1.0
        if H > 1:                                  # (with H = 1 the two coincide)
            wrong = (base + (dY - sm * dY)).astype(F)
            value, rowsum, plain = gk.lsm_bwd_ratios(X, Y, dY, o, wrong)
            assert value > 1.0 and rowsum > 1.0 and plain > 1.0


# ---- drop_lanes ---------------------------------------------------------------------------------------------------------------------------------
def drop_lanes_f32(S, R, R2, ids, lanes, p, seed, site, row_offset, mutant=None):
    H, hd, hd_pad = lanes
    live, tcol = sr.lane_cols(lanes)
    T, dp = S.shape
    col = np.arange(dp) if mutant == "padded_width_index" else tcol
    width = dp if mutant == "padded_width_index" else H * hd
    keep = np.ones((T, dp), bool)
    if p:
        keep = rng.keep_mask(seed, site, (np.arange(T, dtype=np.int64)[:, None] + row_offset) * width + col[None, :], p)
    ks = F(sr.drop_scale(p))
    on = live[None, :] & (np.ones(T, bool) if ids is None else ids != 0)[:, None]
    with np.errstate(over="ignore"):
        if mutant == "dropout_on_residual":
            w = S + (R if R is not None else 0) + (R2 if R2 is not None else 0)
            w = np.where(keep, w * ks, F(0))
        else:
            w = np.where(keep, S * ks, F(0))
            for r_ in (R, R2):
                if r_ is not None:
                    w = w + r_
    return np.where(on, w, F(0)).astype(F)


@pytest.mark.parametrize("lanes", [(2, 25, 32), (3, 50, 64), (1, 100, 128)])
@pytest.mark.parametrize("p", [0.25, 0.5])
def test_drop_lanes_comparison_rejects_wrong_kernels(lanes, p):
    r = np.random.RandomState(3)
    T, seed, site, row_offset = 37, 4321, 19, 1000
    _, S = gk.lanes_buffer(r, T, lanes)
    _, R = gk.lanes_buffer(r, T, lanes)
    ids = np.where(r.rand(T) < 0.3, 0, 5).astype(np.int32)
    for R_, ids_ in ((None, None), (R, ids)):
        gk.check_drop_lanes(drop_lanes_f32(S, R_, None, ids_, lanes, p, seed, site, row_offset), S, R_, None, ids_, lanes, p, seed, site, row_offset)
        with pytest.raises(AssertionError):
            gk.check_drop_lanes(drop_lanes_f32(S, R_, None, ids_, lanes, p, seed, site, row_offset, "padded_width_index"), S, R_, None, ids_, lanes, p, seed, site, row_offset)
    with pytest.raises(AssertionError):
        gk.check_drop_lanes(drop_lanes_f32(S, R, None, ids, lanes, p, seed, site, row_offset, "dropout_on_residual"), S, R, None, ids, lanes, p, seed, site, row_offset)
    with pytest.raises(AssertionError):      # a pad lane that leaks its input
        leak = drop_lanes_f32(S, None, None, None, lanes, p, seed, site, row_offset)
        leak[3, np.flatnonzero(~sr.lane_cols(lanes)[0])[0]] = F(1e-30)
        gk.check_drop_lanes(leak, S, None, None, None, lanes, p, seed, site, row_offset)


# ---- table gradients ----------------------------------------------------------------------------------------------------------------------------
def scatter_f32(ids, G, rs, scale, p, seed, site, row_offset, V1, prefill, order, skip_row0=True, overwrite=False):
    """item_scatter + replica_reduce in float32, the rows added in the given order."""
    T, d = G.shape
    k = sr._row_keep(T, d, p, seed, site, row_offset).astype(F)
    acc = np.zeros((V1, d), F)
    for t in order:
        if (ids[t] == 0 and skip_row0) or (rs is not None and rs[t] == 0):
            continue
        acc[ids[t]] += (G[t] * ((F(1) if rs is None else rs[t]) * F(scale))) * k[t]
    return acc if overwrite else prefill + acc


def rejected(ratio):
    """A comparison rejects by raising (bits that had to stay) or by a ratio above 1."""
    try:
        return ratio() > 1.0
    except AssertionError:
        return True


@pytest.mark.parametrize("p", [0.0, 0.25])
def test_table_grad_comparison_rejects_wrong_kernels(p):
    r = np.random.RandomState(4)
    L, V, d = 43, 40, 52
    T = 7 * L
    ids = r.randint(0, V + 1, size=T).astype(np.int32)
    ids[r.choice(T, T // 2, replace=False)] = 17
    ids[:3] = 0
    G, rs = r.randn(T, d).astype(F), r.randn(T).astype(F)
    rs[::5] = 0
    prefill = r.randn(V + 1, d).astype(F)
    want, mag, cnt = sr.item_scatter_ref(ids, G, rs, 8.0, p, 777, 7, 3 * L, V + 1)
    for order in (np.arange(T), np.arange(T)[::-1], r.permutation(T)):
        good = scatter_f32(ids, G, rs, 8.0, p, 777, 7, 3 * L, V + 1, prefill, order)
        assert gk.table_grad_ratio(good, prefill, want, mag, cnt + 3) <= 1.0
    order = np.arange(T)
    row0 = scatter_f32(ids, G, rs, 8.0, p, 777, 7, 3 * L, V + 1, prefill, order, skip_row0=False)      # row 0 is the padding item: nothing is added to it
    assert rejected(lambda: gk.table_grad_ratio(row0, prefill, want, mag, cnt + 3))
    wrong = scatter_f32(ids, G, rs, 8.0, p, 777, 7, 3 * L, V + 1, prefill, order, overwrite=True)      # replica_reduce that overwrites dst
    assert rejected(lambda: gk.table_grad_ratio(wrong, prefill, want, mag, cnt + 3)), "an overwriting replica_reduce passes"
    # posemb_bwd without the ids != 0 mask
    B = 7
    dX = G
    wantp, magp = sr.posemb_bwd_ref(ids, dX, L, p, 99, 3, 5 * L)
    k = sr._row_keep(T, d, p, 99, 3, 5 * L).astype(F)
    pre = r.randn(L, d).astype(F)
    masked = (dX * k * (ids != 0)[:, None]).reshape(B, L, d)
    good, wrong = pre.copy(), pre.copy()
    for b in range(B):
        good += masked[b]
        wrong += (dX * k).reshape(B, L, d)[b]
    assert gk.table_grad_ratio(good, pre, wantp, magp, B + 1) <= 1.0
    assert rejected(lambda: gk.table_grad_ratio(wrong, pre, wantp, magp, B + 1))
