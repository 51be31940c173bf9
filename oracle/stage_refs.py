"""TEST INFRASTRUCTURE ONLY -- float64 restatements of the stage kernels that the model-level oracles reach only through whole training
steps: the supernet optimiser (adt_grad_sumsq / adt_adam_range / adt_adamw_range), adt_axpy, adt_log_softmax_*, adt_drop_lanes,
adt_lane_map, adt_item_scatter + adt_replica_reduce, adt_posemb_bwd and adt_logits_bwd_df.

Every function is written from the operation's definition (the comments of include/adt_hip.h, torch.optim.Adam / AdamW,
torch.nn.utils.clip_grad_norm_), in float64, with numpy only; none follows a kernel's loop structure.  Functions named *_terms return the
list of float64 addends of each output element (their sum is the value, the sum of their magnitudes scales the rounding bound); *_ref
return the value.  update_err / ulp_close / sum_excess are the comparisons shared by tests/test_direct_kernels_hip.py (GPU) and
tests/test_stage_refs_cpu.py (which shows that each of them rejects a wrong kernel).
"""
import numpy as np

from . import rng

U24 = 2.0 ** -24          # unit roundoff of float32 (half an ulp, relative)


def f32(x):
    """A Python scalar as the C ABI receives it: rounded to float32."""
    return float(np.float32(x))


def _f64(a):
    return np.asarray(a, dtype=np.float64)


# ---- comparisons ---------------------------------------------------------------------------------------------------------------------
def update_err(P0, P1, P1_ref, lr):
    """Largest error of the optimiser UPDATE P1 - P0 against P1_ref - P0, in units of lr.  P1 is the kernel's float32 result, so half an ulp
    of the stored P1 is owed to the store alone and is subtracted first (at |P| = 4 and lr = 1e-3 that half ulp is 2.4e-4 lr: an error
    scaled by max|P| would measure the parameters, not the step)."""
    P1 = np.asarray(P1)
    assert P1.dtype == np.float32 and P1.shape == np.shape(P0) == np.shape(P1_ref)
    assert np.isfinite(P1).all(), "non-finite parameters"
    err = np.abs((P1.astype(np.float64) - _f64(P0)) - (_f64(P1_ref) - _f64(P0)))
    err = np.maximum(err - 0.5 * np.spacing(np.abs(P1)).astype(np.float64), 0.0)
    return float(err.max()) / lr if err.size else 0.0


def sum_excess(got, terms, factor):
    """max over the elements of |got - sum(terms)| / (factor * sum|terms|) (0 / 0 counts as 0, x / 0 as inf): <= 1 means that `got` is
    within the bound.  terms: a list of float64 arrays (broadcastable to got's shape), or (sum, sum of magnitudes) already reduced."""
    got = np.asarray(got)
    assert np.isfinite(got).all(), "non-finite values"
    if isinstance(terms, tuple):
        want, mag = _f64(terms[0]), _f64(terms[1])
    else:
        terms = [np.broadcast_to(_f64(t), got.shape) for t in terms]
        want, mag = sum(terms), sum(np.abs(t) for t in terms)
    err = np.abs(got.astype(np.float64) - want)
    bound = np.broadcast_to(_f64(factor) * mag, err.shape)
    ratio = np.where(err == 0.0, 0.0, err / np.where(bound > 0, bound, 1.0))
    ratio = np.where((bound <= 0) & (err > 0), np.inf, ratio)
    return float(ratio.max()) if ratio.size else 0.0


def ulp_close(got, want_terms):
    """|got - sum(terms)| <= 2**-23 * sum|terms| in every element: what one multiply-add chain a * b + c owes in float32 whether the
    compiler fuses it or not (device code is built with contraction on, so bit equality with an unfused numpy expression is not owed).
    Every further addend is one more rounding: k > 2 terms are allowed k * 2**-24."""
    return sum_excess(got, want_terms, max(2, len(want_terms)) * U24) <= 1.0


# ---- supernet optimiser --------------------------------------------------------------------------------------------------------------
def adam_range_ref(P, G, M, V, gn2, l2, wd_dec, clip, lr, b1, b2, eps, t):
    """One torch.optim step on a flat range behind torch.nn.utils.clip_grad_norm_(clip) with the GLOBAL squared gradient norm gn2:
    coef = min(1, clip / (sqrt(gn2) + 1e-6)); torch.optim.Adam(weight_decay=l2) adds l2 * p to the CLIPPED gradient; torch.optim.AdamW
    (weight_decay=wd_dec) multiplies p by 1 - lr * wd_dec before the update.  t: this range's step count after the step.  The scalars are
    rounded to float32 first, as the C ABI receives them (1 - 0.98f ** t differs from 1 - 0.98 ** t by 1e-5 relative).
    Returns (P', M', V') in float64."""
    P, G, M, V = _f64(P), _f64(G), _f64(M), _f64(V)
    l2, wd_dec, clip, lr, b1, b2, eps, t = (f32(x) for x in (l2, wd_dec, clip, lr, b1, b2, eps, t))
    coef = min(1.0, clip / (np.sqrt(float(gn2)) + 1e-6))
    g = G * coef
    if wd_dec != 0.0:
        P = P * (1.0 - lr * wd_dec)
    if l2 != 0.0:
        g = g + l2 * P
    M1 = b1 * M + (1.0 - b1) * g
    V1 = b2 * V + (1.0 - b2) * g * g
    bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    P1 = P - (lr / bc1) * M1 / (np.sqrt(V1) / np.sqrt(bc2) + eps)
    return P1, M1, V1


# ---- elementwise ---------------------------------------------------------------------------------------------------------------------
def log_softmax_ref(X):
    """log_softmax over the last axis."""
    X = _f64(X)
    m = X.max(-1, keepdims=True)
    return X - (m + np.log(np.exp(X - m).sum(-1, keepdims=True)))


def log_softmax_bwd_ref(Y, dY, dX_old=None):
    """dX (+)= dY - softmax * sum(dY) with softmax = exp(Y)."""
    Y, dY = _f64(Y), _f64(dY)
    g = dY - np.exp(Y) * dY.sum(-1, keepdims=True)
    return g if dX_old is None else _f64(dX_old) + g


def axpy_terms(dst, src, alpha, accumulate, mask_ids=None, d=0):
    """dst = (accumulate ? dst : 0) + alpha * src * (mask_ids is None or mask_ids[i // d] != 0) on flat arrays."""
    src = _f64(src).reshape(-1)
    live = np.ones(src.size, bool) if mask_ids is None else np.repeat(np.asarray(mask_ids) != 0, d)[:src.size]
    terms = [f32(alpha) * src * live]
    if accumulate:
        terms.append(_f64(dst).reshape(-1))
    return terms


def axpy_ref(dst, src, alpha, accumulate, mask_ids=None, d=0):
    return sum(axpy_terms(dst, src, alpha, accumulate, mask_ids, d))


# ---- padded lanes --------------------------------------------------------------------------------------------------------------------
def lane_cols(lanes):
    """(live, true_col) of the d_pad = H * hd_pad columns of a padded row: head h owns columns [h * hd_pad, h * hd_pad + hd), which are
    columns [h * hd, (h + 1) * hd) of the true-width tensor."""
    H, hd, hd_pad = lanes
    c = np.arange(H * hd_pad)
    return (c % hd_pad) < hd, (c // hd_pad) * hd + c % hd_pad


def drop_scale(p):
    """Survivors of a dropout site are scaled by 1 / (1 - drop_prob(p)), drop_prob the rate quantised to 1 / 256 (oracle/rng.py).  The
    scale is a float32 by definition (DropCfg.scale is computed on the host in double and handed to the kernels as a float)."""
    return f32(1.0 / (1.0 - rng.drop_prob(p)))


def drop_lanes_terms(S, lanes, p, seed, site, row_offset, R=None, R2=None, mask_ids=None):
    """out = rowmask(R + R2 + dropout(S)) on the live lanes, 0 on the pad lanes and on the rows with mask_ids == 0; the keep decision of
    (row t, live column c) is that of element (t + row_offset) * (H * hd) + true_col(c) of the TRUE-width tensor.
    Returns ([keep * scale * S, R, R2] (absent ones left out), keep) with keep the boolean mask on the (T, d_pad) grid (True where p = 0)."""
    H, hd, _ = lanes
    S = _f64(S)
    T, dp = S.shape
    live, tcol = lane_cols(lanes)
    assert dp == live.size
    keep = np.ones((T, dp), bool)
    if rng.threshold(p) != 0:
        idx = (np.arange(T, dtype=np.int64)[:, None] + int(row_offset)) * (H * hd) + tcol[None, :]
        keep = rng.keep_mask(seed, site, idx, p)
    on = live[None, :] & (np.ones(T, bool) if mask_ids is None else np.asarray(mask_ids) != 0)[:, None]
    terms = [np.where(on & keep, S, 0.0) * (drop_scale(p) if rng.threshold(p) != 0 else 1.0)]
    for r in (R, R2):
        if r is not None:
            terms.append(np.where(on, _f64(r), 0.0))
    return terms, keep


def drop_lanes_ref(S, lanes, p, seed, site, row_offset, R=None, R2=None, mask_ids=None):
    return sum(drop_lanes_terms(S, lanes, p, seed, site, row_offset, R, R2, mask_ids)[0])


def lane_map_ref(padded, compact, index, scatter):
    """Gather: compact = padded[index]; scatter: padded[index] = compact (index injective).  Returns the array that changes (a copy)."""
    index = np.asarray(index, dtype=np.int64)
    if scatter:
        out = np.array(padded, copy=True)
        out[index] = np.asarray(compact)
        return out
    return np.asarray(padded)[index].copy()


# ---- item / positional table gradients -----------------------------------------------------------------------------------------------
def _row_keep(T, d, p, seed, site, row_offset):
    """Dropout factor keep * scale of a (T, d) tensor whose row t is row t + row_offset of the whole batch."""
    if rng.threshold(p) == 0:
        return np.ones((T, d))
    idx = (np.arange(T, dtype=np.int64)[:, None] + int(row_offset)) * d + np.arange(d)[None, :]
    return rng.keep_mask(seed, site, idx, p) * drop_scale(p)


def item_scatter_ref(ids, G, rowscale, scale, p, seed, site, row_offset, V1):
    """dE[ids[t]] += rowscale[t] * scale * dropmask[t] * G[t] over the rows with ids[t] != 0, into a zero (V1, d) table (row 0, the padding
    item, receives nothing).  Only the sum over the replicas is defined, so there is no replica here.
    Returns (dE, sum of the magnitudes of the addends, number of non-zero addends) per entry."""
    ids = np.asarray(ids).reshape(-1)
    G = _f64(G)
    T, d = G.shape
    c = G * _row_keep(T, d, p, seed, site, row_offset) * f32(scale)
    if rowscale is not None:
        c = c * _f64(rowscale)[:, None]
    c = c * (ids != 0)[:, None]
    out, mag, cnt = np.zeros((V1, d)), np.zeros((V1, d)), np.zeros((V1, d), np.int64)
    np.add.at(out, ids, c)
    np.add.at(mag, ids, np.abs(c))
    np.add.at(cnt, ids, (c != 0).astype(np.int64))
    return out, mag, cnt


def replica_reduce_ref(dst, rep):
    """dst += sum over the replicas; rep: (nrep, n)."""
    return _f64(dst) + _f64(rep).sum(0)


def posemb_bwd_ref(ids, dX, L, p, seed, site, row_offset):
    """dP[l] += sum_b dX[b, l] * dropmask * (ids[b, l] != 0).  Returns (sum, sum of magnitudes), both (L, d), to be added to the old dP."""
    ids = np.asarray(ids).reshape(-1)
    dX = _f64(dX)
    T, d = dX.shape
    c = dX * _row_keep(T, d, p, seed, site, row_offset) * (ids != 0)[:, None]
    c = c.reshape(T // L, L, d)
    return c.sum(0), np.abs(c).sum(0)


def logits_bwd_df_terms(E, pos, neg, dpos, dneg):
    """dF[t] = dpos[t] * E[pos[t]] + dneg[t] * E[neg[t]] (id 0 is an ordinary row here: its gradient is masked by dpos / dneg)."""
    E = _f64(E)
    return [_f64(dpos)[:, None] * E[np.asarray(pos)], _f64(dneg)[:, None] * E[np.asarray(neg)]]


def logits_bwd_df_ref(E, pos, neg, dpos, dneg):
    return sum(logits_bwd_df_terms(E, pos, neg, dpos, dneg))
