"""Torch-tensor wrappers over the C ABI (include/adt_hip.h).  Tensors must be CUDA (HIP) fp32/int32 and
contiguous in their last dimension; every call enqueues on torch's current stream.  Nothing here computes on
the host: a missing libadt_hip.so or a CPU tensor is an error, not a fallback.
"""
import ctypes

import torch

from . import _lib

PREC_F32, PREC_BF16 = 0, 1


def _p(t):
    if t is None:
        return None
    if not t.is_cuda:
        raise _lib.AdtError("adt_amd.ops: tensor is not on the GPU (no CPU fallback)")
    return ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ld(t):
    return t.stride(-2) if t is not None and t.dim() >= 2 else 0


def _f32(t):
    assert t.dtype == torch.float32 and t.stride(-1) == 1, (t.dtype, t.stride())
    return t


def _i32(t):
    assert t.dtype == torch.int32 and t.is_contiguous()
    return t


def embed_fwd(ids, E, P, L, p, seed, site, row_offset=0):
    T = ids.numel()
    d = E.shape[1]
    X = torch.empty(T, d, device=E.device, dtype=torch.float32)
    _lib.check(_lib.load().adt_embed_fwd(_p(_i32(ids)), _p(_f32(E)), _p(_f32(P)), T, L, d, float(p), _p(seed), site,
                                         row_offset, _p(X), _stream()), "embed_fwd")
    return X


def embed_bwd(ids, dX, L, p, seed, site, dE, dP, row_offset=0):
    T, d = dX.shape
    _lib.check(_lib.load().adt_embed_bwd(_p(_i32(ids)), _p(_f32(dX)), T, L, d, float(p), _p(seed), site, row_offset,
                                         _p(dE), _p(dP), _stream()), "embed_bwd")


def embed_bwd3(seq, dec, pos, dXs, dXd, F, dpos, L, p, seed, site_seq, site_dec, dE_rep, dP, nrep=1, rep_stride=0, row_offset=0):
    """Encoder + decoder embedding gradients and the positive-logit rows into the item-table replicas in one pass (adt_embed_bwd3, d = 64)."""
    T = dXs.shape[0]
    _lib.check(_lib.load().adt_embed_bwd3(_p(_i32(seq)), _p(_i32(dec)), _p(_i32(pos)), _p(_f32(dXs)), _p(_f32(dXd)), _p(_f32(F)), _p(_f32(dpos)), T, L,
                                          float(p), _p(seed), site_seq, site_dec, row_offset, _p(dP), _p(dE_rep), nrep, rep_stride, _stream()), "embed_bwd3")


def layernorm_fwd(X, gamma, beta, eps):
    T, d = X.shape
    Y = torch.empty(T, d, device=X.device, dtype=torch.float32)
    _lib.check(_lib.load().adt_layernorm_fwd(_p(_f32(X)), _ld(X), _p(gamma), _p(beta), eps, T, d, _p(Y), d, _stream()), "ln_fwd")
    return Y


def layernorm_bwd(dY, X, gamma, eps, dX, accumulate, dgamma, dbeta):
    T, d = X.shape
    _lib.check(_lib.load().adt_layernorm_bwd(_p(_f32(dY)), _ld(dY), _p(_f32(X)), _ld(X), _p(gamma), eps, T, d, _p(dX), _ld(dX),
                                             int(accumulate), _p(dgamma), _p(dbeta), _stream()), "ln_bwd")


def linear_fwd(prec, X, W, b, Y=None, p=0.0, seed=None, site=0, row_offset=0, relu=False, R1=None, R2=None, mask_ids=None):
    T, K = X.shape
    N = W.shape[0]
    if Y is None:
        Y = torch.empty(T, N, device=X.device, dtype=torch.float32)
    _lib.check(_lib.load().adt_linear_fwd(prec, _p(_f32(X)), _ld(X), _p(_f32(W)), _p(b), T, K, N, _p(Y), _ld(Y), float(p), _p(seed),
                                          site, row_offset, int(relu), _p(R1), _ld(R1), _p(R2), _ld(R2), _p(mask_ids), _stream()),
               "linear_fwd")
    return Y


def linear_bwd(prec, dY, X, W, dW, db, dX=None, beta=False, mask_ids=None, p=0.0, seed=None, site=0, row_offset=0, U=None,
               Radd=None, radd_ids=None):
    T, K = X.shape
    N = W.shape[0]
    _lib.check(_lib.load().adt_linear_bwd(prec, _p(_f32(dY)), _ld(dY), _p(_f32(X)), _ld(X), _p(_f32(W)), T, K, N, _p(mask_ids),
                                          float(p), _p(seed), site, row_offset, _p(U), _ld(U), _p(dX), _ld(dX), int(beta), _p(Radd),
                                          _ld(Radd), _p(radd_ids), _p(dW), _p(db), _stream()), "linear_bwd")


def attn_fwd(prec, Q, K, V, B, H, L, causal=True, p=0.0, seed=None, site=0, b_offset=0, mask=None):
    """Q, K, V: (B*L, >= H*hd) views (head h in columns [h*hd, (h+1)*hd)); returns O (B*L, H*hd), LSE (B*H*L)."""
    d = Q.shape[1]
    hd = d // H
    O = torch.empty(B * L, d, device=Q.device, dtype=torch.float32)
    LSE = torch.empty(B * H * L, device=Q.device, dtype=torch.float32)
    _lib.check(_lib.load().adt_attn_fwd(prec, _p(_f32(Q)), _ld(Q), _p(_f32(K)), _ld(K), _p(_f32(V)), _ld(V), B, H, L, hd, int(causal),
                                        float(p), _p(seed), site, b_offset, _p(O), d, _p(LSE), _p(mask), _stream()), "attn_fwd")
    return O, LSE


def attn_bwd(prec, Q, K, V, O, LSE, dO, B, H, L, causal=True, p=0.0, seed=None, site=0, b_offset=0, mask=None, out=None):
    d = Q.shape[1]
    hd = d // H
    if out is None:
        dQ = torch.empty(B * L, d, device=Q.device, dtype=torch.float32)
        dK = torch.empty_like(dQ)
        dV = torch.empty_like(dQ)
    else:
        dQ, dK, dV = out
    _lib.check(_lib.load().adt_attn_bwd(prec, _p(_f32(Q)), _ld(Q), _p(_f32(K)), _ld(K), _p(_f32(V)), _ld(V), _p(_f32(O)), _ld(O),
                                        _p(LSE), _p(_f32(dO)), _ld(dO), B, H, L, hd, int(causal), float(p), _p(seed), site, b_offset,
                                        _p(dQ), _ld(dQ), _p(dK), _ld(dK), _p(dV), _ld(dV), _p(mask), _stream()), "attn_bwd")
    return dQ, dK, dV


def headcls_fwd(O, Ws, bs, B, L):
    H, hd = Ws.shape
    rec = torch.empty(L * B, H, H, device=O.device, dtype=torch.float32)
    _lib.check(_lib.load().adt_headcls_fwd(_p(_f32(O)), _ld(O), _p(Ws), _p(bs), B, L, H, hd, _p(rec), _stream()), "headcls_fwd")
    return rec


def headcls_bwd(O, Ws, rec, drec, B, L, dO, dWs, dbs):
    H, hd = Ws.shape
    _lib.check(_lib.load().adt_headcls_bwd(_p(_f32(O)), _ld(O), _p(Ws), _p(rec), _p(drec), B, L, H, hd, _p(dO), _ld(dO), _p(dWs),
                                           _p(dbs), _stream()), "headcls_bwd")


def logits_fwd(F, E, pos, neg):
    T, d = F.shape
    pl = torch.empty(T, device=F.device, dtype=torch.float32)
    nl = torch.empty_like(pl)
    _lib.check(_lib.load().adt_logits_fwd(_p(_f32(F)), _ld(F), _p(E), _p(_i32(pos)), _p(_i32(neg)), T, d, _p(pl), _p(nl), _stream()),
               "logits_fwd")
    return pl, nl


def logits_bwd(F, E, pos, neg, dpos, dneg, dE):
    T, d = F.shape
    dF = torch.empty(T, d, device=F.device, dtype=torch.float32)
    _lib.check(_lib.load().adt_logits_bwd(_p(_f32(F)), _ld(F), _p(E), _p(_i32(pos)), _p(_i32(neg)), _p(dpos), _p(dneg), T, d, _p(dF),
                                          d, _p(dE), _stream()), "logits_bwd")
    return dF


def item_scatter(ids, G, rowscale, scale, p, seed, site, row_offset, rep, nrep, rep_stride):
    """rep[wave % nrep][ids[row]] += rowscale[row] * scale * dropmask * G[row]  (rows with id 0 skipped); see adt_item_scatter."""
    T, d = G.shape
    _lib.check(_lib.load().adt_item_scatter(_p(_i32(ids)), _p(_f32(G)), _ld(G), _p(rowscale), T, d, float(scale), float(p), _p(seed), site, row_offset,
                                            _p(rep), nrep, rep_stride, _stream()), "item_scatter")


def replica_reduce(dE, rep, nrep, rep_stride):
    _lib.check(_lib.load().adt_replica_reduce(_p(dE), _p(rep), dE.numel(), nrep, rep_stride, _stream()), "replica_reduce")


def posemb_bwd(ids, dX, L, p, seed, site, row_offset, dP):
    T, d = dX.shape
    _lib.check(_lib.load().adt_posemb_bwd(_p(_i32(ids)), _p(_f32(dX)), T, L, d, float(p), _p(seed), site, row_offset, _p(dP), _stream()), "posemb_bwd")


def logits_bwd_df(E, pos, neg, dpos, dneg):
    T, d = pos.numel(), E.shape[1]
    dF = torch.empty(T, d, device=E.device, dtype=torch.float32)
    _lib.check(_lib.load().adt_logits_bwd_df(_p(E), _p(_i32(pos)), _p(_i32(neg)), _p(dpos), _p(dneg), T, d, _p(dF), d, _stream()), "logits_bwd_df")
    return dF


def bce_seed(pos_logits, neg_logits, pos, norms, loss2):
    T = pos_logits.numel()
    dpos = torch.empty(T, device=pos_logits.device, dtype=torch.float32)
    dneg = torch.empty_like(dpos)
    _lib.check(_lib.load().adt_bce_seed(_p(pos_logits), _p(neg_logits), _p(_i32(pos)), T, _p(norms), _p(dpos), _p(dneg), _p(loss2),
                                        _stream()), "bce_seed")
    return dpos, dneg


def mse_seed(A, Bm, lam, norms, GA, accumulate_a, GB, loss1):
    _lib.check(_lib.load().adt_mse_seed(_p(A), _p(Bm), A.numel(), float(lam), _p(norms), _p(GA), int(accumulate_a), _p(GB), _p(loss1),
                                        _stream()), "mse_seed")


def nll_seed(rec, H, lam2, norms, drec, loss1):
    _lib.check(_lib.load().adt_nll_seed(_p(rec), rec.numel() // (H * H), H, float(lam2), _p(norms), _p(drec), _p(loss1), _stream()),
               "nll_seed")


def clip_adam(P, G, M, V, nE, wd, clip, lr, b1, b2, eps, scal, grad_scale=1.0, n=None):
    n = P.numel() if n is None else n
    _lib.check(_lib.load().adt_clip_adam(_p(P), _p(G), _p(M), _p(V), n, nE, float(wd), float(clip), float(lr), float(b1), float(b2),
                                         float(eps), float(grad_scale), _p(scal), _stream()), "clip_adam")


def clip_adam_pre(P, G, M, V, nE, wd, clip, lr, b1, b2, eps, scal, grad_scale=1.0, n=None):
    """clip_adam for a step opened by SASRecADT.run_step_begin (||E||^2 partials and zeroed slots already in scal)."""
    n = P.numel() if n is None else n
    _lib.check(_lib.load().adt_clip_adam_pre(_p(P), _p(G), _p(M), _p(V), n, nE, float(wd), float(clip), float(lr), float(b1), float(b2),
                                             float(eps), float(grad_scale), _p(scal), _stream()), "clip_adam_pre")


def score_rank(F, ldf, E, cand, B, C, want_rank=True):
    d = E.shape[1]
    logits = torch.empty(B, C, device=E.device, dtype=torch.float32)
    rank = torch.empty(B, device=E.device, dtype=torch.int32) if want_rank else None
    _lib.check(_lib.load().adt_score_rank(_p(F), ldf, _p(E), _p(cand), B, C, d, _p(logits), _p(rank), _stream()), "score_rank")
    return logits, rank


# ---- general ("wide") stage kernels: BERT4Rec-ADT, STOSA-ADT (include/adt_hip.h) ------------------------------------
ACT_NONE, ACT_RELU, ACT_GELU, ACT_ELU, ACT_ELU1 = 0, 1, 2, 3, 4


def dense_fwd(prec, X, W, b=None, act=ACT_NONE, save_u=False, p=0.0, seed=None, site=0, row_offset=0, R=None, mask_ids=None, Y=None,
              t_dev=None, ldy=None, R2=None):
    """Y = mask(R + dropout(act(X W^T + b))); returns (Y, U) with U the saved pre-activation (or None)."""
    T, K = X.shape
    N = W.shape[0]
    if Y is None:
        ldy = N if ldy is None else ldy
        Y = torch.empty(T, ldy, device=X.device, dtype=torch.float32)[:, :N]
    U = torch.empty(T, N, device=X.device, dtype=torch.float32) if save_u else None
    _lib.check(_lib.load().adt_dense_fwd(prec, _p(_f32(X)), _ld(X), _p(_f32(W)), _ld(W), _p(b), T, K, N, act, _p(U), _ld(U), float(p), _p(seed),
                                         site, row_offset, _p(R), _ld(R), _p(R2), _ld(R2), _p(mask_ids), _p(Y), _ld(Y), _p(t_dev), _stream()), "dense_fwd")
    return Y, U


_DENSE_WS = {}


def _ensure_dense_ws(device):
    """Scratch of the 256-wide stage kernels (adt_dense_workspace: private partials of the weight gradients): one 64 MiB buffer per device, kept for the process.  The library holds ONE pointer, so it is re-registered
    when the calls move to another device (one process per GPU is the normal case and registers once, before any graph capture: the
    trainers warm up eagerly)."""
    if _DENSE_WS.get("current") == device:
        return
    ws = _DENSE_WS.get(device)
    if ws is None:
        ws = _DENSE_WS[device] = torch.empty(64 << 20, device=device, dtype=torch.uint8)
    _lib.check(_lib.load().adt_dense_workspace(_p(ws), ws.numel()), "dense_workspace")
    _DENSE_WS["current"] = device


def dense_bwd(prec, dY, X, W, dW=None, db=None, dX=None, beta=False, act=ACT_NONE, U=None, p=0.0, seed=None, site=0, row_offset=0,
              mask_ids=None, t_dev=None):
    """G = dY * mask * dropmask * act'(U); dX (+)= G W; dW += G^T X; db += colsum(G)."""
    T, N = dY.shape
    K = W.shape[1]
    if dW is not None and _lib.load().adt_dense_bwd_ws_bytes(prec, T, K, N) > 0:
        _ensure_dense_ws(dY.device)      # 256-wide layers and 64 x 64 blocks: private partials + an ordered sum instead of an atomic flush
    _lib.check(_lib.load().adt_dense_bwd(prec, _p(_f32(dY)), _ld(dY), T, K, N, _p(mask_ids), float(p), _p(seed), site, row_offset, act, _p(U),
                                         _ld(U), _p(X), _ld(X), _p(_f32(W)), _ld(W), _p(dX), _ld(dX), int(beta), _p(dW), _ld(dW) if dW is not None else 0,
                                         _p(db), _p(t_dev), _stream()), "dense_bwd")


def attn_masked_fwd(prec, Q, K, V, B, H, L, causal=False, key_ids=None, fill=-1e9, p=0.0, seed=None, site=0, b_offset=0, scale=None):
    """scale: score scale when it is not 1 / sqrt(hd) (heads padded with zero lanes keep 1 / sqrt(true head size))."""
    d = Q.shape[1]
    hd = d // H
    O = torch.empty(B * L, d, device=Q.device, dtype=torch.float32)
    LSE = torch.empty(B * H * L, device=Q.device, dtype=torch.float32)
    args = [prec, _p(_f32(Q)), _ld(Q), _p(_f32(K)), _ld(K), _p(_f32(V)), _ld(V), B, H, L, hd, int(causal), _p(key_ids), float(fill), float(p),
            _p(seed), site, b_offset, _p(O), d, _p(LSE), _stream()]
    if scale is None:
        _lib.check(_lib.load().adt_attn_masked_fwd(*args), "attn_masked_fwd")
    else:      # the scaled entry point takes the scale after hd
        _lib.check(_lib.load().adt_attn_masked_scaled_fwd(*args[:11], float(scale), *args[11:]), "attn_masked_scaled_fwd")
    return O, LSE


def attn_masked_bwd(prec, Q, K, V, O, LSE, dO, B, H, L, causal=False, key_ids=None, fill=-1e9, p=0.0, seed=None, site=0, b_offset=0, out=None,
                    scale=None):
    d = Q.shape[1]
    hd = d // H
    if out is None:
        dQ = torch.empty(B * L, d, device=Q.device, dtype=torch.float32)
        dK = torch.empty_like(dQ)
        dV = torch.empty_like(dQ)
    else:
        dQ, dK, dV = out
    args = [prec, _p(_f32(Q)), _ld(Q), _p(_f32(K)), _ld(K), _p(_f32(V)), _ld(V), _p(_f32(O)), _ld(O), _p(LSE), _p(_f32(dO)), _ld(dO), B, H, L, hd,
            int(causal), _p(key_ids), float(fill), float(p), _p(seed), site, b_offset, _p(dQ), _ld(dQ), _p(dK), _ld(dK), _p(dV), _ld(dV), _stream()]
    if scale is None:
        _lib.check(_lib.load().adt_attn_masked_bwd(*args), "attn_masked_bwd")
    else:
        _lib.check(_lib.load().adt_attn_masked_scaled_bwd(*args[:16], float(scale), *args[16:]), "attn_masked_scaled_bwd")
    return dQ, dK, dV


def attn_masked_max_len(hd):
    """The longest sequence attn_masked_fwd / attn_masked_bwd take at head size hd (0: a head size they do not take); attn_long_* go on to 1024."""
    return _lib.load().adt_attn_masked_max_len(int(hd))


def attn_long_fwd(prec, Q, K, V, B, H, L, causal=False, key_ids=None, fill=-1e9, p=0.0, seed=None, site=0, b_offset=0, scale=None):
    """attn_masked_fwd for 1 <= L <= 1024 (every head size streamed); same arguments and results."""
    d = Q.shape[1]
    hd = d // H
    O = torch.empty(B * L, d, device=Q.device, dtype=torch.float32)
    LSE = torch.empty(B * H * L, device=Q.device, dtype=torch.float32)
    scale = float(hd) ** -0.5 if scale is None else scale
    _lib.check(_lib.load().adt_attn_long_fwd(prec, _p(_f32(Q)), _ld(Q), _p(_f32(K)), _ld(K), _p(_f32(V)), _ld(V), B, H, L, hd, float(scale), int(causal),
                                             _p(key_ids), float(fill), float(p), _p(seed), site, b_offset, _p(O), d, _p(LSE), _stream()), "attn_long_fwd")
    return O, LSE


def attn_long_bwd(prec, Q, K, V, O, LSE, dO, B, H, L, causal=False, key_ids=None, fill=-1e9, p=0.0, seed=None, site=0, b_offset=0, out=None,
                  scale=None):
    d = Q.shape[1]
    hd = d // H
    if out is None:
        dQ = torch.empty(B * L, d, device=Q.device, dtype=torch.float32)
        dK = torch.empty_like(dQ)
        dV = torch.empty_like(dQ)
    else:
        dQ, dK, dV = out
    scale = float(hd) ** -0.5 if scale is None else scale
    _lib.check(_lib.load().adt_attn_long_bwd(prec, _p(_f32(Q)), _ld(Q), _p(_f32(K)), _ld(K), _p(_f32(V)), _ld(V), _p(_f32(O)), _ld(O), _p(LSE),
                                             _p(_f32(dO)), _ld(dO), B, H, L, hd, float(scale), int(causal), _p(key_ids), float(fill), float(p), _p(seed),
                                             site, b_offset, _p(dQ), _ld(dQ), _p(dK), _ld(dK), _p(dV), _ld(dV), _stream()), "attn_long_bwd")
    return dQ, dK, dV


def embed_sum_fwd(ids, E, P, L, S0=None, scale=1.0):
    T = ids.numel()
    d = E.shape[1]
    X = torch.empty(T, d, device=E.device, dtype=torch.float32)
    _lib.check(_lib.load().adt_embed_sum_fwd(_p(_i32(ids)), _p(_f32(E)), _p(_f32(P)), _p(S0), float(scale), T, L, d, _p(X), _stream()), "embed_sum_fwd")
    return X


def dropact_fwd(X, p, seed, site, idx_offset=0, act=ACT_NONE):
    Y = torch.empty_like(X)
    _lib.check(_lib.load().adt_dropact_fwd(_p(_f32(X)), X.numel(), float(p), _p(seed), site, idx_offset, act, _p(Y), _stream()), "dropact_fwd")
    return Y


def dropact_bwd(dY, X, p, seed, site, dX, accumulate, idx_offset=0, act=ACT_NONE):
    _lib.check(_lib.load().adt_dropact_bwd(_p(_f32(dY)), _p(_f32(X)), X.numel(), float(p), _p(seed), site, idx_offset, act, _p(dX), int(accumulate),
                                           _stream()), "dropact_bwd")


def gather_rows(F, rows, M=None, m_dev=None):
    M = rows.numel() if M is None else M
    d = F.shape[1]
    out = torch.empty(M, d, device=F.device, dtype=torch.float32)
    _lib.check(_lib.load().adt_gather_rows(_p(_f32(F)), _ld(F), _p(_i32(rows)), M, _p(m_dev), d, _p(out), d, _stream()), "gather_rows")
    return out


def scatter_rows(G, rows, dF, accumulate, M=None, m_dev=None):
    M = rows.numel() if M is None else M
    _lib.check(_lib.load().adt_scatter_rows(_p(_f32(G)), _ld(G), _p(_i32(rows)), M, _p(m_dev), G.shape[1], _p(dF), _ld(dF), int(accumulate), _stream()),
               "scatter_rows")


def ce_rows(logits, labels, V, inv_count, loss64, M=None, m_dev=None):
    M = logits.shape[0] if M is None else M
    _lib.check(_lib.load().adt_ce_rows(_p(_f32(logits)), _ld(logits), _p(_i32(labels)), M, _p(m_dev), V, _p(inv_count), _p(loss64), _stream()), "ce_rows")


def lce_supported(prec, K):
    return bool(_lib.load().adt_lce_supported(prec, K))


_LCE_WS = {}


def lce_fwd_bwd(h, rows, labels, mcap, m_dev, E, bias, inv_count, loss64, dh, dE, dbias, lse_out=None):
    """Fused all-item logits + cross-entropy on the masked rows (include/adt_hip.h: adt_lce_fwd_bwd).  The workspace is cached per
    (device, mcap, V, K): a captured graph keeps pointing at it."""
    V, K = E.shape
    lib = _lib.load()
    key = (h.device, mcap, V, K, lib.adt_lce_slots(0))
    ws = _LCE_WS.get(key)
    if ws is None:
        ws = _LCE_WS[key] = torch.empty(int(lib.adt_lce_workspace_bytes(mcap, V, K)), device=h.device, dtype=torch.uint8)
    _lib.check(lib.adt_lce_fwd_bwd(_p(_f32(h)), _ld(h), _p(_i32(rows)), _p(_i32(labels)), mcap, _p(m_dev), _p(_f32(E)), _ld(E), _p(bias), V, K,
                                   _p(inv_count), _p(loss64), _p(lse_out), _p(dh), _ld(dh) if dh is not None else 0, _p(dE), _ld(dE), _p(dbias),
                                   _p(ws), ws.numel(), _stream()), "lce_fwd_bwd")


def clip_adam_l2(P, G, M, V, l2, clip, lr, b1, b2, eps, scal, grad_scale=1.0, n=None):
    n = P.numel() if n is None else n
    _lib.check(_lib.load().adt_clip_adam_l2(_p(P), _p(G), _p(M), _p(V), n, float(l2), float(clip), float(lr), float(b1), float(b2), float(eps),
                                            float(grad_scale), _p(scal), _stream()), "clip_adam_l2")


def score_rank_bias(F, ldf, E, bias, cand, B, C, want_rank=True):
    d = E.shape[1]
    logits = torch.empty(B, C, device=E.device, dtype=torch.float32)
    rank = torch.empty(B, device=E.device, dtype=torch.int32) if want_rank else None
    _lib.check(_lib.load().adt_score_rank_bias(_p(F), ldf, _p(E), _p(bias), _p(cand), B, C, d, _p(logits), _p(rank), _stream()), "score_rank_bias")
    return logits, rank


def _stosa_attn_call(mfma, valu, args, prec):
    """adt_<mfma> (matrix cores) when prec is given and that entry point covers the shape (rc != 1), else adt_<valu> (vector ALU, exact)."""
    lib = _lib.load()
    if prec is not None:
        rc = getattr(lib, "adt_" + mfma)(int(prec), *args)
        if rc != 1:
            return _lib.check(rc, mfma)
    _lib.check(getattr(lib, "adt_" + valu)(*args), valu)


def _stosa_attn_fwd(mfma, valu, Qm, Qc, Km, Kc, Vm, Vc, key_ids, B, H, L, p, seed, site, b_offset, prec, scaled=()):
    """scaled: () or (scale, hd_live), the two arguments the *_scaled_* entry points take after hd."""
    d = Qm.shape[1]
    hd = d // H
    Om = torch.empty(B * L, d, device=Qm.device, dtype=torch.float32)
    Oc = torch.empty_like(Om)
    LSE = torch.empty(B * H * L, device=Qm.device, dtype=torch.float32)
    args = [_p(_f32(Qm)), _ld(Qm), _p(_f32(Qc)), _ld(Qc), _p(_f32(Km)), _ld(Km), _p(_f32(Kc)), _ld(Kc), _p(_f32(Vm)), _ld(Vm), _p(_f32(Vc)), _ld(Vc),
            _p(_i32(key_ids)), B, H, L, hd, *scaled, float(p), _p(seed), site, b_offset, _p(Om), d, _p(Oc), d, _p(LSE), _stream()]
    _stosa_attn_call(mfma, valu, args, prec)
    return Om, Oc, LSE


def _stosa_attn_bwd(mfma, valu, Qm, Qc, Km, Kc, Vm, Vc, key_ids, Om, Oc, LSE, dOm, dOc, B, H, L, p, seed, site, b_offset, out, prec, scaled=()):
    d = Qm.shape[1]
    hd = d // H
    outs = [torch.empty(B * L, d, device=Qm.device, dtype=torch.float32) for _ in range(6)] if out is None else list(out)
    ldd = _ld(outs[0])
    assert all(_ld(o) == ldd for o in outs)
    args = [_p(_f32(Qm)), _ld(Qm), _p(_f32(Qc)), _ld(Qc), _p(_f32(Km)), _ld(Km), _p(_f32(Kc)), _ld(Kc), _p(_f32(Vm)), _ld(Vm), _p(_f32(Vc)), _ld(Vc),
            _p(_i32(key_ids)), _p(Om), _ld(Om), _p(Oc), _ld(Oc), _p(LSE), _p(_f32(dOm)), _ld(dOm), _p(_f32(dOc)), _ld(dOc), B, H, L, hd, *scaled, float(p),
            _p(seed), site, b_offset, *[_p(o) for o in outs], ldd, _stream()]
    _stosa_attn_call(mfma, valu, args, prec)
    return outs


def wattn_fwd(Qm, Qc, Km, Kc, Vm, Vc, key_ids, B, H, L, p=0.0, seed=None, site=0, b_offset=0, prec=None):
    """prec: PREC_BF16 / PREC_F32 selects the matrix-core kernels (adt_wattn_mfma.cuh) where they cover the shape; None (or an
    uncovered shape) the exact vector-ALU kernels."""
    return _stosa_attn_fwd("wattn_mfma_fwd", "wattn_fwd", Qm, Qc, Km, Kc, Vm, Vc, key_ids, B, H, L, p, seed, site, b_offset, prec)


def wattn_bwd(Qm, Qc, Km, Kc, Vm, Vc, key_ids, Om, Oc, LSE, dOm, dOc, B, H, L, p=0.0, seed=None, site=0, b_offset=0, out=None, prec=None):
    """out: optional (dQm, dQc, dKm, dKc, dVm, dVc) views sharing one row stride.  prec: as wattn_fwd (use the same value)."""
    return _stosa_attn_bwd("wattn_mfma_bwd", "wattn_bwd", Qm, Qc, Km, Kc, Vm, Vc, key_ids, Om, Oc, LSE, dOm, dOc, B, H, L, p, seed, site, b_offset, out, prec)


def wdist_bpr(Sm, Sc, Em, Ec, pos, neg, pvn_weight, inv_count, dEm, dEc, loss3):
    T, d = Sm.shape
    dSm = torch.empty(T, d, device=Sm.device, dtype=torch.float32)
    dSc = torch.empty_like(dSm)
    _lib.check(_lib.load().adt_wdist_bpr(_p(_f32(Sm)), _p(_f32(Sc)), _ld(Sm), _p(Em), _p(Ec), _p(_i32(pos)), _p(_i32(neg)), T, d, float(pvn_weight),
                                         _p(inv_count), _p(dSm), _p(dSc), d, _p(dEm), _p(dEc), _p(loss3), _stream()), "wdist_bpr")
    return dSm, dSc


def wdist_full(Sm, Sc, Em, Ec, V):
    B, d = Sm.shape
    dist = torch.empty(B, V, device=Sm.device, dtype=torch.float32)
    _lib.check(_lib.load().adt_wdist_full(_p(_f32(Sm)), _p(_f32(Sc)), _ld(Sm), _p(Em), _p(Ec), B, V, d, _p(dist), V, _stream()), "wdist_full")
    return dist


def klattn_fwd(Qm, Qc, Km, Kc, Vm, Vc, key_ids, B, H, L, p=0.0, seed=None, site=0, b_offset=0, prec=None):
    """KL-divergence attention, arguments and outputs as wattn_fwd.  prec: PREC_BF16 / PREC_F32 selects the matrix-core kernels
    (adt_wattn_mfma.cuh with the KL score) where they cover the shape; None (or an uncovered shape) the exact vector-ALU kernels
    (adt_klattn.cuh)."""
    return _stosa_attn_fwd("klattn_mfma_fwd", "klattn_fwd", Qm, Qc, Km, Kc, Vm, Vc, key_ids, B, H, L, p, seed, site, b_offset, prec)


def klattn_bwd(Qm, Qc, Km, Kc, Vm, Vc, key_ids, Om, Oc, LSE, dOm, dOc, B, H, L, p=0.0, seed=None, site=0, b_offset=0, out=None, prec=None):
    """As wattn_bwd: out = optional (dQm, dQc, dKm, dKc, dVm, dVc) views sharing one row stride (overwritten); prec as klattn_fwd
    (use the same value)."""
    return _stosa_attn_bwd("klattn_mfma_bwd", "klattn_bwd", Qm, Qc, Km, Kc, Vm, Vc, key_ids, Om, Oc, LSE, dOm, dOc, B, H, L, p, seed, site, b_offset, out, prec)


def wattn_max_len(hd):
    """The longest sequence at which wattn_* / klattn_* run both directions at head size hd (256 at hd 16 / 32, 141 at hd 64: their LDS
    footprint; 0: a head size they do not take); wattn_long_* / klattn_long_* go on to 1024."""
    n = _lib.load().adt_wattn_max_len(int(hd))
    if n < 0:
        _lib.check(n, "wattn_max_len")
    return n


def _stosa_long_prec(prec):
    return PREC_F32 if prec is None else int(prec)


def _stosa_long_fwd(name, Qm, Qc, Km, Kc, Vm, Vc, key_ids, B, H, L, p, seed, site, b_offset, prec, scaled=()):
    d = Qm.shape[1]
    hd = d // H
    Om = torch.empty(B * L, d, device=Qm.device, dtype=torch.float32)
    Oc = torch.empty_like(Om)
    LSE = torch.empty(B * H * L, device=Qm.device, dtype=torch.float32)
    _lib.check(getattr(_lib.load(), "adt_" + name)(
        _stosa_long_prec(prec), _p(_f32(Qm)), _ld(Qm), _p(_f32(Qc)), _ld(Qc), _p(_f32(Km)), _ld(Km), _p(_f32(Kc)), _ld(Kc), _p(_f32(Vm)), _ld(Vm),
        _p(_f32(Vc)), _ld(Vc), _p(_i32(key_ids)), B, H, L, hd, *scaled, float(p), _p(seed), site, b_offset, _p(Om), d, _p(Oc), d, _p(LSE), _stream()), name)
    return Om, Oc, LSE


def _stosa_long_bwd(name, Qm, Qc, Km, Kc, Vm, Vc, key_ids, Om, Oc, LSE, dOm, dOc, B, H, L, p, seed, site, b_offset, out, prec, scaled=()):
    d = Qm.shape[1]
    hd = d // H
    outs = [torch.empty(B * L, d, device=Qm.device, dtype=torch.float32) for _ in range(6)] if out is None else list(out)
    ldd = _ld(outs[0])
    assert all(_ld(o) == ldd for o in outs)
    _lib.check(getattr(_lib.load(), "adt_" + name)(
        _stosa_long_prec(prec), _p(_f32(Qm)), _ld(Qm), _p(_f32(Qc)), _ld(Qc), _p(_f32(Km)), _ld(Km), _p(_f32(Kc)), _ld(Kc), _p(_f32(Vm)), _ld(Vm),
        _p(_f32(Vc)), _ld(Vc), _p(_i32(key_ids)), _p(Om), _ld(Om), _p(Oc), _ld(Oc), _p(LSE), _p(_f32(dOm)), _ld(dOm), _p(_f32(dOc)), _ld(dOc), B, H, L,
        hd, *scaled, float(p), _p(seed), site, b_offset, *[_p(o) for o in outs], ldd, _stream()), name)
    return outs


def wattn_long_fwd(Qm, Qc, Km, Kc, Vm, Vc, key_ids, B, H, L, p=0.0, seed=None, site=0, b_offset=0, prec=None):
    """wattn_fwd for every 1 <= L <= 1024 on the streamed matrix-core kernels (adt_wattn_long.cuh); same arguments and results.  prec:
    PREC_BF16, or PREC_F32 / None for the exact fp32 MFMA.  A shape they do not take is an error: there is nothing to fall back to."""
    return _stosa_long_fwd("wattn_long_fwd", Qm, Qc, Km, Kc, Vm, Vc, key_ids, B, H, L, p, seed, site, b_offset, prec)


def wattn_long_bwd(Qm, Qc, Km, Kc, Vm, Vc, key_ids, Om, Oc, LSE, dOm, dOc, B, H, L, p=0.0, seed=None, site=0, b_offset=0, out=None, prec=None):
    """wattn_bwd for every 1 <= L <= 1024; LSE (and the contexts) must come from wattn_long_fwd at the same prec."""
    return _stosa_long_bwd("wattn_long_bwd", Qm, Qc, Km, Kc, Vm, Vc, key_ids, Om, Oc, LSE, dOm, dOc, B, H, L, p, seed, site, b_offset, out, prec)


def klattn_long_fwd(Qm, Qc, Km, Kc, Vm, Vc, key_ids, B, H, L, p=0.0, seed=None, site=0, b_offset=0, prec=None):
    """klattn_fwd for every 1 <= L <= 1024; as wattn_long_fwd."""
    return _stosa_long_fwd("klattn_long_fwd", Qm, Qc, Km, Kc, Vm, Vc, key_ids, B, H, L, p, seed, site, b_offset, prec)


def klattn_long_bwd(Qm, Qc, Km, Kc, Vm, Vc, key_ids, Om, Oc, LSE, dOm, dOc, B, H, L, p=0.0, seed=None, site=0, b_offset=0, out=None, prec=None):
    """klattn_bwd for every 1 <= L <= 1024; as wattn_long_bwd."""
    return _stosa_long_bwd("klattn_long_bwd", Qm, Qc, Km, Kc, Vm, Vc, key_ids, Om, Oc, LSE, dOm, dOc, B, H, L, p, seed, site, b_offset, out, prec)


def kldist_bpr(Sm, Sc, Em, Ec, pos, neg, pvn_weight, inv_count, dEm, dEc, loss3):
    """bpr_optimization on row-wise KL divergences; arguments and outputs as wdist_bpr."""
    T, d = Sm.shape
    dSm = torch.empty(T, d, device=Sm.device, dtype=torch.float32)
    dSc = torch.empty_like(dSm)
    _lib.check(_lib.load().adt_kldist_bpr(_p(_f32(Sm)), _p(_f32(Sc)), _ld(Sm), _p(Em), _p(Ec), _p(_i32(pos)), _p(_i32(neg)), T, d, float(pvn_weight),
                                          _p(inv_count), _p(dSm), _p(dSc), d, _p(dEm), _p(dEc), _p(loss3), _stream()), "kldist_bpr")
    return dSm, dSc


def kldist_full(Sm, Sc, Em, Ec, V):
    """kl_predict_full for one eval batch: the B rows of Sm / Sc ARE the batch (the scores depend on B and on each row's place)."""
    B, d = Sm.shape
    dist = torch.empty(B, V, device=Sm.device, dtype=torch.float32)
    _lib.check(_lib.load().adt_kldist_full(_p(_f32(Sm)), _p(_f32(Sc)), _ld(Sm), _p(Em), _p(Ec), B, V, d, _p(dist), V, _stream()), "kldist_full")
    return dist


def topk_masked(dist, k, indptr=None, indices=None, want_val=False):
    """k smallest entries per row in ascending order after pushing the CSR-listed columns to 1e24; `dist` is consumed."""
    B, N = dist.shape
    idx = torch.empty(B, k, device=dist.device, dtype=torch.int32)
    val = torch.empty(B, k, device=dist.device, dtype=torch.float32) if want_val else None
    _lib.check(_lib.load().adt_topk_masked(_p(dist), dist.stride(0), B, N, _p(indptr), _p(indices), k, _p(idx), _p(val), _stream()), "topk_masked")
    return (idx, val) if want_val else idx


def axpy(dst, src, alpha=1.0, accumulate=True, mask_ids=None, d=0):
    """dst = (accumulate ? dst : 0) + alpha * src * rowmask."""
    _lib.check(_lib.load().adt_axpy(_p(dst), _p(_f32(src)), float(alpha), int(accumulate), src.numel(), _p(mask_ids), d, _stream()), "axpy")
    return dst


def _lsm_rows(t, H):
    return t.numel() // H if H > 0 else 0      # H < 1 is the library's to reject (AdtError), not a ZeroDivisionError here


def log_softmax_fwd(X, H):
    Y = torch.empty_like(X)
    _lib.check(_lib.load().adt_log_softmax_fwd(_p(_f32(X)), _lsm_rows(X, H), H, _p(Y), _stream()), "log_softmax_fwd")
    return Y


def log_softmax_bwd(Y, dY, H, dX, accumulate):
    _lib.check(_lib.load().adt_log_softmax_bwd(_p(Y), _p(_f32(dY)), _lsm_rows(Y, H), H, _p(dX), int(accumulate), _stream()), "log_softmax_bwd")


def grad_sumsq(G, out64):
    _lib.check(_lib.load().adt_grad_sumsq(_p(G), G.numel(), _p(out64), _stream()), "grad_sumsq")


def adam_range(P, G, M, V, l2, clip, lr, b1, b2, eps, step, gn2_slots):
    _lib.check(_lib.load().adt_adam_range(_p(P), _p(G), _p(M), _p(V), P.numel(), float(l2), float(clip), float(lr), float(b1), float(b2), float(eps),
                                          float(step), _p(gn2_slots), _stream()), "adam_range")


def adamw_range(P, G, M, V, wd, clip, lr, b1, b2, eps, step, gn2_slots):
    """adam_range with torch.optim.AdamW's decoupled weight decay."""
    _lib.check(_lib.load().adt_adamw_range(_p(P), _p(G), _p(M), _p(V), P.numel(), float(wd), float(clip), float(lr), float(b1), float(b2), float(eps),
                                           float(step), _p(gn2_slots), _stream()), "adamw_range")


def dense_gradsrc(dY, act, U, p=0.0, seed=None, site=0, row_offset=0, mask_ids=None, t_dev=None):
    """G = dY * rowmask * dropmask * act'(U), materialised (see adt_dense_gradsrc)."""
    T, N = dY.shape
    G = torch.empty(T, N, device=dY.device, dtype=torch.float32)
    _lib.check(_lib.load().adt_dense_gradsrc(_p(_f32(dY)), _ld(dY), T, N, _p(mask_ids), float(p), _p(seed), site, row_offset, act, _p(U), _ld(U),
                                             _p(G), N, _p(t_dev), _stream()), "dense_gradsrc")
    return G


def dense_rows_enable(on):
    """bf16 dense layers: True = row-streaming kernels where the shape allows (default), False = always the tiled kernels.
    Returns the previous setting."""
    return bool(_lib.load().adt_dense_rows_enable(int(bool(on))))


# ---- deterministic item-table / positional-table gradient (include/adt_hip.h: adt_item_sort ...) -----------------------------------------
def _ptr_array(tensors, n):
    arr = (ctypes.c_void_p * n)()
    for i in range(n):
        t = tensors[i] if i < len(tensors) else None
        arr[i] = None if t is None else t.data_ptr()
    return arr


def item_sort(ids_list, V1, rows, coef, kind, row_offset=0):
    """Sorts the entries (src, t) of the int32 id tensors in ids_list (same length T each) by item and records the gather plan (rows / coef /
    kind per source: include/adt_hip.h); returns the work buffer for item_segsum."""
    lib = _lib.load()
    nsrc, T = len(ids_list), ids_list[0].numel()
    work = torch.empty(lib.adt_item_sort_work_ints(nsrc, T, V1) + 2, device=ids_list[0].device, dtype=torch.int32)
    kinds = (ctypes.c_int * 4)(*[int(kind[i]) if i < len(kind) else 0 for i in range(4)])
    _lib.check(lib.adt_item_sort(_ptr_array([_i32(t) for t in ids_list], 4), nsrc, T, V1, _ptr_array(rows, 4), _ptr_array(coef, 4), kinds,
                                 row_offset, _p(work), _stream()), "item_sort")
    work._adt_keep = (rows, coef)          # the plan holds their addresses
    return work


def item_segsum(work, nsrc, T, V1, src_mask, site, p, seed, emb_scale, dE, accumulate=False):
    """dE[item] (+)= the sorted entries of `item` from the sources in src_mask (adt_item_segsum)."""
    sites = (ctypes.c_uint32 * 4)(*[int(site[i]) if i < len(site) else 0 for i in range(4)])
    _lib.check(_lib.load().adt_item_segsum(_p(work), nsrc, T, V1, src_mask, sites, float(p), _p(seed), float(emb_scale), _p(_f32(dE)),
                                           int(bool(accumulate)), _stream()), "item_segsum")


def posemb_sum(ids_list, dX_list, sites, B, L, p, seed, row_offset, dP):
    n = len(ids_list)
    s = (ctypes.c_uint32 * 2)(*[int(sites[i]) if i < n else 0 for i in range(2)])
    _lib.check(_lib.load().adt_posemb_sum(_ptr_array([_i32(t) for t in ids_list], 2), _ptr_array(dX_list, 2), s, n, B, L, float(p), _p(seed),
                                          row_offset, _p(_f32(dP)), _stream()), "posemb_sum")


# ---- widths that are not multiples of 64: padded lanes, true-width arithmetic (include/adt_hip.h; adt_amd/wide.py:padded_layout) ---------
def layernorm_lanes_fwd(X, gamma, beta, eps, lanes):
    """LayerNorm over the live lanes of padded rows; lanes = (H, hd, hd_pad), X is (T, H * hd_pad) with zero pad lanes."""
    H, hd, hd_pad = lanes
    T, dp = X.shape
    assert dp == H * hd_pad, (X.shape, lanes)
    Y = torch.empty(T, dp, device=X.device, dtype=torch.float32)
    _lib.check(_lib.load().adt_layernorm_lanes_fwd(_p(_f32(X)), _ld(X), _p(gamma), _p(beta), eps, T, H, hd, hd_pad, _p(Y), dp, _stream()), "ln_lanes_fwd")
    return Y


def layernorm_lanes_bwd(dY, X, gamma, eps, dX, accumulate, dgamma, dbeta, lanes):
    H, hd, hd_pad = lanes
    T, dp = X.shape
    assert dp == H * hd_pad, (X.shape, lanes)
    _lib.check(_lib.load().adt_layernorm_lanes_bwd(_p(_f32(dY)), _ld(dY), _p(_f32(X)), _ld(X), _p(gamma), eps, T, H, hd, hd_pad, _p(dX), _ld(dX),
                                                   int(accumulate), _p(dgamma), _p(dbeta), _stream()), "ln_lanes_bwd")


def drop_lanes(S, lanes, p=0.0, seed=None, site=0, row_offset=0, R=None, R2=None, mask_ids=None, out=None):
    """out = rowmask(R + R2 + dropout(S)) on the live lanes (dropout indexed at the true width), exact zeros on the pad lanes.
    out may be S itself (every element is read and written by the same thread)."""
    H, hd, hd_pad = lanes
    T, dp = S.shape
    assert dp == H * hd_pad, (S.shape, lanes)
    if out is None:
        out = torch.empty(T, dp, device=S.device, dtype=torch.float32)
    _lib.check(_lib.load().adt_drop_lanes(_p(_f32(S)), _ld(S), _p(R), _ld(R), _p(R2), _ld(R2), _p(mask_ids), T, H, hd, hd_pad, float(p), _p(seed), site,
                                          row_offset, _p(_f32(out)), _ld(out), _stream()), "drop_lanes")
    return out


def drn_lanes_fwd(S, R, gamma, beta, eps, lanes, p=0.0, seed=None, site=0, row_offset=0, Z=None, Y=None):
    """Fused drop-residual-normalise on padded rows: Z = R + dropout(S) on the live lanes (dropout indexed at the true width), Y = LayerNorm
    of Z over the live lanes; exact zeros on the pad lanes of both.  Z may be S itself.  Returns (Z, Y)."""
    H, hd, hd_pad = lanes
    T, dp = S.shape
    assert dp == H * hd_pad and R.shape == S.shape, (S.shape, R.shape, lanes)
    if Z is None:
        Z = torch.empty(T, dp, device=S.device, dtype=torch.float32)
    if Y is None:
        Y = torch.empty(T, dp, device=S.device, dtype=torch.float32)
    _lib.check(_lib.load().adt_drn_lanes_fwd(_p(_f32(S)), _ld(S), _p(_f32(R)), _ld(R), _p(gamma), _p(beta), eps, T, H, hd, hd_pad, float(p), _p(seed),
                                             site, row_offset, _p(_f32(Z)), _ld(Z), _p(_f32(Y)), _ld(Y), _stream()), "drn_lanes_fwd")
    return Z, Y


def drn_lanes_bwd(dY, Z, gamma, eps, lanes, p, seed, site, row_offset, dR, accumulate, dS, dgamma, dbeta):
    """Backward of drn_lanes_fwd: dR (+)= dZ, dS = keep / (1 - p) * dZ, dgamma / dbeta += their sums over the rows."""
    H, hd, hd_pad = lanes
    T, dp = Z.shape
    assert dp == H * hd_pad, (Z.shape, lanes)
    _lib.check(_lib.load().adt_drn_lanes_bwd(_p(_f32(dY)), _ld(dY), _p(_f32(Z)), _ld(Z), _p(gamma), eps, T, H, hd, hd_pad, float(p), _p(seed), site,
                                             row_offset, _p(_f32(dR)), _ld(dR), int(accumulate), _p(_f32(dS)), _ld(dS), _p(dgamma), _p(dbeta),
                                             _stream()), "drn_lanes_bwd")


def lane_map(padded, compact, index, scatter):
    """compact[i] = padded[index[i]] (scatter False) or padded[index[i]] = compact[i] (scatter True)."""
    assert padded.dtype == torch.float32 and compact.dtype == torch.float32 and compact.is_contiguous() and compact.numel() == index.numel()
    _lib.check(_lib.load().adt_lane_map(_p(padded), _p(compact), _p(_i32(index)), index.numel(), int(bool(scatter)), _stream()), "lane_map")


# ---- STOSA-ADT at padded widths: lanes = (H, hd, hd_pad), rows of H * hd_pad floats with zero pad lanes ------------
def _lane_chunks(dp, *ts):
    """The (rows, views) one adt_act_lanes_* call covers: tensors of n padded rows side by side are n * T rows when all are contiguous,
    else n column slices of T rows at the tensors' own row strides."""
    T, w = ts[0].shape
    assert w % dp == 0 and all(t.shape == ts[0].shape and t.stride(1) == 1 and t.stride(0) % 4 == 0 for t in ts), ([t.shape for t in ts], dp)
    if all(t.is_contiguous() for t in ts):
        return [(T * (w // dp), ts, (dp,) * len(ts))]
    return [(T, tuple(t[:, k:k + dp] for t in ts), tuple(t.stride(0) for t in ts)) for k in range(0, w, dp)]


def act_lanes_fwd(X, lanes, act, p=0.0, seed=None, site=0, row_offset=0):
    """Y = act(dropout(X)) on the live lanes (dropout indexed at the true width), +0.0 on the pad lanes (adt_act_lanes_fwd).  X may hold
    n padded rows side by side, (T, n * H * hd_pad) -- the q / k / v projections -- when p = 0."""
    H, hd, hd_pad = lanes
    dp = H * hd_pad
    assert X.shape[1] == dp or p == 0.0, (X.shape, lanes, p)
    Y = torch.empty(X.shape, device=X.device, dtype=torch.float32)
    for rows, (x, y), (ldx, ldy) in _lane_chunks(dp, _f32(X), Y):
        _lib.check(_lib.load().adt_act_lanes_fwd(_p(x), ldx, rows, H, hd, hd_pad, float(p), _p(seed), site, row_offset, int(act), _p(y), ldy, _stream()),
                   "act_lanes_fwd")
    return Y


def act_lanes_bwd(dY, X, lanes, act, dX, accumulate, p=0.0, seed=None, site=0, row_offset=0):
    """dX (+)= dY * act'(dropout(X)) * keep / (1 - p) on the live lanes; the pad lanes of dX are written +0.0 (adt_act_lanes_bwd)."""
    H, hd, hd_pad = lanes
    dp = H * hd_pad
    assert X.shape[1] == dp or p == 0.0, (X.shape, lanes, p)
    for rows, (dy, x, dx), (lddy, ldx, lddx) in _lane_chunks(dp, _f32(dY), _f32(X), _f32(dX)):
        _lib.check(_lib.load().adt_act_lanes_bwd(_p(dy), lddy, _p(x), ldx, rows, H, hd, hd_pad, float(p), _p(seed), site, row_offset, int(act), _p(dx),
                                                 lddx, int(accumulate), _stream()), "act_lanes_bwd")


def _scaled(scale, hd_live):
    return (float(scale), int(hd_live))


def wattn_scaled_fwd(Qm, Qc, Km, Kc, Vm, Vc, key_ids, B, H, L, scale, hd_live, p=0.0, seed=None, site=0, b_offset=0, prec=None):
    """wattn_fwd on heads padded from hd_live to Qm.shape[1] / H lanes, with the score scale given (1 / sqrt(true head size))."""
    return _stosa_attn_fwd("wattn_mfma_scaled_fwd", "wattn_scaled_fwd", Qm, Qc, Km, Kc, Vm, Vc, key_ids, B, H, L, p, seed, site, b_offset, prec,
                           _scaled(scale, hd_live))


def wattn_scaled_bwd(Qm, Qc, Km, Kc, Vm, Vc, key_ids, Om, Oc, LSE, dOm, dOc, B, H, L, scale, hd_live, p=0.0, seed=None, site=0, b_offset=0, out=None,
                     prec=None):
    """wattn_bwd for wattn_scaled_fwd (the same scale, hd_live and prec): the pad lanes of all six gradients are +0.0."""
    return _stosa_attn_bwd("wattn_mfma_scaled_bwd", "wattn_scaled_bwd", Qm, Qc, Km, Kc, Vm, Vc, key_ids, Om, Oc, LSE, dOm, dOc, B, H, L, p, seed, site,
                           b_offset, out, prec, _scaled(scale, hd_live))


def wattn_long_scaled_fwd(Qm, Qc, Km, Kc, Vm, Vc, key_ids, B, H, L, scale, hd_live, p=0.0, seed=None, site=0, b_offset=0, prec=None):
    """wattn_long_fwd (1 <= L <= 1024, streamed) with the score scale given and hd_live live lanes per head."""
    return _stosa_long_fwd("wattn_long_scaled_fwd", Qm, Qc, Km, Kc, Vm, Vc, key_ids, B, H, L, p, seed, site, b_offset, prec, _scaled(scale, hd_live))


def wattn_long_scaled_bwd(Qm, Qc, Km, Kc, Vm, Vc, key_ids, Om, Oc, LSE, dOm, dOc, B, H, L, scale, hd_live, p=0.0, seed=None, site=0, b_offset=0,
                          out=None, prec=None):
    return _stosa_long_bwd("wattn_long_scaled_bwd", Qm, Qc, Km, Kc, Vm, Vc, key_ids, Om, Oc, LSE, dOm, dOc, B, H, L, p, seed, site, b_offset, out, prec,
                           _scaled(scale, hd_live))


def wdist_bpr_lanes(Sm, Sc, Em, Ec, pos, neg, pvn_weight, inv_count, dEm, dEc, loss3, lanes):
    """wdist_bpr on padded rows and tables: the pad lanes stay out of the three distances and get +0.0 in dSm / dSc."""
    H, hd, hd_pad = lanes
    T, dp = Sm.shape
    assert dp == H * hd_pad and Em.shape[1] == dp and Ec.shape[1] == dp, (Sm.shape, Em.shape, lanes)
    dSm = torch.empty(T, dp, device=Sm.device, dtype=torch.float32)
    dSc = torch.empty_like(dSm)
    _lib.check(_lib.load().adt_wdist_bpr_lanes(_p(_f32(Sm)), _p(_f32(Sc)), _ld(Sm), _p(Em), _p(Ec), _p(_i32(pos)), _p(_i32(neg)), T, H, hd, hd_pad,
                                               float(pvn_weight), _p(inv_count), _p(dSm), _p(dSc), dp, _p(dEm), _p(dEc), _p(loss3), _stream()),
               "wdist_bpr_lanes")
    return dSm, dSc


def wdist_full_lanes(Sm, Sc, Em, Ec, V, lanes):
    """wdist_full on padded rows and tables: the distance over the live lanes."""
    H, hd, hd_pad = lanes
    B, dp = Sm.shape
    assert dp == H * hd_pad and Em.shape[1] == dp and Ec.shape[1] == dp, (Sm.shape, Em.shape, lanes)
    dist = torch.empty(B, V, device=Sm.device, dtype=torch.float32)
    _lib.check(_lib.load().adt_wdist_full_lanes(_p(_f32(Sm)), _p(_f32(Sc)), _ld(Sm), _p(Em), _p(Ec), B, V, H, hd, hd_pad, _p(dist), V, _stream()),
               "wdist_full_lanes")
    return dist


def wdist_pack_lanes(M, C, elu, nrm_scale, lanes):
    """wdist_pack on padded rows: img (rows, 2 d_pad) with +0.0 on the pad lanes of both halves, nrm over the live lanes."""
    H, hd, hd_pad = lanes
    assert M.dim() == 2 and M.shape == C.shape and M.stride(0) == C.stride(0) and M.shape[1] == H * hd_pad, (M.shape, C.shape, lanes)
    rows, dp = M.shape
    img = torch.empty(rows, 2 * dp, device=M.device, dtype=torch.float32)
    nrm = torch.empty(rows, device=M.device, dtype=torch.float32)
    _lib.check(_lib.load().adt_wdist_pack_lanes(_p(_f32(M)), _p(_f32(C)), M.stride(0), rows, H, hd, hd_pad, int(bool(elu)), _p(img), 2 * dp, _p(nrm),
                                                float(nrm_scale), _stream()), "wdist_pack_lanes")
    return img, nrm


# ---- the same under distance_metric='kl' (DESIGN.md section 27): a pad lane holds cov = 0, which 1 / ck and log c do not take ----------
def klattn_scaled_fwd(Qm, Qc, Km, Kc, Vm, Vc, key_ids, B, H, L, scale, hd_live, p=0.0, seed=None, site=0, b_offset=0, prec=None):
    """klattn_fwd on heads padded from hd_live to Qm.shape[1] / H lanes (mean 0, covariance 0 on the pad lanes), with the score scale given
    (1 / sqrt(true head size)); the matrix-core or the vector-ALU kernels by klattn_fwd's rule."""
    return _stosa_attn_fwd("klattn_mfma_scaled_fwd", "klattn_scaled_fwd", Qm, Qc, Km, Kc, Vm, Vc, key_ids, B, H, L, p, seed, site, b_offset, prec,
                           _scaled(scale, hd_live))


def klattn_scaled_bwd(Qm, Qc, Km, Kc, Vm, Vc, key_ids, Om, Oc, LSE, dOm, dOc, B, H, L, scale, hd_live, p=0.0, seed=None, site=0, b_offset=0, out=None,
                      prec=None):
    """klattn_bwd for klattn_scaled_fwd (the same scale, hd_live and prec): the pad lanes of all six gradients are +0.0."""
    return _stosa_attn_bwd("klattn_mfma_scaled_bwd", "klattn_scaled_bwd", Qm, Qc, Km, Kc, Vm, Vc, key_ids, Om, Oc, LSE, dOm, dOc, B, H, L, p, seed, site,
                           b_offset, out, prec, _scaled(scale, hd_live))


def klattn_long_scaled_fwd(Qm, Qc, Km, Kc, Vm, Vc, key_ids, B, H, L, scale, hd_live, p=0.0, seed=None, site=0, b_offset=0, prec=None):
    """klattn_long_fwd (1 <= L <= 1024, streamed) with the score scale given and hd_live live lanes per head."""
    return _stosa_long_fwd("klattn_long_scaled_fwd", Qm, Qc, Km, Kc, Vm, Vc, key_ids, B, H, L, p, seed, site, b_offset, prec, _scaled(scale, hd_live))


def klattn_long_scaled_bwd(Qm, Qc, Km, Kc, Vm, Vc, key_ids, Om, Oc, LSE, dOm, dOc, B, H, L, scale, hd_live, p=0.0, seed=None, site=0, b_offset=0,
                           out=None, prec=None):
    return _stosa_long_bwd("klattn_long_scaled_bwd", Qm, Qc, Km, Kc, Vm, Vc, key_ids, Om, Oc, LSE, dOm, dOc, B, H, L, p, seed, site, b_offset, out, prec,
                           _scaled(scale, hd_live))


# ---- the distance attention at head size 128: every 1 <= L <= 1024, scale and hd_live always given ---------------
def wattn_hd128_fwd(Qm, Qc, Km, Kc, Vm, Vc, key_ids, B, H, L, scale, hd_live, p=0.0, seed=None, site=0, b_offset=0, prec=None):
    """wattn_long_scaled_fwd at head size Qm.shape[1] / H = 128 (adt_wattn_hd128.hip); an unpadded head passes 1 / sqrt(128) and 128.
    Any other head size is an error."""
    return _stosa_long_fwd("wattn_hd128_fwd", Qm, Qc, Km, Kc, Vm, Vc, key_ids, B, H, L, p, seed, site, b_offset, prec, _scaled(scale, hd_live))


def wattn_hd128_bwd(Qm, Qc, Km, Kc, Vm, Vc, key_ids, Om, Oc, LSE, dOm, dOc, B, H, L, scale, hd_live, p=0.0, seed=None, site=0, b_offset=0, out=None,
                    prec=None):
    """wattn_long_scaled_bwd at head size 128, for wattn_hd128_fwd (the same scale, hd_live and prec)."""
    return _stosa_long_bwd("wattn_hd128_bwd", Qm, Qc, Km, Kc, Vm, Vc, key_ids, Om, Oc, LSE, dOm, dOc, B, H, L, p, seed, site, b_offset, out, prec,
                           _scaled(scale, hd_live))


def klattn_hd128_fwd(Qm, Qc, Km, Kc, Vm, Vc, key_ids, B, H, L, scale, hd_live, p=0.0, seed=None, site=0, b_offset=0, prec=None):
    """klattn_long_scaled_fwd at head size 128; hd_live = 128 runs the unpadded KL kernel, fewer the lane-aware one."""
    return _stosa_long_fwd("klattn_hd128_fwd", Qm, Qc, Km, Kc, Vm, Vc, key_ids, B, H, L, p, seed, site, b_offset, prec, _scaled(scale, hd_live))


def klattn_hd128_bwd(Qm, Qc, Km, Kc, Vm, Vc, key_ids, Om, Oc, LSE, dOm, dOc, B, H, L, scale, hd_live, p=0.0, seed=None, site=0, b_offset=0, out=None,
                     prec=None):
    """klattn_long_scaled_bwd at head size 128, for klattn_hd128_fwd (the same scale, hd_live and prec)."""
    return _stosa_long_bwd("klattn_hd128_bwd", Qm, Qc, Km, Kc, Vm, Vc, key_ids, Om, Oc, LSE, dOm, dOc, B, H, L, p, seed, site, b_offset, out, prec,
                           _scaled(scale, hd_live))


def kldist_bpr_lanes(Sm, Sc, Em, Ec, pos, neg, pvn_weight, inv_count, dEm, dEc, loss3, lanes):
    """kldist_bpr on padded rows and tables: the pad lanes stay out of every sum and log, the divergences subtract the true d, dSm / dSc
    get +0.0 there."""
    H, hd, hd_pad = lanes
    T, dp = Sm.shape
    assert dp == H * hd_pad and Em.shape[1] == dp and Ec.shape[1] == dp, (Sm.shape, Em.shape, lanes)
    dSm = torch.empty(T, dp, device=Sm.device, dtype=torch.float32)
    dSc = torch.empty_like(dSm)
    _lib.check(_lib.load().adt_kldist_bpr_lanes(_p(_f32(Sm)), _p(_f32(Sc)), _ld(Sm), _p(Em), _p(Ec), _p(_i32(pos)), _p(_i32(neg)), T, H, hd, hd_pad,
                                                float(pvn_weight), _p(inv_count), _p(dSm), _p(dSc), dp, _p(dEm), _p(dEc), _p(loss3), _stream()),
               "kldist_bpr_lanes")
    return dSm, dSc


def kldist_full_lanes(Sm, Sc, Em, Ec, V, lanes):
    """kldist_full on padded rows and tables (the B rows are the eval batch): the score over the live lanes, with the true d."""
    H, hd, hd_pad = lanes
    B, dp = Sm.shape
    assert dp == H * hd_pad and Em.shape[1] == dp and Ec.shape[1] == dp, (Sm.shape, Em.shape, lanes)
    dist = torch.empty(B, V, device=Sm.device, dtype=torch.float32)
    _lib.check(_lib.load().adt_kldist_full_lanes(_p(_f32(Sm)), _p(_f32(Sc)), _ld(Sm), _p(Em), _p(Ec), B, V, H, hd, hd_pad, _p(dist), V, _stream()),
               "kldist_full_lanes")
    return dist


def klrow_pack_lanes(M, C, items, lanes):
    """klrow_pack on padded rows: img (rows, 2 d_pad) with +0.0 on the pad lanes of both halves, off over the live lanes with the true d."""
    H, hd, hd_pad = lanes
    assert M.dim() == 2 and M.shape == C.shape and M.stride(0) == C.stride(0) and M.shape[1] == H * hd_pad, (M.shape, C.shape, lanes)
    rows, dp = M.shape
    img = torch.empty(rows, 2 * dp, device=M.device, dtype=torch.float32)
    off = torch.empty(rows, device=M.device, dtype=torch.float32)
    _lib.check(_lib.load().adt_klrow_pack_lanes(_p(_f32(M)), _p(_f32(C)), M.stride(0), rows, H, hd, hd_pad, int(bool(items)), _p(img), 2 * dp, _p(off),
                                                _stream()), "klrow_pack_lanes")
    return img, off


# ---- full-catalogue ranking (include/adt_hip.h: adt_full_rank; adt_amd/csrc/adt_fullrank.cuh) ---------------------------------------------
def seen_csr_host(seen, rows):
    """The seen items of `rows` users as int32 CSR (indptr (rows + 1,), indices) numpy arrays.  `seen`: a scipy sparse matrix (its stored
    entries are the seen items), a dense (rows, n) 0/1 array, an (indptr, indices) pair, or None -> (None, None); also (None, None) when nothing is stored."""
    import numpy as np
    if seen is None:
        return None, None
    if isinstance(seen, tuple):
        ip, ix = seen
    elif hasattr(seen, "tocsr"):
        csr = seen.tocsr()
        ip, ix = csr.indptr, csr.indices
    else:
        r, cols = np.nonzero(np.asarray(seen))
        ip = np.zeros(rows + 1, np.int64)
        np.cumsum(np.bincount(r, minlength=rows), out=ip[1:])
        ix = cols
    if len(ip) < rows + 1:
        raise ValueError("seen has %d rows, the batch %d" % (len(ip) - 1, rows))
    if len(ix) == 0:
        return None, None
    return np.ascontiguousarray(ip, dtype=np.int32), np.ascontiguousarray(ix, dtype=np.int32)


def seen_csr(seen, rows, device):
    """seen_csr_host on the device: (indptr, indices) int32 tensors, or (None, None)."""
    ip, ix = seen_csr_host(seen, rows)
    if ip is None:
        return None, None
    return torch.from_numpy(ip).to(device), torch.from_numpy(ix).to(device)


def full_rank(F, ldf, E, n_items, target=None, bias=None, indptr=None, indices=None, k=0, splits=0, first_id=1):
    """Exact fp32 scores F[b] . E[j] (+ bias[j]) of every eligible item 1 <= j <= n_items not in the user's CSR seen list, never
    materialised: returns (rank (B,) int32 of target[b] among the eligible items, -1 without a target; n_elig (B,) int32 eligible items
    other than the target; top_idx (B, k) int32 and top_val (B, k) of the k best, score descending, ties to the smaller id, -1 / -inf
    tail; both None when k = 0).  F: B rows of width E.shape[1] at row stride ldf (any view whose first element is row 0).
    first_id = 0 (adt_full_rank_from) lets item 0 compete as well: ranked, counted, selected, excluded where the seen list names it."""
    # F is either the (B, d) view itself or a longer buffer whose rows sit ldf apart: then the targets / the CSR give the batch
    if F.dim() == 2 and F.stride(0) == ldf:
        B = F.shape[0]
    elif target is not None:
        B = target.numel()
    elif indptr is not None:
        B = indptr.numel() - 1
    else:
        raise _lib.AdtError("full_rank: the batch size is unknown: pass F as the (B, d) view with row stride ldf, or a target / indptr")
    if bias is not None and (bias.dtype != torch.float32 or not bias.is_contiguous() or bias.numel() < n_items + 1):
        raise _lib.AdtError("full_rank: bias must be contiguous fp32 with at least n_items + 1 = %d entries" % (n_items + 1))
    if E.shape[0] < n_items + 1:
        raise _lib.AdtError("full_rank: the item table has %d rows, n_items + 1 = %d are read" % (E.shape[0], n_items + 1))
    d, lde = E.shape[1], E.stride(0)
    dev = E.device
    lib = _lib.load()
    ws = torch.empty(max(int(lib.adt_full_rank_ws_bytes(B, int(n_items), int(k), int(splits))), 16), device=dev, dtype=torch.uint8)
    rank = torch.empty(B, device=dev, dtype=torch.int32)
    n_elig = torch.empty(B, device=dev, dtype=torch.int32)
    top_idx = torch.empty(B, k, device=dev, dtype=torch.int32) if k > 0 else None
    top_val = torch.empty(B, k, device=dev, dtype=torch.float32) if k > 0 else None
    _lib.check(lib.adt_full_rank_from(_p(_f32(F)), int(ldf), _p(_f32(E)), lde, _p(bias), B, d, int(n_items), int(first_id),
                                      _p(None if target is None else _i32(target)), _p(None if indptr is None else _i32(indptr)),
                                      _p(None if indices is None else _i32(indices)), int(k), int(splits), _p(ws), ws.numel(), _p(rank),
                                      _p(n_elig), _p(top_idx), _p(top_val), _stream()), "full_rank")
    return rank, n_elig, top_idx, top_val


def full_rank_groups(F, ldf, E, n_items, target, seen_off, seen_items, n_rows, rows_per_group, row0=0, bias=None, k=0, splits=0, first_id=1):
    """full_rank for P stacked candidates of the same users (adt_full_rank_groups): n_rows = P * rows_per_group feature rows (F: any view
    whose first element is row 0, row stride ldf), group-major -- row r is user u = r % rows_per_group, whose target is target[row0 + u]
    and whose seen list is row row0 + u of the RESIDENT CSR seen_off (int64, one entry more than the rows) / seen_items (int32), e.g.
    DeviceEvalData's, taken as it is: a batch is named by row0.  target None ranks nothing (top-k only); seen_off and seen_items both None
    means nothing seen.  Returns full_rank's (rank, n_elig, top_idx, top_val), each with n_rows rows."""
    n_rows, rpg, row0 = int(n_rows), int(rows_per_group), int(row0)
    if target is not None and (target.dtype != torch.int32 or not target.is_contiguous()):
        raise _lib.AdtError("full_rank_groups: target must be a contiguous int32 tensor")
    if (seen_off is None) != (seen_items is None):
        raise _lib.AdtError("full_rank_groups: seen_off and seen_items go together")
    if seen_off is not None and (seen_off.dtype != torch.int64 or not seen_off.is_contiguous() or seen_items.dtype != torch.int32 or not seen_items.is_contiguous()):
        raise _lib.AdtError("full_rank_groups: seen_off must be contiguous int64 and seen_items contiguous int32")
    # the rows the resident lists cover: what the kernel may index with row0 + u
    n_total = seen_off.numel() - 1 if seen_off is not None else (target.numel() if target is not None else row0 + max(rpg, 0))
    if target is not None and target.numel() < n_total:
        raise _lib.AdtError("full_rank_groups: %d targets for the %d rows of seen_off" % (target.numel(), n_total))
    if rpg < 1 or n_rows % rpg != 0:
        raise _lib.AdtError("full_rank_groups: %d rows, rows_per_group=%d" % (n_rows, rpg))
    if bias is not None and (bias.dtype != torch.float32 or not bias.is_contiguous() or bias.numel() < n_items + 1):
        raise _lib.AdtError("full_rank_groups: bias must be contiguous fp32 with at least n_items + 1 = %d entries" % (n_items + 1))
    if E.shape[0] < n_items + 1:
        raise _lib.AdtError("full_rank_groups: the item table has %d rows, n_items + 1 = %d are read" % (E.shape[0], n_items + 1))
    d, lde = E.shape[1], E.stride(0)
    dev = E.device
    lib = _lib.load()
    ws = torch.empty(max(int(lib.adt_full_rank_ws_bytes(n_rows, int(n_items), int(k), int(splits))), 16), device=dev, dtype=torch.uint8)
    rank = torch.empty(n_rows, device=dev, dtype=torch.int32)
    n_elig = torch.empty(n_rows, device=dev, dtype=torch.int32)
    top_idx = torch.empty(n_rows, k, device=dev, dtype=torch.int32) if k > 0 else None
    top_val = torch.empty(n_rows, k, device=dev, dtype=torch.float32) if k > 0 else None
    _lib.check(lib.adt_full_rank_groups(_p(_f32(F)), int(ldf), _p(_f32(E)), lde, _p(bias), n_rows, rpg, d, int(n_items), int(first_id), _p(target),
                                        _p(seen_off), _p(seen_items), int(n_total), row0, int(k), int(splits), _p(ws), ws.numel(), _p(rank),
                                        _p(n_elig), _p(top_idx), _p(top_val), _stream()), "full_rank_groups")
    return rank, n_elig, top_idx, top_val


FULLSTATS_MAX_KH = 1024


def full_rank_stats(rank, n_elig, rows_per_group, kh, hist=None, auc=None):
    """The additive statistics of full-catalogue ranks, counted on the device (adt_full_rank_stats): rank / n_elig (N,) int32 as
    full_rank / full_rank_groups return them, group-major.  For every row of group g with rank >= 0: hist[g][min(rank, kh)] += 1 and
    auc[g] += (n_elig - rank) / max(n_elig, 1).  Returns (hist (groups, kh + 1) int64, auc (groups,) float64): new zeros where an
    output is None, otherwise the tensor given, accumulated into.  The float64 sum has a fixed order: two runs give the same bits."""
    if rank.dtype != torch.int32 or n_elig.dtype != torch.int32 or not rank.is_contiguous() or not n_elig.is_contiguous() or rank.numel() != n_elig.numel():
        raise _lib.AdtError("full_rank_stats: rank and n_elig must be contiguous int32 tensors of one length")
    N, rpg, kh = rank.numel(), int(rows_per_group), int(kh)
    if rpg < 1 or N % rpg != 0:
        raise _lib.AdtError("full_rank_stats: %d rows, rows_per_group=%d" % (N, rpg))
    if not 1 <= kh <= FULLSTATS_MAX_KH:
        raise _lib.AdtError("full_rank_stats: kh=%d outside 1..%d" % (kh, FULLSTATS_MAX_KH))
    groups = N // rpg
    if hist is None:
        hist = torch.zeros(groups, kh + 1, device=rank.device, dtype=torch.int64)
    elif hist.dtype != torch.int64 or not hist.is_contiguous() or hist.numel() != groups * (kh + 1):
        raise _lib.AdtError("full_rank_stats: hist must be contiguous int64 with %d x %d entries" % (groups, kh + 1))
    if auc is None:
        auc = torch.zeros(groups, device=rank.device, dtype=torch.float64)
    elif auc.dtype != torch.float64 or not auc.is_contiguous() or auc.numel() != groups:
        raise _lib.AdtError("full_rank_stats: auc must be contiguous float64 with %d entries" % groups)
    if N > 0:      # an empty tensor has no address to hand over
        _lib.check(_lib.load().adt_full_rank_stats(_p(rank), _p(n_elig), N, rpg, kh, _p(hist), _p(auc), _stream()), "full_rank_stats")
    return hist, auc


def wdist_pack(M, C, elu, nrm_scale):
    """Row images for Wasserstein full-catalogue ranking (adt_wdist_pack): img (rows, 2d) = [M | sqrt(max(c, 1e-24))] and
    nrm (rows,) = nrm_scale * (sum M^2 + sum c), c = ELU(C) + 1 when elu else C.  Items: (True, -0.5) -> (W, bias) of full_rank; user
    states: (False, 1.0) -> (A, na), with dist[b][j] = na[b] - 2 * (A[b] . W[j] + bias[j])."""
    assert M.dim() == 2 and M.shape == C.shape and M.stride(0) == C.stride(0), (M.shape, C.shape, M.stride(), C.stride())
    rows, d = M.shape
    img = torch.empty(rows, 2 * d, device=M.device, dtype=torch.float32)
    nrm = torch.empty(rows, device=M.device, dtype=torch.float32)
    _lib.check(_lib.load().adt_wdist_pack(_p(_f32(M)), _p(_f32(C)), M.stride(0), rows, d, int(bool(elu)), _p(img), 2 * d, _p(nrm), float(nrm_scale),
                                          _stream()), "wdist_pack")
    return img, nrm


def kldist_pack(Em, Ec):
    """The item image of the grouped KL full sort (adt_kldist_pack): img (V, 2d) = [Em | 1 / ci], lv (V,) = sum_c log ci, ci = ELU(Ec) + 1."""
    assert Em.dim() == 2 and Em.shape == Ec.shape and Em.stride(0) == Ec.stride(0), (Em.shape, Ec.shape, Em.stride(), Ec.stride())
    V, d = Em.shape
    img = torch.empty(V, 2 * d, device=Em.device, dtype=torch.float32)
    lv = torch.empty(V, device=Em.device, dtype=torch.float32)
    _lib.check(_lib.load().adt_kldist_pack(_p(_f32(Em)), _p(_f32(Ec)), Em.stride(0), V, d, _p(img), 2 * d, _p(lv), _stream()), "kldist_pack")
    return img, lv


def klrow_pack(M, C, items):
    """Row images for full-catalogue ranking by the row-wise KL divergence (adt_klrow_pack), KL[u][v] = nu[u] - (A[u] . W[v] + bias[v]).
    Items (items=True): c = ELU(C) + 1, img (rows, 2d) = [-0.5 / c | M / c], off (rows,) = -0.5 (sum log c + sum M^2 / c) -> (W, bias) of
    full_rank; user states (items=False): c = C, img = [M^2 + c | M], off = -0.5 (d + sum log c) -> (A, nu)."""
    assert M.dim() == 2 and M.shape == C.shape and M.stride(0) == C.stride(0), (M.shape, C.shape, M.stride(), C.stride())
    rows, d = M.shape
    img = torch.empty(rows, 2 * d, device=M.device, dtype=torch.float32)
    off = torch.empty(rows, device=M.device, dtype=torch.float32)
    _lib.check(_lib.load().adt_klrow_pack(_p(_f32(M)), _p(_f32(C)), M.stride(0), rows, d, int(bool(items)), _p(img), 2 * d, _p(off), _stream()),
               "klrow_pack")
    return img, off


def kldist_full_groups(Sm, Sc, img, lv, E, V):
    """kl_predict_full for the P = rows / E stacked eval batches of E users each (candidate-major rows of Sm / Sc) against the packed
    items (kldist_pack): dist (rows, V).  The reference's chunking by E pairs the rows of one group only; rows == E is kldist_full to
    fp32 rounding."""
    assert Sm.dim() == 2 and Sm.shape == Sc.shape and Sm.stride(0) == Sc.stride(0), (Sm.shape, Sc.shape, Sm.stride(), Sc.stride())
    rows, d = Sm.shape
    assert img.shape[1] == 2 * d and img.shape[0] >= V and lv.numel() >= V, (img.shape, lv.shape, V, d)
    dist = torch.empty(rows, V, device=Sm.device, dtype=torch.float32)
    _lib.check(_lib.load().adt_kldist_full_groups(_p(_f32(Sm)), _p(_f32(Sc)), Sm.stride(0), _p(_f32(img)), img.stride(0), _p(_f32(lv)), rows, int(E),
                                                  int(V), d, _p(dist), V, _stream()), "kldist_full_groups")
    return dist


def kldist_pack_lanes(Em, Ec, lanes):
    """kldist_pack on padded tables (adt_kldist_pack_lanes): img (V, 2 d_pad) with +0.0 on the pad lanes of both halves, lv over the live
    lanes; no pad lane reaches a log or a divide."""
    H, hd, hd_pad = lanes
    assert Em.dim() == 2 and Em.shape == Ec.shape and Em.stride(0) == Ec.stride(0), (Em.shape, Ec.shape, Em.stride(), Ec.stride())
    V, dp = Em.shape
    img = torch.empty(V, 2 * dp, device=Em.device, dtype=torch.float32)
    lv = torch.empty(V, device=Em.device, dtype=torch.float32)
    _lib.check(_lib.load().adt_kldist_pack_lanes(_p(_f32(Em)), _p(_f32(Ec)), Em.stride(0), V, dp, H, hd, hd_pad, _p(img), 2 * dp, _p(lv), _stream()),
               "kldist_pack_lanes")
    return img, lv


def kldist_full_groups_lanes(Sm, Sc, img, lv, E, V, lanes):
    """kldist_full_groups on padded state rows and the image of kldist_pack_lanes: the score over the live lanes, with the true d."""
    H, hd, hd_pad = lanes
    assert Sm.dim() == 2 and Sm.shape == Sc.shape and Sm.stride(0) == Sc.stride(0), (Sm.shape, Sc.shape, Sm.stride(), Sc.stride())
    rows, dp = Sm.shape
    assert img.shape[1] == 2 * dp and img.shape[0] >= V and lv.numel() >= V, (img.shape, lv.shape, V, dp)
    dist = torch.empty(rows, V, device=Sm.device, dtype=torch.float32)
    _lib.check(_lib.load().adt_kldist_full_groups_lanes(_p(_f32(Sm)), _p(_f32(Sc)), Sm.stride(0), _p(_f32(img)), img.stride(0), _p(_f32(lv)), rows,
                                                        int(E), int(V), dp, H, hd, hd_pad, _p(dist), V, _stream()), "kldist_full_groups_lanes")
    return dist


# ---- STOSA-ADT batches built on the device (include/adt_hip.h: adt_seqbatch_build; adt_amd/csrc/adt_seqbatch.cuh) -----------------------
def seqbatch_build(seq_off, seq_items, set_off, set_items, users, L, cut, item_size, seed=0, step=0, rows=None, want_neg=True,
                   want_inv_count=True, views=True):
    """Rows rows=(lo, hi) (default: all) of the batch `users` (device int32, the GLOBAL batch, ids inside the CSRs) as (hi - lo, L) int32
    device tensors (inp, dec, pos, neg, inv_count): the train (cut 3) / valid (2) / test (1) view of every sequence, negatives outside
    the user's set drawn from (seed, step, global row, position), inv_count = 1 / max(non-zero pos entries of ALL users, 1).  neg /
    inv_count are None when not wanted; views=False also leaves dec and pos out (evaluation reads inp alone)."""
    for off, items in ((seq_off, seq_items), (set_off, set_items)):
        assert off.dtype == torch.int64 and off.is_contiguous() and off.numel() >= 2, (off.dtype, off.shape)
        _i32(items)
    n_users = users.numel()
    lo, hi = (0, n_users) if rows is None else (int(rows[0]), int(rows[1]))
    if not 0 <= lo <= hi <= n_users:
        raise _lib.AdtError("seqbatch_build: rows (%d, %d) outside the batch of %d users" % (lo, hi, n_users))
    dev = users.device
    inp, dec, pos, neg = (torch.empty(hi - lo, int(L), device=dev, dtype=torch.int32) if want else None
                          for want in (True, views, views, want_neg))
    inv_count = torch.empty(1, device=dev, dtype=torch.float32) if want_inv_count else None
    _lib.check(_lib.load().adt_seqbatch_build(_p(seq_off), _p(seq_items), _p(set_off), _p(set_items), _p(_i32(users)), n_users, lo, hi - lo,
                                              int(L), int(cut), int(item_size), int(seed) & 0xFFFFFFFF, int(step) & 0xFFFFFFFF, _p(inp), _p(dec),
                                              _p(pos), _p(neg), _p(inv_count), _stream()), "seqbatch_build")
    return inp, dec, pos, neg, inv_count


def seqbatch_draw(seed, step, row, t, attempt, item_size):
    """The id in [1, item_size - 1] that attempt `attempt` proposes as the negative of position t of GLOBAL batch row `row` (host only:
    the inline function adt_seqbatch_build's kernel calls)."""
    return int(_lib.load().adt_seqbatch_draw(int(seed) & 0xFFFFFFFF, int(step) & 0xFFFFFFFF, int(row), int(t), int(attempt), int(item_size)))


# ---- BERT4Rec-ADT batches masked and built on the device (include/adt_hip.h: adt_bertbatch_*; adt_amd/csrc/adt_bertbatch.cuh) -----------
def bertbatch_threshold(mask_prob):
    """thr_mask of adt_bertbatch_build: a position is masked iff a 32-bit hash is below min(floor(mask_prob * 2^32), 2^32 - 1)."""
    p = float(mask_prob)
    if not 0.0 <= p < 1.0:
        raise _lib.AdtError("bertbatch: mask_prob = %r, need 0 <= mask_prob < 1" % (mask_prob,))
    return min(int(p * 4294967296.0), 0xFFFFFFFF)


def bertbatch_build(seq_off, seq_items, win_start, win_len, examples, L, dupe, itemnum, thr_mask, seed=0, salt=0, rows=None, want_labels=True):
    """Rows rows=(lo, hi) (default: all) of the batch `examples` (device int32, the GLOBAL batch of example ids: e < W * dupe is random copy
    e % dupe of window e // dupe, W * dupe + u the mask-last example of user u) as device tensors (src, dec, labels, rows, labels_c, M,
    inv_count): src / dec / labels (hi - lo, L) int32 (labels None when not wanted), rows / labels_c ((hi - lo) * L,) the ascending flat
    indices of the non-zero labels and those labels, zero beyond M (int32 (1,)), inv_count (1,) = 1 / max(labels of ALL examples, 1).  The
    masks are a function of (seed, salt, example id, window position) alone.  Example ids are the caller's to check (an id outside the
    table gives an all-padding row)."""
    assert seq_off.dtype == torch.int64 and seq_off.is_contiguous() and seq_off.numel() >= 1, (seq_off.dtype, seq_off.shape)
    assert win_start.dtype == torch.int64 and win_start.is_contiguous() and win_start.numel() == win_len.numel(), (win_start.dtype, win_start.shape)
    _i32(seq_items), _i32(win_len)
    n = examples.numel()
    lo, hi = (0, n) if rows is None else (int(rows[0]), int(rows[1]))
    if not 0 <= lo <= hi <= n:
        raise _lib.AdtError("bertbatch_build: rows (%d, %d) outside the batch of %d examples" % (lo, hi, n))
    dev, L = examples.device, int(L)
    src, dec, labels = (torch.empty(hi - lo, max(L, 0), device=dev, dtype=torch.int32) if want else None for want in (True, True, want_labels))
    rows_c, labels_c = (torch.empty((hi - lo) * max(L, 0), device=dev, dtype=torch.int32) for _ in range(2))
    M = torch.empty(1, device=dev, dtype=torch.int32)
    inv_count = torch.empty(1, device=dev, dtype=torch.float32)
    work = torch.empty(n + 1, device=dev, dtype=torch.int32)
    _lib.check(_lib.load().adt_bertbatch_build(_p(seq_off), _p(seq_items), _p(win_start), _p(win_len), _p(_i32(examples)), n, lo, hi - lo, L,
                                               win_start.numel(), int(dupe), seq_off.numel() - 1, int(itemnum), int(seed) & 0xFFFFFFFF,
                                               int(salt) & 0xFFFFFFFF, int(thr_mask) & 0xFFFFFFFF, _p(src), _p(dec), _p(labels), _p(rows_c),
                                               _p(labels_c), _p(M), _p(inv_count), _p(work), _stream()), "bertbatch_build")
    return src, dec, labels, rows_c, labels_c, M, inv_count


def bertbatch_eval(seq_off, seq_items, users, L, itemnum):
    """(len(users), L) int32: the last L - 1 training items of every user (device int32 indices into the CSR) followed by [MASK] =
    itemnum + 1, left-padded (BertEvalDataset.sequence)."""
    assert seq_off.dtype == torch.int64 and seq_off.is_contiguous() and seq_off.numel() >= 1, (seq_off.dtype, seq_off.shape)
    _i32(seq_items)
    n, L = users.numel(), int(L)
    seq = torch.empty(n, max(L, 0), device=users.device, dtype=torch.int32)
    _lib.check(_lib.load().adt_bertbatch_eval(_p(seq_off), _p(seq_items), _p(_i32(users)), n, seq_off.numel() - 1, L, int(itemnum), _p(seq),
                                              _stream()), "bertbatch_eval")
    return seq


def bertbatch_token(seed, salt, example, pos, thr_mask, itemnum, item):
    """(token, masked) at window position `pos` of random example `example` whose item is `item` (host only: the inline function
    adt_bertbatch_build's kernel calls)."""
    masked = ctypes.c_int(0)
    tok = _lib.load().adt_bertbatch_token(int(seed) & 0xFFFFFFFF, int(salt) & 0xFFFFFFFF, int(example), int(pos), int(thr_mask) & 0xFFFFFFFF,
                                          int(itemnum), int(item), ctypes.byref(masked))
    return int(tok), bool(masked.value)


# ---- STOSA-ADT full-sort scores on the device (include/adt_hip.h: adt_hit_hist; adt_amd/csrc/adt_hithist.cuh) ---------------------------
def hit_hist(top_idx, answers, rows_per_group=None, hist=None, want_pos=False):
    """Histogram of where each held-out item stands in its top-K list: top_idx (N, K) device int32 at any row stride (adt_full_rank_from /
    adt_topk_masked output, -1 tails included), group-major -- row r belongs to group r // rows_per_group and its answer is
    answers[r % rows_per_group]; answers a device int32 (rows_per_group,) or (rows_per_group, 1) (rows_per_group defaults to its
    length).  Position = the first j with top_idx[r][j] == answer, K when there is none.  Returns hist (groups, K + 1) int64: new zeros
    when `hist` is None, otherwise `hist` itself, accumulated into; with want_pos also the (N,) int32 positions."""
    if top_idx.dim() != 2 or top_idx.dtype != torch.int32 or (top_idx.shape[1] > 1 and top_idx.stride(1) != 1):
        raise _lib.AdtError("hit_hist: top_idx must be (N, K) int32 with unit column stride")
    N, K = top_idx.shape
    ans = answers.reshape(-1)
    if ans.dtype != torch.int32 or not ans.is_contiguous():
        raise _lib.AdtError("hit_hist: answers must be a contiguous int32 (rows_per_group,) or (rows_per_group, 1) tensor")
    rpg = ans.numel() if rows_per_group is None else int(rows_per_group)
    if rpg < 1 or ans.numel() != rpg or N % rpg != 0:
        raise _lib.AdtError("hit_hist: %d list rows, %d answers, rows_per_group=%d" % (N, ans.numel(), rpg))
    groups = N // rpg
    if hist is None:
        hist = torch.zeros(groups, K + 1, device=top_idx.device, dtype=torch.int64)
    elif hist.dtype != torch.int64 or not hist.is_contiguous() or (N > 0 and hist.numel() != groups * (K + 1)):
        raise _lib.AdtError("hit_hist: hist must be contiguous int64 with %d x %d entries" % (groups, K + 1))
    pos = torch.empty(N, device=top_idx.device, dtype=torch.int32) if want_pos else None
    ld = top_idx.stride(0) if N > 1 else max(top_idx.stride(0), K)
    _lib.check(_lib.load().adt_hit_hist(_p(top_idx), int(ld), N, K, _p(ans), rpg, _p(hist), _p(pos), _stream()), "hit_hist")
    return (hist, pos) if want_pos else hist


# ---- SASRec-ADT sampled evaluation on the device (include/adt_hip.h: adt_evalcand_*, adt_cand_rank_hist; adt_evalcand.cuh, adt_candrank.cuh)
EVALCAND_MAX_DRAWS, EVALCAND_MAX_S = 4096, 1024


def evalcand_stream(cum, seed, salt, row, n0, n):
    """Stream values n0 .. n0 + n - 1 of GLOBAL row `row` as a numpy int32 array (host only: the inline function adt_evalcand_draw's kernel
    calls).  cum: HOST int64 prefix sums of the item counts, cum[0] = 0, total = cum[-1] < 2^32."""
    import numpy as np
    cum = np.ascontiguousarray(cum, dtype=np.int64)
    out = np.empty(max(int(n), 0), np.int32)
    _lib.check(_lib.load().adt_evalcand_stream(cum.ctypes.data, cum.size - 1, int(seed) & 0xFFFFFFFF, int(salt) & 0xFFFFFFFF, int(row), int(n0), int(n),
                                               out.ctypes.data), "evalcand_stream")
    return out


def evalcand_draw(cum, total, seen_off, seen_items, targets, S, seed=0, salt=0, rows=None, out=None, want_filled=False):
    """Rows rows=(lo, hi) (default: all) of the candidate table of the evaluation user list: (hi - lo, 1 + S) int32, column 0 =
    targets[row], columns 1..S the first S distinct values outside the row's sorted seen ids (CSR seen_off int64 / seen_items int32, over
    the GLOBAL rows) of the popularity stream of (seed, salt, GLOBAL row).  cum: device int64 prefix sums, total = its last entry (the
    caller's host copy: nothing is read back).  out: an int32 (hi - lo, >= 1 + S) view to write into (row stride free, unit column
    stride), default a new tensor.  With want_filled also the (hi - lo,) int32 count of properly filled slots (S unless a user has
    fewer than S drawable ids: the open slots hold id 0)."""
    assert cum.dtype == torch.int64 and cum.is_contiguous() and seen_off.dtype == torch.int64 and seen_off.is_contiguous(), (cum.dtype, seen_off.dtype)
    _i32(seen_items), _i32(targets)
    n_total, S = targets.numel(), int(S)
    if seen_off.numel() != n_total + 1:
        raise _lib.AdtError("evalcand_draw: %d targets, seen_off has %d entries" % (n_total, seen_off.numel()))
    lo, hi = (0, n_total) if rows is None else (int(rows[0]), int(rows[1]))
    if not 0 <= lo <= hi <= n_total:
        raise _lib.AdtError("evalcand_draw: rows (%d, %d) outside the list of %d users" % (lo, hi, n_total))
    if out is None:
        out = torch.empty(hi - lo, 1 + max(S, 0), device=targets.device, dtype=torch.int32)
    elif out.dtype != torch.int32 or out.dim() != 2 or out.shape[0] != hi - lo or out.shape[1] < 1 + S or (out.shape[1] > 1 and out.stride(1) != 1):
        raise _lib.AdtError("evalcand_draw: out must be an int32 (%d, >= %d) view with unit column stride" % (hi - lo, 1 + S))
    filled = torch.empty(hi - lo, device=targets.device, dtype=torch.int32) if want_filled else None
    ldc = out.stride(0) if hi - lo > 1 else max(out.stride(0), out.shape[1])
    _lib.check(_lib.load().adt_evalcand_draw(_p(cum), cum.numel() - 1, int(total), _p(seen_off), _p(seen_items), _p(targets), n_total, lo, hi - lo, S,
                                             int(seed) & 0xFFFFFFFF, int(salt) & 0xFFFFFFFF, _p(out), int(ldc), _p(filled), _stream()), "evalcand_draw")
    return (out, filled) if want_filled else out


def cand_rank_hist(F, ldf, E, cand, n_rows, rows_per_group=None, hist=None, bias=None, want_rank=False):
    """score_rank's scores and ranks without the logit matrix, counted on the device: n_rows feature rows (F: any view whose first
    element is row 0, row stride ldf), group-major -- row r is scored against candidate row r % rows_per_group of cand (rows_per_group, C)
    int32, column 0 the held-out item -- and hist[r // rows_per_group][rank] += 1.  Returns hist (groups, C) int64: new zeros when `hist`
    is None, otherwise `hist` itself, accumulated into; with want_rank also the (n_rows,) int32 ranks."""
    if cand.dim() != 2 or cand.dtype != torch.int32 or not cand.is_contiguous():
        raise _lib.AdtError("cand_rank_hist: cand must be a contiguous (rows_per_group, C) int32 tensor")
    rpg = cand.shape[0] if rows_per_group is None else int(rows_per_group)
    C, n_rows = cand.shape[1], int(n_rows)
    if rpg < 1 or cand.shape[0] != rpg or n_rows % rpg != 0:
        raise _lib.AdtError("cand_rank_hist: %d rows, %d candidate rows, rows_per_group=%d" % (n_rows, cand.shape[0], rpg))
    if not E.is_contiguous() or (bias is not None and (bias.dtype != torch.float32 or not bias.is_contiguous())):
        raise _lib.AdtError("cand_rank_hist: E and bias must be contiguous fp32")
    groups = n_rows // rpg
    if hist is None:
        hist = torch.zeros(groups, C, device=E.device, dtype=torch.int64)
    elif hist.dtype != torch.int64 or not hist.is_contiguous() or hist.numel() != groups * C:
        raise _lib.AdtError("cand_rank_hist: hist must be contiguous int64 with %d x %d entries" % (groups, C))
    rank = torch.empty(n_rows, device=E.device, dtype=torch.int32) if want_rank else None
    _lib.check(_lib.load().adt_cand_rank_hist(_p(_f32(F)), int(ldf), _p(_f32(E)), _p(bias), _p(cand), n_rows, rpg, C, E.shape[1], _p(hist), _p(rank),
                                              _stream()), "cand_rank_hist")
    return (hist, rank) if want_rank else hist
