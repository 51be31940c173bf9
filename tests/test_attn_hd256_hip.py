"""GPU check of the general masked attention at head size 256 (adt_amd/csrc/adt_attn_long.cuh at 256 rows: key / query chunks streamed through
LDS, online softmax in the forward; also head size 128 in the exact-fp32 mode at L > 64, which runs there) against the float64 restatement of tests/test_wide_kernels.py::test_masked_attention, with that
test's tolerances: causal only (fill -inf, the SASRec mask), key padding only and both (fill -1e9, BERT's: a fully padded sequence
attends uniformly), dropout off and on with a nonzero b_offset, both precisions, L from 1 to 256."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import tape as tp  # noqa: E402

TOL = {0: 3e-5, 1: 2e-2}      # exact fp32 / bf16 operands (test_wide_kernels.py)


def T_(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def rel(a, b, floor=1e-6):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), floor)


def attn_oracle(q, k, v, B, H, L, key_valid, causal, fill, p, seed, site, b_off, dO):
    """test_wide_kernels.attn_oracle."""
    d = q.shape[1]
    hd = d // H
    vq, vk, vv = tp.leaf(q), tp.leaf(k), tp.leaf(v)

    def split(x):
        return tp.transpose(tp.reshape(x, (B, L, H, hd)), (0, 2, 1, 3))
    s = tp.div_const(tp.matmul(split(vq), tp.transpose(split(vk), (0, 1, 3, 2))), np.sqrt(hd))
    mask = np.broadcast_to(~key_valid[:, None, None, :], s.shape).copy()
    if causal:
        mask |= np.triu(np.ones((L, L), bool), 1)[None, None]
    s = tp.masked_fill(s, mask, fill)
    w = tp.dropout(tp.softmax(s), p, seed, site, tp.idx_attn(B, H, L, b_off))
    o = tp.reshape(tp.transpose(tp.matmul(w, split(vv)), (0, 2, 1, 3)), (B * L, d))
    tp.backward(o, dO)
    return o.v, vq.g, vk.g, vv.g


@pytest.mark.parametrize("prec", [0, 1])
@pytest.mark.parametrize("p", [0.0, 0.2])
@pytest.mark.parametrize("mask", ["causal", "keypad", "both"])
@pytest.mark.parametrize("L", [1, 16, 50, 64, 65, 128, 200, 256])
def test_masked_attention_hd256(L, mask, p, prec):
    check_attention(256, 1, L, mask, p, prec)


@pytest.mark.parametrize("p", [0.0, 0.2])
@pytest.mark.parametrize("mask", ["causal", "keypad", "both"])
@pytest.mark.parametrize("L", [65, 200, 256])
def test_masked_attention_hd128_fp32_long(L, mask, p):
    check_attention(128, 2, L, mask, p, 0)


def check_attention(hd, H, L, mask, p, prec):
    from adt_amd import ops
    B = 3
    d = H * hd
    r = np.random.RandomState(7 * L + {"causal": 0, "keypad": 1, "both": 2}[mask])
    qkv = r.standard_normal((B * L, 3 * d)).astype(np.float32)
    dO = r.standard_normal((B * L, d)).astype(np.float32)
    causal = mask != "keypad"
    if mask == "causal":
        ids, fill = None, float("-inf")
        valid = np.ones((B, L), bool)
    else:
        ids = r.randint(1, 50, size=(B, L)).astype(np.int32)
        ids[0, : L // 3] = 0      # left padding
        ids[2, :] = 0             # a fully padded sequence: uniform attention over all L keys (finite fill)
        fill = -1e9
        valid = ids > 0
    seed, site, b_off = 99, 17, 5
    q, k, v = qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:]
    o, dq, dk, dv = attn_oracle(q, k, v, B, H, L, valid, causal, fill, p, seed, site, b_off, dO)
    g = T_(qkv)
    sd = torch.tensor([seed], device="cuda:0", dtype=torch.int32)
    kid = None if ids is None else T_(ids.reshape(-1))
    O, LSE = ops.attn_masked_fwd(prec, g[:, :d], g[:, d:2 * d], g[:, 2 * d:], B, H, L, causal, kid, fill, p, sd, site, b_off)
    assert rel(O.cpu().numpy(), o) < TOL[prec]
    dQ, dK, dV = ops.attn_masked_bwd(prec, g[:, :d], g[:, d:2 * d], g[:, 2 * d:], O, LSE, T_(dO), B, H, L, causal, kid, fill, p, sd, site, b_off)
    tol = TOL[prec] * (3 if prec else 1)
    # dQ and dK vanish identically at L = 1 (softmax over one key): all three gradients are measured against dV's magnitude at least
    floor = np.abs(dv).max()
    assert rel(dQ.cpu().numpy(), dq, floor) < tol
    assert rel(dK.cpu().numpy(), dk, floor) < tol
    assert rel(dV.cpu().numpy(), dv) < tol


def test_hd256_bounds():
    from adt_amd import _lib, ops
    g = torch.zeros(257, 3 * 256, device="cuda:0")
    with pytest.raises(_lib.AdtError, match="outside 1..256"):
        ops.attn_masked_fwd(0, g[:, :256], g[:, 256:512], g[:, 512:], 1, 1, 257, True, None, float("-inf"))
