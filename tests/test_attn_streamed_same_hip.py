"""GPU: the two instantiations of the streamed masked attention (adt_amd/csrc/adt_attn_long.cuh) are the same function.  adt_attn_masked_*
launches it with 256 rows of per-sequence state (head size 256, and head size 128 in the exact-fp32 mode at L > 64), adt_attn_long_* with
1024; nothing else differs, so on identical tensors O, LSE, dQ, dK and dV must agree bit for bit.  L 256 is the last row of the 256-row
state, 17 and 65 leave ragged tiles and chunks, 200 is the template length.  Sequence 0 is left-padded for L // 3 rows (dead causal prefix
queries: the first-attendable-key rule), sequence 1 is fully padded; at L 1 that is no padding and a single padded key."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SHAPES = [(256, 1, prec, L) for prec in (0, 1) for L in (1, 17, 65, 200, 256)] + [(128, 2, 0, L) for L in (65, 256)]


@pytest.mark.parametrize("p", [0.0, 0.2])
@pytest.mark.parametrize("mask", ["causal", "keypad", "both"])
@pytest.mark.parametrize("hd,H,prec,L", SHAPES)
def test_masked_and_long_agree_bitwise(hd, H, prec, L, mask, p):
    from adt_amd import ops
    B, d = 2, H * hd
    r = np.random.RandomState(11 * L + hd + {"causal": 0, "keypad": 1, "both": 2}[mask])
    g = torch.from_numpy(r.standard_normal((B * L, 3 * d)).astype(np.float32)).to("cuda:0")
    dO = torch.from_numpy(r.standard_normal((B * L, d)).astype(np.float32)).to("cuda:0")
    causal = mask != "keypad"
    if mask == "causal":
        kid, fill = None, float("-inf")      # the causal skip is on
    else:
        ids = r.randint(1, 50, size=(B, L)).astype(np.int32)
        ids[0, : L // 3] = 0
        ids[1, :] = 0
        kid, fill = torch.from_numpy(ids.reshape(-1)).to("cuda:0"), -1e9
    sd = torch.tensor([99], device="cuda:0", dtype=torch.int32)
    q, k, v = g[:, :d], g[:, d:2 * d], g[:, 2 * d:]
    mask_args = (B, H, L, causal, kid, fill, p, sd, 17, 5 if p else 0)
    got = {}
    for name, fwd, bwd in (("masked", ops.attn_masked_fwd, ops.attn_masked_bwd), ("long", ops.attn_long_fwd, ops.attn_long_bwd)):
        O, LSE = fwd(prec, q, k, v, *mask_args)
        got[name] = (O, LSE) + tuple(bwd(prec, q, k, v, O, LSE, dO, *mask_args))
    for what, a, b in zip(("O", "LSE", "dQ", "dK", "dV"), got["masked"], got["long"]):
        assert torch.equal(a, b), "%s: %d elements differ, max |diff| %g" % (what, int((a != b).sum()), float((a - b).abs().max()))
