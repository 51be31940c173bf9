"""GPU: every resident and chunked instantiation of the general masked attention (adt_amd/csrc/adt_attn_gen.cuh; adt_attn_masked_fwd / _bwd and
the _scaled_ pair) called directly, over the case table of tests/attn_cases.py.  tests/test_attn_cases_cpu.py proves on the CPU that the table
reaches each instantiation key (direction, prec, hd, family, MAXKT, NCH, CSK) below under every mask mode that can reach it -- causal with
fill -inf (the model code's call), key padding and both with fill -1e9 (a left-padded and a fully padded sequence), at hd 128 also causal
with fill -1e9 (tile skip on) and -1e4 (off) -- and with dropout off and on (nonzero b_offset):

  k_attn_gen_fwd<prec, hd, 4 | 8 | 14>, k_attn_gen_bwd<prec, hd, 4 | 8 | 14>        hd 16, 32, 64; fp32 and bf16; L 1..64 | 65..128 | 129..224
  k_attn_gen_bwd_chunked<F32, 64, 16, 2>                                             in place of k_attn_gen_bwd<F32, 64, 14>
  k_attn_gen_fwd<prec, 128, 4, CSK 0 | 1>, k_attn_gen_bwd_chunked<prec, 128, 4, 1>   fp32 and bf16, L 1..64
  k_attn_gen_fwd<BF16, 128, 16, CSK 0 | 1>, k_attn_gen_bwd_chunked<BF16, 128, 16, 2> bf16 only, L 65..256 (fp32 streams there: test_attn_hd256_hip.py)

Tolerances.  (a) the project's own (test_wide_kernels.py, test_attn_hd256_hip.py), relative to the reference tensor's maximum: exact fp32
3e-5 forward and gradients; bf16 operands 2e-2 forward, 6e-2 gradients; the gradients' denominator is at least max |dV| (dQ = dK = 0 at L = 1).
LSE: 1e-4 absolute in fp32; in bf16 1e-4 plus the score error of operands rounded to 8 bits, (2^-7 + 2^-16) scale max_j sum_i |q_i| |k_ji| per
query (each operand off by at most 2^-8 of itself; a log-sum-exp moves by at most the largest score error).  (b), (c) none: bit for bit.
(d) 2^-8 of the sum of the absolute terms, derived in that test's docstring.  The reference is attn_cases.ref64: attn_oracle of
test_attn_hd256_hip.py in float64 with the score scale (test_attn_cases_cpu.py holds it against the float32 tape oracle itself)."""
import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import attn_cases as ac  # noqa: E402

DEV = "cuda:0"
TOL_FWD = {ac.F32: 3e-5, ac.BF16: 2e-2}
TOL_BWD = {ac.F32: 3e-5, ac.BF16: 6e-2}
LSE_ABS = 1e-4


def T_(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def rel(a, b, floor=1e-6):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), floor)


def run(prec, qkv, dO, nB, H, L, mask, ids, fill, p, b_off, scale=None, out=None):
    """Forward and backward on column views of the packed (T, 3 d) projection, as the models call them.  qkv, dO, ids: device tensors.
    Returns (O, LSE, dQ, dK, dV)."""
    from adt_amd import ops
    d = qkv.shape[1] // 3
    q, k, v = qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:]
    causal = ac.flags(mask)[0]
    sd = torch.tensor([ac.SEED], device=DEV, dtype=torch.int32)
    O, LSE = ops.attn_masked_fwd(prec, q, k, v, nB, H, L, causal, ids, fill, p, sd, ac.SITE, b_off, scale=scale)
    dQ, dK, dV = ops.attn_masked_bwd(prec, q, k, v, O, LSE, dO, nB, H, L, causal, ids, fill, p, sd, ac.SITE, b_off, out=out, scale=scale)
    return O, LSE, dQ, dK, dV


def same(a, b):
    return torch.equal(a, b)      # bit for bit up to the sign of a zero; NaN never equal


# ---- (a) parity with float64 over the whole table -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ac.CASES, ids=ac.case_id)
def test_parity_with_float64(case):
    prec, H, hd, L, mask, fill, p, scale = case
    qkv, dO, ids, valid = ac.make_inputs(case)
    ref = ac.reference(case)
    d, t = H * hd, ac.true_hd(hd, scale)
    kid = None if ids is None else T_(ids.reshape(-1))
    got = [x.cpu().numpy() for x in run(prec, T_(qkv), T_(dO), ac.B, H, L, mask, kid, fill, p, ac.B_OFF, scale)]
    O, LSE, dQ, dK, dV = got
    assert all(np.isfinite(x).all() for x in got)
    if t < hd:      # zero lanes in, zero lanes out: exactly
        for x in (O, dQ, dK, dV):
            assert not x.reshape(-1, H, hd)[:, :, t:].any()
        O, dQ, dK, dV = (ac.true_lanes(x, H, hd, t) for x in (O, dQ, dK, dV))
    floor = np.abs(ref["dv"]).max()
    errs = dict(O=rel(O, ref["o"]), dQ=rel(dQ, ref["dq"], floor), dK=rel(dK, ref["dk"], floor), dV=rel(dV, ref["dv"]))
    lse_err = np.abs(LSE.reshape(ac.B, H, L) - ref["lse"])
    lse_tol = LSE_ABS + ((2.0 ** -7 + 2.0 ** -16) * ref["qk"] if prec == ac.BF16 else 0.0)
    print("%s: %s lse %.3g (tol %.3g)" % (ac.case_id(case), " ".join("%s %.3g" % kv for kv in errs.items()), lse_err.max(), np.max(lse_tol)))
    assert errs["O"] < TOL_FWD[prec]
    assert errs["dQ"] < TOL_BWD[prec] and errs["dK"] < TOL_BWD[prec] and errs["dV"] < TOL_BWD[prec]
    assert np.all(lse_err <= lse_tol)
    if mask != "causal":      # the fully padded sequence: uniform attention, LSE = log L
        assert np.abs(LSE.reshape(ac.B, H, L)[2] - math.log(L)).max() <= LSE_ABS


def test_scaled_entry_points_reject_a_nonpositive_scale():
    from adt_amd import _lib, ops
    g = torch.zeros(16, 3 * 64, device=DEV)
    q, k, v = g[:, :64], g[:, 64:128], g[:, 128:]
    for scale in (0.0, -0.2):
        with pytest.raises(_lib.AdtError, match="must be positive"):
            ops.attn_masked_fwd(0, q, k, v, 1, 2, 16, True, None, float("-inf"), scale=scale)
        with pytest.raises(_lib.AdtError, match="must be positive"):
            ops.attn_masked_bwd(0, q, k, v, q, torch.zeros(32, device=DEV), q, 1, 2, 16, True, None, float("-inf"), scale=scale)


@pytest.mark.parametrize("hd,L,text", [(64, 225, "L=225 > 224 unsupported"), (128, 257, "L=257 > 256 unsupported at head_dim 128")])
def test_lengths_past_the_maximum_raise_the_plans_error(hd, L, text):
    from adt_amd import _lib, ops
    g = torch.zeros(L, 3 * hd, device=DEV)
    q, k, v = g[:, :hd], g[:, hd:2 * hd], g[:, 2 * hd:]
    for prec in (0, 1):
        with pytest.raises(_lib.AdtError, match=text):
            ops.attn_masked_fwd(prec, q, k, v, 1, 1, L, True, None, float("-inf"))
        with pytest.raises(_lib.AdtError, match=text):
            ops.attn_masked_bwd(prec, q, k, v, q, torch.zeros(L, device=DEV), q, 1, 1, L, True, None, float("-inf"))


# ---- (b) strided outputs ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", [ac.F32, ac.BF16])
def test_backward_into_strided_views(prec):
    """out= of ops.attn_masked_bwd: three column views of one (B L, 3 d + 4) buffer (the packed gradient of the in-projection).  The views equal
    the contiguous result bit for bit and the four spare columns keep their sentinel.  (ops.attn_masked_fwd allocates its own O: no forward twin.)"""
    case = (prec, 2, 128, 200, "both", -1e9, 0.2, None)
    H, hd, L, mask, fill, p = case[1:7]
    d = H * hd
    qkv, dO, ids, _ = ac.make_inputs(case)
    g, gdO, kid = T_(qkv), T_(dO), T_(ids.reshape(-1))
    want = run(prec, g, gdO, ac.B, H, L, mask, kid, fill, p, ac.B_OFF)
    buf = torch.full((ac.B * L, 3 * d + 4), -7.25, device=DEV)
    views = (buf[:, :d], buf[:, d:2 * d], buf[:, 2 * d:3 * d])
    got = run(prec, g, gdO, ac.B, H, L, mask, kid, fill, p, ac.B_OFF, out=views)
    assert all(a.data_ptr() == b.data_ptr() for a, b in zip(got[2:], views))
    for name, a, b in zip(("dQ", "dK", "dV"), views, want[2:]):
        assert same(a, b), name
    assert bool((buf[:, 3 * d:] == -7.25).all())
    assert float(want[2].abs().max()) > 0 and float(want[4].abs().max()) > 0


# ---- (c) mask leaks, bit for bit --------------------------------------------------------------------------------------------------------------------
def leak_inputs(prec, H, hd, L):
    r = np.random.RandomState(31 * hd + L + prec)
    d = H * hd
    qkv = r.standard_normal((ac.B * L, 3 * d)).astype(np.float32)
    dO = r.standard_normal((ac.B * L, d)).astype(np.float32)
    loud_qkv = (10.0 * r.standard_normal((ac.B * L, 3 * d))).astype(np.float32)      # fresh values of ten times the magnitude
    loud_dO = (10.0 * r.standard_normal((ac.B * L, d))).astype(np.float32)
    return r, qkv, dO, loud_qkv, loud_dO


def leak_id(c):
    return "%s-hd%d-L%d" % ("bf16" if c[0] else "f32", c[2], c[3])


@pytest.mark.parametrize("case", ac.LEAK_CASES, ids=leak_id)
def test_causal_mask_leaks_nothing(case):
    """Rows >= t of Q, K, V and dO of every sequence replaced: O, LSE and dQ of the rows before t do not change in any bit (masked scores are
    replaced by the fill before the maximum, dS is zeroed under the mask, exp(-inf - lse) = 0).  t: 1, the last tile boundary, and an odd row
    inside the last, half-empty tile pair.  fill -inf, no key ids: the model code's call (CSK on at hd 128)."""
    prec, H, hd, L = case
    _, qkv, dO, loud_qkv, loud_dO = leak_inputs(prec, H, hd, L)
    base = run(prec, T_(qkv), T_(dO), ac.B, H, L, "causal", None, ac.NINF, 0.2, ac.B_OFF)
    last = 16 * ((L - 1) // 16)
    assert 1 < last < last + 3 < L and (last // 16) % 2 == 0
    row = np.arange(ac.B * L) % L
    for t in (1, last, last + 3):
        x, g = qkv.copy(), dO.copy()
        x[row >= t], g[row >= t] = loud_qkv[row >= t], loud_dO[row >= t]
        got = run(prec, T_(x), T_(g), ac.B, H, L, "causal", None, ac.NINF, 0.2, ac.B_OFF)
        before = T_(row < t)
        before_lse = T_(np.arange(ac.B * H * L) % L < t)
        assert same(got[0][before], base[0][before]), ("O", t)
        assert same(got[1][before_lse], base[1][before_lse]), ("LSE", t)
        assert same(got[2][before], base[2][before]), ("dQ", t)
        assert not same(got[0], base[0]) and bool(torch.isfinite(got[2]).all())


@pytest.mark.parametrize("mask", ["keypad", "both"])
@pytest.mark.parametrize("case", ac.LEAK_CASES, ids=leak_id)
def test_padded_keys_leak_nothing(case, mask):
    """K and V rows at padded keys replaced (every sequence keeps a valid key and no query loses all of its keys: right padding under the causal
    mask, scattered padding without it): O, LSE, dQ of every row and dK, dV at valid keys do not change in any bit; dK and dV at padded keys are
    exactly 0 in both runs (exp(-1e9 - lse) = 0)."""
    prec, H, hd, L = case
    r, qkv, dO, loud_qkv, _ = leak_inputs(prec, H, hd, L)
    d = H * hd
    ids = r.randint(1, 50, size=(ac.B, L)).astype(np.int32)
    if mask == "both":
        for b, n in enumerate((L // 3, 1, L - 1)):      # right padding: n padded keys at the end
            ids[b, L - n:] = 0
    else:
        ids[r.rand(ac.B, L) < 0.3] = 0
        ids[0, 0], ids[1, :17], ids[2, 5] = 0, 0, 7      # a padded first key, a padded first tile, and a valid key in any case
    pad = (ids == 0).reshape(-1)
    assert pad.any() and (ids > 0).any(1).all()
    x = qkv.copy()
    x[pad, d:] = loud_qkv[pad, d:]
    kid, gdO = T_(ids.reshape(-1)), T_(dO)
    base = run(prec, T_(qkv), gdO, ac.B, H, L, mask, kid, -1e9, 0.2, ac.B_OFF)
    got = run(prec, T_(x), gdO, ac.B, H, L, mask, kid, -1e9, 0.2, ac.B_OFF)
    for name, a, b in zip(("O", "LSE", "dQ"), got[:3], base[:3]):
        assert same(a, b), name
    tpad = T_(pad)
    for name, a, b in zip(("dK", "dV"), got[3:], base[3:]):
        assert same(a[~tpad], b[~tpad]), name
        assert not bool(a[tpad].any()) and not bool(b[tpad].any()), name
        assert bool(b[~tpad].any())


@pytest.mark.parametrize("mask", ["causal", "keypad"])
@pytest.mark.parametrize("case", ac.LEAK_CASES, ids=leak_id)
def test_sequences_are_independent(case, mask):
    """Sequence b of a B = 3 call against a B = 1 call on that sequence's rows with b_offset + b: every output bit for bit."""
    prec, H, hd, L = case
    r, qkv, dO, _, _ = leak_inputs(prec, H, hd, L)
    ids, fill = (None, ac.NINF) if mask == "causal" else (ac.key_ids(r, L, mask)[0], -1e9)
    g, gdO = T_(qkv), T_(dO)
    kid = None if ids is None else T_(ids.reshape(-1))
    full = run(prec, g, gdO, ac.B, H, L, mask, kid, fill, 0.2, ac.B_OFF)
    for b in range(ac.B):
        rows = slice(b * L, (b + 1) * L)
        one = run(prec, g[rows], gdO[rows], 1, H, L, mask, None if kid is None else kid[rows], fill, 0.2, ac.B_OFF + b)
        for name, a, w in zip(("O", "LSE", "dQ", "dK", "dV"), one, full):
            assert same(a, w[b * H * L:(b + 1) * H * L] if name == "LSE" else w[rows]), (name, b)


# ---- (d) a sharp bf16 bound where bf16 is the only precision -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,mask,fill,p", ac.SHARP_CASES, ids=lambda v: "%g" % v if isinstance(v, float) else str(v))
def test_bf16_only_kernels_to_the_rounding_of_the_probabilities(L, mask, fill, p):
    """k_attn_gen_fwd<BF16, 128, 16, CSK 0 | 1> and k_attn_gen_bwd_chunked<BF16, 128, 16, 2> have no fp32 twin, and 2e-2 of the tensor maximum
    cannot see one mis-masked key among two hundred.  Here every operand is exact, so the bound is the rounding of the probabilities alone.

    Q, K, V, dO are multiples of 1/8 in [-2, 2] and the scale is 2^-3 (the scaled entry point).  Then Q * scale (k / 64, |k| <= 16) and K, V, dO
    (k / 8, |k| <= 16) have five significant bits and are exact in bf16; a score is a sum of 128 multiples of 1/512, each at most 1/2 in
    magnitude, exact in the fp32 accumulator.  What is rounded to bf16 are the probabilities the second matrix product reads: exp(s - m), times
    1 / (1 - p) if kept, in the forward, and exp(s - lse) likewise for dV.  bf16 keeps 8 significant bits and the conversion rounds to nearest
    even (v_cvt_pk_bf16_f32), so a probability is off by at most half a unit in the last place: 2^-9 of the power of two below it, which is
    2^-9 of the value at best and 2^-8 / (1 + 2^-8) of it at worst (a value just above a power of two).  O = sum_j w_j v_j and
    dV = sum_q w_q dO_q are sums of such terms, W the dropped and rescaled probabilities, so |O - o| <= 2^-8 (1 - 2^-8 + 2^-16) (W |V|) plus
    what fp32 adds, relative to the same sum of absolute terms: __expf (the argument's product with log2 e is rounded: |s - m| 2^-24, below
    2^-17.5 for any argument whose exponential is not zero), for dV the saved LSE and __logf (2^-19), the fp32 accumulation of at most 8 matrix
    products and the row sum (2^-20), the one division (2^-24).  Those add up to less than the 2^-16 that the worst case of the rounding
    leaves free, so the bound asserted -- 2^-8 (W |V|), and 2^-8 (W^T |dO|) for dV, element by element -- holds for a correct kernel: with a
    factor 2 over the typical rounding and next to none over the worst (elements with one dominant term reach 0.97 of it).  One key among two
    hundred attended or dropped by mistake moves O by about 1/200 of W |V|, above 2^-8; under the project's tolerance it would have to reach
    2e-2 of max |O|.  dQ and dK (dS is rounded too, with cancellation) stay at the project's 6e-2."""
    H, hd = 2, 128
    d = H * hd
    r = np.random.RandomState(5 * L + len(mask))
    qkv = (r.randint(-16, 17, size=(ac.B * L, 3 * d)) / 8.0).astype(np.float32)
    dO = (r.randint(-16, 17, size=(ac.B * L, d)) / 8.0).astype(np.float32)
    if mask == "causal":
        ids, valid = None, np.ones((ac.B, L), bool)
    else:      # sequence 0 left-padded, sequence 2 with holes
        ids = r.randint(1, 50, size=(ac.B, L)).astype(np.int32)
        ids[0, : L // 3] = 0
        ids[2, r.rand(L) < 0.3] = 0
        valid = ids > 0
    scale = 2.0 ** -3
    ref = ac.ref64(qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:], dO, ac.B, H, L, valid, ac.flags(mask)[0], fill, p, ac.SEED, ac.SITE, ac.B_OFF, scale)

    def heads(x):
        return np.abs(np.asarray(x, np.float64)).reshape(ac.B, L, H, hd).transpose(0, 2, 1, 3)

    def rows(x):
        return x.transpose(0, 2, 1, 3).reshape(ac.B * L, d)
    bound_o = 2.0 ** -8 * rows(ref["w"] @ heads(qkv[:, 2 * d:]))
    bound_dv = 2.0 ** -8 * rows(ref["w"].transpose(0, 1, 3, 2) @ heads(dO))
    kid = None if ids is None else T_(ids.reshape(-1))
    O, LSE, dQ, dK, dV = (x.cpu().numpy() for x in run(ac.BF16, T_(qkv), T_(dO), ac.B, H, L, mask, kid, fill, p, ac.B_OFF, scale))
    err_o, err_dv = np.abs(O - ref["o"]), np.abs(dV - ref["dv"])
    with np.errstate(divide="ignore", invalid="ignore"):
        print("L %d %s %g p %g: O %.3g, dV %.3g of the bound; LSE %.3g" % (L, mask, fill, p, np.nanmax(err_o / bound_o), np.nanmax(err_dv / bound_dv),
                                                                          np.abs(LSE.reshape(ac.B, H, L) - ref["lse"]).max()))
    assert np.all(err_o <= bound_o)
    assert np.all(err_dv <= bound_dv)
    assert np.abs(LSE.reshape(ac.B, H, L) - ref["lse"]).max() <= LSE_ABS      # exact scores: the fp32 bound holds
    floor = np.abs(ref["dv"]).max()
    assert rel(dQ, ref["dq"], floor) < TOL_BWD[ac.BF16] and rel(dK, ref["dk"], floor) < TOL_BWD[ac.BF16]
