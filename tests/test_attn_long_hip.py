"""GPU: the masked attention for 1 <= L <= 1024 (adt_amd/csrc/adt_attn_long.cuh; adt_attn_long_fwd / _bwd) called directly, at every head
size in both precisions:

  k_attn_long_fwd<prec, hd, 4, 32 | 64>, k_attn_long_bwd<prec, hd, 4, 32>        hd 16, 32, 64, 128, 256; fp32 and bf16

Inputs, masks and the float64 reference are those of tests/attn_cases.py (B = 3; with key ids sequence 0 is left-padded by a third and
sequence 2 fully padded).  Lengths: 37 and 200 (the resident kernels run there too), 225 and 257 (the first past each of their bounds and past
their 256-row arrays), 300, 513 and 1009 (L % 4 != 0, a partial last tile, one row past a chunk boundary), 1024 (every array full).  The five
mask modes of attn_cases.MODES_128 and dropout off / on rotate over the lengths of one (prec, hd) as attn_cases._rotate does.

Tolerances are the project's own (test_attn_branches_hip.py), relative to the reference tensor's maximum: exact fp32 3e-5 forward and
gradients; bf16 operands 2e-2 forward, 6e-2 gradients, the gradients' denominator at least max |dV|; LSE 1e-4 absolute, in bf16 plus the score
error of operands rounded to 8 bits, (2^-7 + 2^-16) scale max_j sum_i |q_i| |k_ji| per query.  Leaks, independence, determinism and strided
outputs: bit for bit."""
import functools
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

HEADS = (16, 32, 64, 128, 256)
LENGTHS = (37, 200, 225, 257, 300, 513, 1009, 1024)


def heads_of(hd):
    return 2 if hd <= 64 else 1


CASES = [c for prec in (ac.F32, ac.BF16) for n, hd in enumerate(HEADS) for c in ac._rotate(prec, heads_of(hd), hd, LENGTHS, ac.MODES_128, n + prec)]
# heads padded with zero lanes keep 1 / sqrt(true head size): hd 64 holding a head of 50
SCALED_CASES = [(ac.F32, 2, 64, 272, "both", -1e9, 0.2, 1 / math.sqrt(50)), (ac.BF16, 2, 64, 272, "causal", ac.NINF, 0.0, 1 / math.sqrt(50))]
# one length per (prec, hd): past both old bounds, an odd number of 16-row tiles, L % 4 = 1, more than one workgroup per (b, h)
LEAK_CASES = [(prec, heads_of(hd), hd, 613 if hd in (32, 128) else 301) for prec in (ac.F32, ac.BF16) for hd in HEADS]


def leak_id(c):
    return "%s-hd%d-L%d" % ("bf16" if c[0] else "f32", c[2], c[3])


def T_(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def rel(a, b, floor=1e-6):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), floor)


def same(a, b):
    return torch.equal(a, b)      # bit for bit up to the sign of a zero; NaN never equal


def run(prec, qkv, dO, nB, H, L, mask, ids, fill, p, b_off, scale=None, out=None):
    """Forward and backward on column views of the packed (T, 3 d) projection, as the model calls them.  Returns (O, LSE, dQ, dK, dV)."""
    from adt_amd import ops
    d = qkv.shape[1] // 3
    q, k, v = qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:]
    causal = ac.flags(mask)[0]
    sd = torch.tensor([ac.SEED], device=DEV, dtype=torch.int32)
    O, LSE = ops.attn_long_fwd(prec, q, k, v, nB, H, L, causal, ids, fill, p, sd, ac.SITE, b_off, scale=scale)
    dQ, dK, dV = ops.attn_long_bwd(prec, q, k, v, O, LSE, dO, nB, H, L, causal, ids, fill, p, sd, ac.SITE, b_off, out=out, scale=scale)
    return O, LSE, dQ, dK, dV


@functools.lru_cache(maxsize=None)
def reference(case):
    return ac.reference(case)


# ---- parity with float64 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES + SCALED_CASES, ids=ac.case_id)
def test_parity_with_float64(case):
    prec, H, hd, L, mask, fill, p, scale = case
    qkv, dO, ids, valid = ac.make_inputs(case)
    ref = reference(case)
    t = ac.true_hd(hd, scale)
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


def test_the_table_rotates_every_mode_and_both_dropout_settings_over_every_head_size():
    for prec in (ac.F32, ac.BF16):
        for hd in HEADS:
            mine = [c for c in CASES if c[0] == prec and c[2] == hd]
            assert [c[3] for c in mine] == list(LENGTHS)
            assert {c[4:6] for c in mine} == set(ac.MODES_128) and {c[6] for c in mine} == {0.0, 0.2}


# ---- mask leaks, bit for bit -------------------------------------------------------------------------------------------------------------------
def leak_inputs(prec, H, hd, L):
    r = np.random.RandomState(31 * hd + L + prec)
    d = H * hd
    qkv = r.standard_normal((ac.B * L, 3 * d)).astype(np.float32)
    dO = r.standard_normal((ac.B * L, d)).astype(np.float32)
    loud_qkv = (10.0 * r.standard_normal((ac.B * L, 3 * d))).astype(np.float32)      # fresh values of ten times the magnitude
    loud_dO = (10.0 * r.standard_normal((ac.B * L, d))).astype(np.float32)
    return r, qkv, dO, loud_qkv, loud_dO


@pytest.mark.parametrize("case", LEAK_CASES, ids=leak_id)
def test_causal_mask_leaks_nothing(case):
    """Rows >= t of Q, K, V and dO of every sequence replaced: O, LSE and dQ of the rows before t do not change in any bit.  t: 1, a group
    boundary (64 rows: the rows of other workgroups), the last tile boundary and an odd row inside the last, half-empty tile pair.  fill -inf,
    no key ids: the model code's call, chunks and tile pairs above the diagonal skipped."""
    prec, H, hd, L = case
    _, qkv, dO, loud_qkv, loud_dO = leak_inputs(prec, H, hd, L)
    base = run(prec, T_(qkv), T_(dO), ac.B, H, L, "causal", None, ac.NINF, 0.2, ac.B_OFF)
    last = 16 * ((L - 1) // 16)
    assert 256 < last < last + 3 < L and (last // 16) % 2 == 0
    row = np.arange(ac.B * L) % L
    for t in (1, 256, last, last + 3):
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
@pytest.mark.parametrize("case", LEAK_CASES, ids=leak_id)
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
        ids[0, 0], ids[1, :270], ids[2, 5] = 0, 0, 7      # a padded first key, four padded groups, and a valid key in any case
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
@pytest.mark.parametrize("case", LEAK_CASES, ids=leak_id)
def test_sequences_are_independent_and_runs_repeat(case, mask):
    """Sequence 1 replaced: every output of sequences 0 and 2 keeps every bit.  Sequence 2 alone, as a B = 1 call with b_offset + 2, gives the
    same bits again.  And a second run of the same call equals the first: no atomics, no dependence on scheduling."""
    prec, H, hd, L = case
    r, qkv, dO, loud_qkv, loud_dO = leak_inputs(prec, H, hd, L)
    ids, fill = (None, ac.NINF) if mask == "causal" else (ac.key_ids(r, L, mask)[0], -1e9)
    g, gdO = T_(qkv), T_(dO)
    kid = None if ids is None else T_(ids.reshape(-1))
    full = run(prec, g, gdO, ac.B, H, L, mask, kid, fill, 0.2, ac.B_OFF)
    again = run(prec, g, gdO, ac.B, H, L, mask, kid, fill, 0.2, ac.B_OFF)
    for name, a, w in zip(("O", "LSE", "dQ", "dK", "dV"), again, full):
        assert same(a, w), name
    x, gx = qkv.copy(), dO.copy()
    x[L:2 * L], gx[L:2 * L] = loud_qkv[L:2 * L], loud_dO[L:2 * L]
    other = run(prec, T_(x), T_(gx), ac.B, H, L, mask, kid, fill, 0.2, ac.B_OFF)
    rows = T_(np.arange(ac.B * L) // L != 1)
    rows_lse = T_(np.arange(ac.B * H * L) // (H * L) != 1)
    for name, a, w in zip(("O", "LSE", "dQ", "dK", "dV"), other, full):
        m = rows_lse if name == "LSE" else rows
        assert same(a[m], w[m]), name
    assert not same(other[0], full[0])
    sl = slice(2 * L, 3 * L)
    one = run(prec, g[sl], gdO[sl], 1, H, L, mask, None if kid is None else kid[sl], fill, 0.2, ac.B_OFF + 2)
    for name, a, w in zip(("O", "LSE", "dQ", "dK", "dV"), one, full):
        assert same(a, w[2 * H * L:] if name == "LSE" else w[sl]), name


# ---- strided outputs ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", [ac.F32, ac.BF16])
def test_backward_into_strided_views(prec):
    """out= of ops.attn_long_bwd: three column views of one (B L, 3 d + 4) buffer (the packed gradient of the in-projection).  The views equal
    the contiguous result bit for bit and the four spare columns keep their sentinel."""
    case = (prec, 2, 32, 300, "both", -1e9, 0.2, None)
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


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------------
def _zeros(L, d):
    g = torch.zeros(L, 3 * d, device=DEV)
    return g[:, :d], g[:, d:2 * d], g[:, 2 * d:]


def _both_raise(text, prec, q, k, v, B, H, L, **kw):
    from adt_amd import _lib, ops
    with pytest.raises(_lib.AdtError, match=text):
        ops.attn_long_fwd(prec, q, k, v, B, H, L, True, None, ac.NINF, **kw)
    with pytest.raises(_lib.AdtError, match=text):
        ops.attn_long_bwd(prec, q, k, v, q, torch.zeros(B * H * L, device=DEV), q, B, H, L, True, None, ac.NINF, **kw)


def test_lengths_head_sizes_and_scales_outside_the_plan_raise():
    for prec in (ac.F32, ac.BF16):
        _both_raise("L=1025 outside 1..1024", prec, *_zeros(1025, 32), 1, 1, 1025)
        _both_raise("L=0 outside 1..1024", prec, *_zeros(16, 32), 1, 1, 0)
        _both_raise("head_dim=48 unsupported", prec, *_zeros(300, 48), 1, 1, 300)
        for scale in (0.0, -0.2):
            _both_raise("must be positive", prec, *_zeros(300, 32), 1, 1, 300, scale=scale)


def test_dropout_index_space_past_2_to_32_raises():
    """(b_offset + B) H L L elements are indexed in a uint32.  At L = 1024, H = 1 the 4096 sequences before b_offset 4096 fill it: one more is
    refused with dropout on, runs with dropout off, and the last sequence that fits (b_offset 4095) runs with dropout on."""
    from adt_amd import ops
    L, hd = 1024, 16
    q, k, v = (x + 0.25 for x in _zeros(L, hd))
    sd = torch.tensor([ac.SEED], device=DEV, dtype=torch.int32)
    _both_raise("exceeds 2\\^32", ac.BF16, q, k, v, 1, 1, L, p=0.2, seed=sd, site=ac.SITE, b_offset=4096)
    for p, off in ((0.0, 4096), (0.2, 4095)):
        O, LSE = ops.attn_long_fwd(ac.BF16, q, k, v, 1, 1, L, True, None, ac.NINF, p, sd, ac.SITE, off)
        dQ, dK, dV = ops.attn_long_bwd(ac.BF16, q, k, v, O, LSE, q, 1, 1, L, True, None, ac.NINF, p, sd, ac.SITE, off)
        assert all(bool(torch.isfinite(x).all()) for x in (O, LSE, dQ, dK, dV))
        assert abs(float(LSE[L - 1]) - (math.log(L) + hd * 0.0625 / 4)) < 1e-3      # equal scores 16 * 0.25^2 / sqrt(16) over L keys


def test_the_older_kernels_bounds_are_reported():
    from adt_amd import ops
    assert [ops.attn_masked_max_len(hd) for hd in (16, 32, 64, 128, 256, 48)] == [224, 224, 224, 256, 256, 0]
