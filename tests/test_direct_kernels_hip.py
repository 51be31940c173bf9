"""GPU tests of the C-ABI stage kernels that tests/test_hip_kernels.py and tests/test_wide_kernels.py do not call: each wrapper of
adt_amd/ops.py below is run on its own against the float64 restatement in oracle/stage_refs.py, at the sizes where its grid-stride
loop, its float4 tail, its unroll or its row mask can go wrong.

Tolerances are of two kinds.  Derived ones follow from float32 rounding and are written where they are used.  MEASURED ones cover the
device's powf / sqrtf / expf / logf and the compiler's contraction: the constant is four times the largest error seen on an MI355X over
all cases of this file, it has a cap that it must stay under, and both figures stand beside it (and in
profiles/r10_direct_kernel_tests.txt).  Every test prints its figures as `MEASURE <name> <value>` before it asserts.
tests/test_stage_refs_cpu.py feeds the same comparisons deliberately wrong kernels and requires them to be rejected at these constants.
"""
import numpy as np
import pytest
import torch

from oracle import sasrec_oracle as so
from oracle import stage_refs as sr

pytestmark = pytest.mark.gpu

U24 = sr.U24

# ---- measured tolerances (MI355X, gfx950; see the module docstring) -------------------------------------------------------------------
# update error of the optimiser kernels in units of lr (stage_refs.update_err); each is 4 x the largest value seen; cap 1e-2
UPDATE_TOL_CAP = 1e-2
ADAM_UPDATE_TOL = 2.11e-4      # measured 5.27e-5 lr (adam_range, step 1 of the last range: the entries where eps decides; 5.14e-5 in another run)
ADAMW_UPDATE_TOL = 2.4e-5      # measured 5.93e-6 lr (adamw_range, the unclipped step at t = 4); wrong `decay after the update` scores 5.0e-3
CLIP_ADAM_UPDATE_TOL = 1.4e-6  # measured 3.43e-7 lr (clip_adam_pre, step 3)
# log_softmax forward: |err| <= 2**-23 * (|x| + |lz|) + LSM_FN_TOL (the part owed to logf / expf), and |err| <= LSM_ABS_TOL on rows with |x| <= 100
LSM_ABS_CAP = 2e-6
LSM_FN_TOL = 4.6e-7            # measured 1.15e-7 (H = 8)
LSM_ABS_TOL = 2e-6             # measured 5.28e-7 (524,291 rows of H = 2); 4 x that is 2.11e-6, above the cap, so the CAP is what is asserted.  The
                               # figure is no noise level: an output of magnitude 4 .. 8 carries two roundings of 2.4e-7 each ((x - m), then - log s)

OPT = dict(clip=5.0, b1=0.9, b2=0.98, eps=1e-8)
ADAM_CASE = dict(lr=1e-3, l2=1e-2, wd=0.0)       # torch.optim.Adam(weight_decay=l2)
ADAMW_CASE = dict(lr=1e-2, l2=0.0, wd=0.5)       # torch.optim.AdamW: `decay after the update` is lr * wd = 5e-3 of the update here


def dev():
    return torch.device("cuda:0")


def T_(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    return t.to(dev())


def N_(t):
    return t.detach().cpu().numpy()


def seed_t(seed):
    return torch.from_numpy(np.array([seed], dtype=np.uint32).view(np.int32)).to(dev())


def measure(name, value):
    print("MEASURE %s %.6e" % (name, value))
    return value


@pytest.fixture(scope="module")
def ops():
    from adt_amd import ops as o
    torch.cuda.init()
    return o


@pytest.fixture(scope="module")
def adt_error():
    from adt_amd import _lib
    return _lib.AdtError


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and bool((a.view(np.int32) == b.view(np.int32)).all())


# ---- supernet optimiser: grad_sumsq, adam_range, adamw_range -------------------------------------------------------------------------
OPT_N = 300001                                             # > 1024 * 256 (k_adam_range's grid cap) and > 512 * 256 (k_sumsq64's); not a multiple of 4
OPT_RANGES = [(0, 70001), (70001, 70003), (70003, 300001)]   # odd starts, as m.flat[lo:hi] has them
GRAD_SCALES = (0.02, 3.0, 0.02)


def optimiser_inputs(n, seed=20):
    """P (float32) and the three steps' gradients: P = 0.05 randn with 100 entries at 20x; G = scale * randn with 2,000 entries at 1e-7 of the
    scale (where eps = 1e-8 matters) and 100 exact zeros.  A quarter of the first step's tiny gradients meet P = 0: with a coupled l2 the
    gradient is g + l2 * p, and only there does it stay small enough for eps to decide."""
    r = np.random.RandomState(seed)
    P = 0.05 * r.randn(n)
    P[r.choice(n, min(100, n // 10), replace=False)] *= 20.0
    Gs = []
    for k, s in enumerate(GRAD_SCALES):
        g = s * r.randn(n)
        tiny = r.choice(n, min(2000, n // 5), replace=False)
        g[tiny] *= 1e-7
        if k == 0:
            P[tiny[:tiny.size // 4]] = 0.0
        g[r.choice(n, min(100, n // 10), replace=False)] = 0.0
        Gs.append(g.astype(np.float32))
    return P.astype(np.float32), Gs


# M' and V': 4 * 2**-24 relative (three roundings each) was the first bound tried.  A float32 evaluation does not owe that: the clip
# coefficient is itself computed in float32 from the 64 slots (tree sum of 64 values, 6 roundings, halved by the square root; sqrtf; the
# + 1e-6; the division: COEF_ULPS = 6 units of 2**-24 at most), it multiplies G before anything else, and V' squares g, which doubles what g
# carries.  Counting every rounding (unfused; fusing removes some): M' <= (4 + COEF_ULPS) and V' <= (7 + 2 * COEF_ULPS) units of the
# magnitudes of their terms.  (The unfused float32 emulation of tests/test_stage_refs_cpu.py, whose coefficient has 3 roundings, already
# reaches 5.2 units on V' in step 1.)
COEF_ULPS = 6
M_ULPS, V_ULPS = 4 + COEF_ULPS, 7 + 2 * COEF_ULPS


def moments_close(got, terms, ulps):
    """M' = b1 M + (1 - b1) g or V' = b2 V + (1 - b2) g^2 within ulps * 2**-24 of the magnitudes of its terms: worst ratio, <= 1 passes."""
    return sr.sum_excess(got, terms, ulps * U24)


def moment_terms(P0, G, M0, V0, gn2, l2, wd, clip, lr, b1, b2):
    """What moments_close takes for M' and for V' (float64), from the same definition as stage_refs.adam_range_ref.  g = coef G + l2 p is
    itself a sum that can cancel, so its two addends count separately: M' has the three terms b1 M, (1 - b1) coef G, (1 - b1) l2 p, and V'
    (value, magnitude) has the magnitude b2 V + (1 - b2) (|coef G| + |l2 p|)^2.  Without a coupled l2 these are |M'|'s two terms and V'
    itself, i.e. 4 * 2**-24 relative."""
    P0, G = P0.astype(np.float64), G.astype(np.float64)
    coef = min(1.0, sr.f32(clip) / (np.sqrt(gn2) + 1e-6))
    a, b = G * coef, sr.f32(l2) * (P0 * (1.0 - sr.f32(lr) * sr.f32(wd)))
    b1, b2 = sr.f32(b1), sr.f32(b2)
    v0 = b2 * V0.astype(np.float64)
    return [b1 * M0.astype(np.float64), (1 - b1) * a, (1 - b1) * b], (v0 + (1 - b2) * (a + b) ** 2, v0 + (1 - b2) * (np.abs(a) + np.abs(b)) ** 2)


def run_range_step(ops, case, P, G, M, V, lo, hi, t, slots, gn2):
    """One adam_range / adamw_range call on [lo, hi) and its comparison with the float64 reference restarted from the kernel's float32 state.
    Returns (update error in lr, worst moment ratio against M_ULPS / V_ULPS, worst moment error in units of 2**-24 of its terms)."""
    P0, M0, V0, g = N_(P[lo:hi]), N_(M[lo:hi]), N_(V[lo:hi]), N_(G[lo:hi])
    lr, l2, wd = case["lr"], case["l2"], case["wd"]
    if wd:
        ops.adamw_range(P[lo:hi], G[lo:hi], M[lo:hi], V[lo:hi], wd, OPT["clip"], lr, OPT["b1"], OPT["b2"], OPT["eps"], t, slots)
    else:
        ops.adam_range(P[lo:hi], G[lo:hi], M[lo:hi], V[lo:hi], l2, OPT["clip"], lr, OPT["b1"], OPT["b2"], OPT["eps"], t, slots)
    P1, M1, V1 = N_(P[lo:hi]), N_(M[lo:hi]), N_(V[lo:hi])
    Pr, Mr, Vr = sr.adam_range_ref(P0, g, M0, V0, gn2, l2, wd, OPT["clip"], lr, OPT["b1"], OPT["b2"], OPT["eps"], t)
    mt, vt = moment_terms(P0, g, M0, V0, gn2, l2, wd, OPT["clip"], lr, OPT["b1"], OPT["b2"])
    assert np.abs(sum(mt) - Mr).max() <= 1e-12 * max(np.abs(Mr).max(), 1e-30) and np.abs(vt[0] - Vr).max() <= 1e-12 * max(np.abs(Vr).max(), 1e-30)
    assert same_bits(N_(G[lo:hi]), g), "the gradient is an input"
    return sr.update_err(P0, P1, Pr, lr), max(moments_close(M1, mt, M_ULPS), moments_close(V1, vt, V_ULPS)), max(moments_close(M1, mt, 1), moments_close(V1, vt, 1))


def check_sumsq(ops, G, slots, what):
    """grad_sumsq into `slots`; the 64 slots must sum to the float64 ||G||^2 within n * 2**-24 relative (loose by design: the sum is
    reassociated).  Returns the float64 sum of the slots, which is what the optimiser kernels are given."""
    ops.grad_sumsq(G, slots)
    s = N_(slots).astype(np.float64)
    assert s.shape == (64,) and (s >= 0).all()
    want = float((N_(G).astype(np.float64) ** 2).sum())
    rel = abs(s.sum() - want) / max(want, 1e-300)
    measure("sumsq_rel_%s" % what, rel)
    assert rel <= G.numel() * U24, (what, rel)
    return float(s.sum())


@pytest.mark.parametrize("name", ["adam", "adamw"])
def test_supernet_optimiser_three_steps(ops, name):
    case, tol = (ADAM_CASE, ADAM_UPDATE_TOL) if name == "adam" else (ADAMW_CASE, ADAMW_UPDATE_TOL)
    assert tol <= UPDATE_TOL_CAP
    P0, Gs = optimiser_inputs(OPT_N)
    P, M, V = T_(P0), torch.zeros(OPT_N, device=dev()), torch.zeros(OPT_N, device=dev())
    slots = torch.full((64,), 1e30, device=dev())          # grad_sumsq owes the zeroing
    steps = {}
    worst_u = worst_m = 0.0
    for k in range(3):
        stepped = OPT_RANGES if k != 1 else OPT_RANGES[:1]      # step 2: the middle and the last range have grad None
        g = Gs[k].copy()
        for lo, hi in OPT_RANGES:
            if (lo, hi) not in stepped:
                g[lo:hi] = 0.0                                  # SupernetTrainer.step zeroes flat_grad; a grad of None adds nothing to the norm
        G = T_(g)
        if k == 0:
            check_sumsq(ops, T_(Gs[1]), slots, "%s_first" % name)      # a second call must overwrite the slots, not add to them
        gn2 = check_sumsq(ops, G, slots, "%s_step%d" % (name, k + 1))
        frozen = [(lo, hi, N_(P[lo:hi]), N_(M[lo:hi]), N_(V[lo:hi])) for lo, hi in OPT_RANGES if (lo, hi) not in stepped]
        for lo, hi in stepped:
            t = steps[(lo, hi)] = steps.get((lo, hi), 0) + 1
            u, m, mu = run_range_step(ops, case, P, G, M, V, lo, hi, t, slots, gn2)
            measure("%s_update_err_lr_step%d_range%d_t%d" % (name, k + 1, lo, t), u)
            measure("%s_moment_units_step%d_range%d_t%d" % (name, k + 1, lo, t), mu)
            worst_u, worst_m = max(worst_u, u), max(worst_m, m)
        for lo, hi, p_, m_, v_ in frozen:
            assert same_bits(N_(P[lo:hi]), p_) and same_bits(N_(M[lo:hi]), m_) and same_bits(N_(V[lo:hi]), v_), "range [%d, %d) was not stepped" % (lo, hi)
    assert steps == {OPT_RANGES[0]: 3, OPT_RANGES[1]: 2, OPT_RANGES[2]: 2}
    measure("%s_update_err_lr_max" % name, worst_u)
    measure("%s_moment_ratio_max" % name, worst_m)
    assert worst_m <= 1.0, "M' / V' at %.2f of their bound" % worst_m
    assert worst_u <= tol, "update error %.3e lr > %.3e lr" % (worst_u, tol)


@pytest.mark.parametrize("name", ["adam", "adamw"])
def test_supernet_optimiser_unclipped_step(ops, name):
    """The other branch of the clip: ||g|| = 0.63 < clip, so coef is exactly 1; t = 4 from non-zero moments."""
    case, tol = (ADAM_CASE, ADAM_UPDATE_TOL) if name == "adam" else (ADAMW_CASE, ADAMW_UPDATE_TOL)
    n = 1003
    P0, Gs = optimiser_inputs(n, seed=21)
    r = np.random.RandomState(22)
    P, G = T_(P0), T_(Gs[0])
    M, V = T_((0.01 * r.randn(n)).astype(np.float32)), T_((1e-4 * r.rand(n)).astype(np.float32))
    slots = torch.empty(64, device=dev())
    gn2 = check_sumsq(ops, G, slots, "%s_unclipped" % name)
    assert np.sqrt(gn2) < OPT["clip"]
    u, m, mu = run_range_step(ops, case, P, G, M, V, 1, n, 4, slots, gn2)
    measure("%s_update_err_lr_unclipped" % name, u)
    measure("%s_moment_units_unclipped" % name, mu)
    assert m <= 1.0 and u <= tol, (u, m)


def test_supernet_optimiser_edges(ops):
    r = np.random.RandomState(23)
    n = 777
    P0 = r.randn(n).astype(np.float32)
    slots = torch.zeros(64, device=dev())
    zero = torch.zeros(n, device=dev())
    # an empty range is a no-op that succeeds
    P, M, V = T_(P0), zero.clone(), zero.clone()
    ops.adam_range(P[5:5], zero[5:5], M[5:5], V[5:5], 1e-2, 5.0, 1e-3, 0.9, 0.98, 1e-8, 1, slots)
    ops.adamw_range(P[5:5], zero[5:5], M[5:5], V[5:5], 0.5, 5.0, 1e-2, 0.9, 0.98, 1e-8, 1, slots)
    assert same_bits(N_(P), P0) and not M.any() and not V.any()
    # all-zero gradient: gn2 = 0, coef = min(1, clip / 1e-6) = 1; nothing but the decay terms moves P, and everything stays finite
    assert check_sumsq(ops, zero, slots, "zero_grad") == 0.0
    ops.adam_range(P, zero, M, V, 0.0, 5.0, 1e-3, 0.9, 0.98, 1e-8, 1, slots)          # no decay: nothing moves
    assert same_bits(N_(P), P0) and not M.any() and not V.any()
    ops.adamw_range(P, zero, M, V, 0.5, 5.0, 1e-2, 0.9, 0.98, 1e-8, 1, slots)         # decoupled decay only: p *= 1 - lr * wd
    assert not M.any() and not V.any()
    p64 = P0.astype(np.float64)
    assert sr.ulp_close(N_(P), [p64, -sr.f32(1e-2) * sr.f32(0.5) * p64])
    P = T_(P0)
    ops.adam_range(P, zero, M, V, 1e-2, 5.0, 1e-3, 0.9, 0.98, 1e-8, 1, slots)         # coupled decay: the gradient is l2 * p
    Pr, Mr, Vr = sr.adam_range_ref(P0, np.zeros(n), np.zeros(n), np.zeros(n), 0.0, 1e-2, 0.0, 5.0, 1e-3, 0.9, 0.98, 1e-8, 1)
    assert np.isfinite(N_(P)).all() and np.isfinite(N_(M)).all() and np.isfinite(N_(V)).all()
    assert measure("adam_update_err_lr_zero_grad", sr.update_err(P0, N_(P), Pr, 1e-3)) <= ADAM_UPDATE_TOL
    assert sr.sum_excess(N_(M), [Mr], M_ULPS * U24) <= 1.0 and sr.sum_excess(N_(V), [Vr], V_ULPS * U24) <= 1.0


# ---- clip_adam_pre: the flagship step's optimiser without the priming launches --------------------------------------------------------
def test_clip_adam_pre_three_steps(ops):
    """adt_clip_adam_pre's contract: scal[64..128) holds partial sums of ||E||^2, scal[128..192) is zero and scal[2] the running step count
    when it is called.  The data of test_hip_kernels.py::test_clip_adam_three_steps, the priming done here."""
    assert CLIP_ADAM_UPDATE_TOL <= UPDATE_TOL_CAP
    r = np.random.RandomState(10)
    n, nE, wd, lr, clip = 5000, 1280, 1e-2, 1e-3, 5.0
    P0 = r.randn(n).astype(np.float32)
    P = {"item_emb.weight": P0[:nE].reshape(20, 64).copy(), "rest": P0[nE:].copy()}
    state = {}
    Pt, Pt2 = T_(P0.copy()), T_(P0.copy())
    M, V, M2, V2 = (torch.zeros(n, device=dev()) for _ in range(4))
    scal, scal2 = torch.zeros(192, device=dev()), torch.zeros(192, device=dev())
    worst = 0.0
    for step in range(3):
        g = (r.randn(n) * (3.0 if step == 1 else 0.02)).astype(np.float32)   # step 1 clips, others do not
        G = {"item_emb.weight": g[:nE].reshape(20, 64).copy(), "rest": g[nE:].copy()}
        nrm = np.sqrt((P["item_emb.weight"].astype(np.float64) ** 2).sum())
        G["item_emb.weight"] = G["item_emb.weight"] + (wd / nrm * P["item_emb.weight"]).astype(np.float32)
        tn, coef = so.clip_adam(P, G, state, lr=lr, clip=clip)
        # float64 reference of this step from the kernel's own float32 state
        p0, m0, v0 = N_(Pt), N_(M), N_(V)
        e2 = float((p0[:nE].astype(np.float64) ** 2).sum())
        geff = g.astype(np.float64)
        geff[:nE] += sr.f32(wd) / np.sqrt(e2) * p0[:nE].astype(np.float64)
        gn2 = float((geff ** 2).sum())
        Pr, _, _ = sr.adam_range_ref(p0, geff, m0, v0, gn2, 0.0, 0.0, clip, lr, 0.9, 0.98, 1e-8, step + 1)
        # the priming that adt_sasrec_step_begin does in production
        scal[64:128] = e2 / 64.0
        scal[128:192] = 0.0
        Gt = T_(g)
        ops.clip_adam_pre(Pt, Gt, M, V, nE, wd, clip, lr, 0.9, 0.98, 1e-8, scal)
        ops.clip_adam(Pt2, T_(g), M2, V2, nE, wd, clip, lr, 0.9, 0.98, 1e-8, scal2)
        want = np.concatenate([P["item_emb.weight"].reshape(-1), P["rest"]])
        got = N_(Pt)
        e = float(np.abs(got.astype(np.float64) - want).max()) / max(float(np.abs(want).max()), 1e-6)
        assert e <= 2e-6, "adam step %d: rel err %.3e" % (step, e)
        u = measure("clip_adam_pre_update_err_lr_step%d" % (step + 1), sr.update_err(p0, got, Pr, lr))
        worst = max(worst, u)
        s = N_(scal)
        assert abs(float(s[1]) - gn2) <= n * U24 * gn2, (s[1], gn2)
        assert abs(np.sqrt(s[1]) - tn) < 1e-4 * tn
        assert s[2] == step + 1
        assert abs(float(s[0]) - e2) <= 64 * U24 * e2
    measure("clip_adam_pre_update_err_lr_max", worst)
    assert worst <= CLIP_ADAM_UPDATE_TOL
    # clip_adam primes scal itself and shares every kernel: after three steps the two copies agree within twice the update tolerance
    # (each stored value owes half an ulp of its own)
    a, b = N_(Pt), N_(Pt2)
    diff = np.abs(a.astype(np.float64) - b.astype(np.float64)) - 0.5 * np.spacing(np.abs(a)) - 0.5 * np.spacing(np.abs(b))
    d = measure("clip_adam_pre_vs_clip_adam_lr", float(np.maximum(diff, 0).max()) / lr)
    assert d <= 2 * CLIP_ADAM_UPDATE_TOL


# ---- log_softmax over rows of H <= 8 ------------------------------------------------------------------------------------------------
def lsm_rows(rows, H, seed=30):
    r = np.random.RandomState(seed + H)
    X = r.randn(rows, H)
    X[0:50] = r.randn(50, 1)                    # all-equal rows
    X[50:100] += 80.0
    X[100:150] -= 80.0
    X[150:200] += 1e4                           # without the max shift exp overflows
    X[200:250] -= 1e4
    X[250:260, r.randint(0, H)] = -1e30         # one entry out of range of everything
    return X.astype(np.float32)


def lsm_fwd_errors(X, Y):
    """(largest |err| beyond 2**-23 * (|x| + |lz|) over all rows, largest |err| on the rows with |x| <= 100) of a float32 log_softmax Y of
    X against the float64 reference; (inf, inf) when Y is not finite."""
    if Y.shape != X.shape or not np.isfinite(Y).all():
        return np.inf, np.inf
    want = sr.log_softmax_ref(X)
    x64 = X.astype(np.float64)
    lz = x64 - want
    err = np.abs(Y.astype(np.float64) - want)
    small = np.abs(X).max(1) <= 100
    assert small.sum() >= X.shape[0] - 200
    return float(np.maximum(err - 2.0 ** -23 * (np.abs(x64) + np.abs(lz)), 0).max()), float(err[small].max())


def lsm_bwd_ratios(X, Y, dY, old, got):
    """(value, row sum, plain row sum) of a float32 log_softmax backward `got` (old: the prior dX of accumulate = 1, or None), each as the
    worst ratio error / bound: <= 1 passes.
    value: against dY - exp(Y) * sum(dY) (+ old) in float64.  Roundings: the sum of H values, expf (2**-22 relative allowed; the device
    documents 1 ulp), the product, the subtraction, the accumulate.
    row sum: each row of the gradient sums to sum(dY) * (1 - sum(exp(Y))): zero but for what the float32 Y itself is off a normalised row
    (2**-24 of |lz|: 1e-3 on the rows at 1e4), which the reference shares; beyond that, H * 2**-22 * sum|dY|.
    plain row sum: the rows with |x| <= 4.5 sum to zero within the same bound outright."""
    H = X.shape[1]
    if not np.isfinite(got).all():
        return np.inf, np.inf, np.inf
    o = 0 if old is None else old.astype(np.float64)
    sabs = np.abs(dY.astype(np.float64)).sum(1, keepdims=True)
    sm = np.exp(Y.astype(np.float64))
    want = sr.log_softmax_bwd_ref(Y, dY, old)
    bound = 2.0 ** -23 * (np.abs(dY) + np.abs(o)) + sm * sabs * (H * 2.0 ** -23 + 2.0 ** -22)
    err = np.abs(got - want)
    value = float(np.where(err == 0, 0.0, err / np.where(bound > 0, bound, np.finfo(np.float64).tiny)).max())
    g, gref = got.astype(np.float64) - o, want - o
    rb = np.where(sabs > 0, H * 2.0 ** -22 * sabs, np.finfo(np.float64).tiny)
    rs = np.abs(g.sum(1, keepdims=True) - gref.sum(1, keepdims=True))
    normal = np.abs(X).max(1) <= 4.5
    assert normal.sum() > X.shape[0] // 2
    plain = np.abs(g.sum(1, keepdims=True))[normal]
    return value, float(np.where(rs == 0, 0.0, rs / rb).max()), float(np.where(plain == 0, 0.0, plain / rb[normal]).max())


def lsm_bwd_inputs(rows, H, Y):
    r = np.random.RandomState(31)
    dY = r.randn(rows, H).astype(np.float32)
    dY[::7] = 0.0
    sabs = np.abs(dY.astype(np.float64)).sum(1, keepdims=True)
    # the prior dX of accumulate = 1 stays within half of the row's sum|dY|: the float32 store of old + g rounds at 2**-24 of |old + g|, which
    # the row-sum bound (stated in sum|dY| alone) has to cover as well
    old = ((r.rand(rows, H) - 0.5) * sabs).astype(np.float32)
    return dY, old


@pytest.mark.parametrize("rows,H", [(1000, h) for h in range(1, 9)] + [(2048 * 256 + 3, 2)])
def test_log_softmax_fwd_bwd(ops, rows, H):
    assert LSM_ABS_TOL <= LSM_ABS_CAP
    X = lsm_rows(rows, H)
    Yt = ops.log_softmax_fwd(T_(X), H)
    Y = N_(Yt)
    excess, abs_small = lsm_fwd_errors(X, Y)
    measure("lsm_fwd_excess_rows%d_H%d" % (rows, H), excess)
    measure("lsm_fwd_abs_rows%d_H%d" % (rows, H), abs_small)
    assert excess <= LSM_FN_TOL and abs_small <= LSM_ABS_TOL, (excess, abs_small)
    if H == 1:
        assert not Y.any()
    # backward from the kernel's own Y: dX (+)= dY - exp(Y) * sum(dY)
    dY, old = lsm_bwd_inputs(rows, H, Y)
    for acc in (0, 1):
        dX = T_(old.copy()) if acc else torch.full((rows, H), float("nan"), device=dev())
        ops.log_softmax_bwd(Yt, T_(dY), H, dX, acc)
        got = N_(dX)
        value, rowsum, plain = lsm_bwd_ratios(X, Y, dY, old if acc else None, got)
        measure("lsm_bwd_value_ratio_rows%d_H%d_acc%d" % (rows, H, acc), value)
        measure("lsm_bwd_rowsum_ratio_rows%d_H%d_acc%d" % (rows, H, acc), rowsum)
        measure("lsm_bwd_plain_rowsum_ratio_rows%d_H%d_acc%d" % (rows, H, acc), plain)
        assert value <= 1.0 and rowsum <= 1.0 and plain <= 1.0, (value, rowsum, plain)
        if H == 1 and not acc:
            assert not got.any()


@pytest.mark.parametrize("H", [0, 9])
def test_log_softmax_rejects_width(ops, adt_error, H):
    X = torch.zeros(72, device=dev())
    with pytest.raises(adt_error):
        ops.log_softmax_fwd(X, H)
    with pytest.raises(adt_error):
        ops.log_softmax_bwd(X, X, H, torch.zeros(72, device=dev()), 0)


# ---- axpy -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [4 * 1000, 2048 * 1024 + 4 * 77])      # the second is above the grid cap of 2048 blocks x 256 float4
@pytest.mark.parametrize("d", [None, 4, 64, 52])
def test_axpy(ops, n, d):
    r = np.random.RandomState(40)
    src, old = r.randn(n).astype(np.float32), r.randn(n).astype(np.float32)
    ids = None
    if d is not None:
        nrow = (n + d - 1) // d
        ids = np.where(r.rand(nrow) < 0.33, 0, r.randint(1, 9, size=nrow)).astype(np.int32)
        ids[0] = ids[-1] = 0
        ids[1] = 3
    live = np.ones(n, bool) if ids is None else np.repeat(ids != 0, d)[:n]
    src_t, ids_t = T_(src), (None if ids is None else T_(ids))
    for acc in (0, 1):
        for alpha in (1.0, -0.37):
            dst = T_(old.copy()) if acc else torch.full((n,), float("nan"), device=dev())
            out = ops.axpy(dst, src_t, alpha, acc, ids_t, d or 0)
            assert out is dst
            got = N_(dst)
            if acc:
                assert same_bits(got[~live], old[~live])
            else:
                assert not got[~live].any()
            terms = sr.axpy_terms(old, src, alpha, acc, ids, d or 0)
            assert sr.ulp_close(got[live], [t[live] for t in terms]), (acc, alpha)
            if alpha == 1.0 and not acc:
                assert same_bits(got[live], src[live])


def test_axpy_rejects_shapes(ops, adt_error):
    a, b = torch.zeros(64, device=dev()), torch.ones(64, device=dev())
    ids = torch.ones(64, device=dev(), dtype=torch.int32)
    with pytest.raises(adt_error):
        ops.axpy(a[:6], b[:6])
    for d in (6, 0):
        with pytest.raises(adt_error):
            ops.axpy(a, b, mask_ids=ids, d=d)
    assert not a.any()


# ---- drop_lanes -------------------------------------------------------------------------------------------------------------------------
LANES = [(1, 50, 64), (2, 25, 32), (2, 50, 64), (3, 50, 64), (1, 100, 128), (2, 100, 128), (4, 64, 64)]
PAD = 3e38
SENT = -7.25


def lanes_buffer(r, T, lanes, fill_pad=PAD):
    """A (T, d_pad + 8) buffer whose columns [4, 4 + d_pad) are the padded rows: randn (never zero) on the live lanes, `fill_pad` on the pad
    lanes, SENT in the slack columns.  Returns (buffer, the (T, d_pad) values)."""
    live, _ = sr.lane_cols(lanes)
    dp = live.size
    v = r.randn(T, dp).astype(np.float32)
    v[v == 0] = 1.0
    v[:, ~live] = fill_pad
    buf = np.full((T, dp + 8), SENT, np.float32)
    buf[:, 4:4 + dp] = v
    return buf, v


def check_drop_lanes(got, S, R, R2, ids, lanes, p, seed, site, row_offset):
    """Everything a (T, d_pad) float32 result of adt_drop_lanes owes (S, R, R2: the (T, d_pad) inputs, R / R2 / ids may be None)."""
    live, _ = sr.lane_cols(lanes)
    T = S.shape[0]
    on = np.ones(T, bool) if ids is None else ids != 0
    assert got.shape == S.shape and np.isfinite(got).all()
    assert not got[:, ~live].any() and not got[~on].any(), "pad lanes / masked rows must be exact zeros"
    terms, keep = sr.drop_lanes_terms(S, lanes, p, seed, site, row_offset, R, R2, ids)
    assert sr.ulp_close(got, terms), "values"
    if R is None and R2 is None:
        assert ((got != 0) == (keep & live[None, :] & on[:, None])).all(), "zero pattern differs from the oracle's mask"
    if p in (0.0, 0.5):      # the scale is a power of two: every product is exact, the sums round once each whatever is fused
        ks = np.float32(sr.drop_scale(p)) if p else np.float32(1.0)
        with np.errstate(over="ignore"):      # (the pad lanes hold 3e38)
            w = np.where(keep, S * ks, np.float32(0))
            for r_ in (R, R2):
                if r_ is not None:
                    w = w + r_
        w = np.where(live[None, :] & on[:, None], w, np.float32(0)).astype(np.float32)
        assert same_bits(got + np.float32(0), w + np.float32(0)), "not bit-equal to the float32 expression"


@pytest.mark.parametrize("lanes", LANES)
@pytest.mark.parametrize("p", [0.0, 0.25, 0.5])
def test_drop_lanes(ops, lanes, p):
    r = np.random.RandomState(50)
    T, seed, site = 37, 4321, 19
    live, _ = sr.lane_cols(lanes)
    dp = live.size
    sbuf, S = lanes_buffer(r, T, lanes)
    rbuf, R = lanes_buffer(r, T, lanes)
    r2buf, R2 = lanes_buffer(r, T, lanes)
    ids = np.where(r.rand(T) < 0.3, 0, 5).astype(np.int32)
    ids[0], ids[1] = 0, 5
    St, Rt, R2t, ids_t = T_(sbuf), T_(rbuf), T_(r2buf), T_(ids)
    view = lambda t: t[:, 4:4 + dp]
    for row_offset in (0, 1000):
        for use_r, use_r2, use_ids in [(a, b, c) for a in (0, 1) for b in (0, 1) for c in (0, 1)]:
            kw = dict(R=view(Rt) if use_r else None, R2=view(R2t) if use_r2 else None, mask_ids=ids_t if use_ids else None)
            obuf = torch.full((T, dp + 8), SENT, device=dev())
            out = ops.drop_lanes(view(St), lanes, p, seed_t(seed), site, row_offset, out=view(obuf), **kw)
            assert out.data_ptr() == view(obuf).data_ptr()
            ob = N_(obuf)
            assert (ob[:, :4] == SENT).all() and (ob[:, 4 + dp:] == SENT).all(), "slack columns written"
            check_drop_lanes(ob[:, 4:4 + dp], S, R if use_r else None, R2 if use_r2 else None, ids if use_ids else None, lanes, p, seed, site, row_offset)
            s2 = T_(sbuf)                       # in place: out = S
            ops.drop_lanes(view(s2), lanes, p, seed_t(seed), site, row_offset, out=view(s2), **kw)
            assert same_bits(N_(s2), ob)
    if p:
        _, keep = sr.drop_lanes_terms(S, lanes, p, seed, site, 0)
        assert abs((1 - keep[:, live].mean()) - p) < 0.08


def test_drop_lanes_rejects_shapes(ops, adt_error):
    T = 8
    S = torch.ones(T, 16, device=dev())
    with pytest.raises(adt_error):
        ops.drop_lanes(S, (1, 3, 16))                      # d_pad = 16 is not 64, 128, 192 or 256
    lanes = (1, 50, 64)
    good = torch.ones(T, 64, device=dev())
    odd = torch.ones(T, 70, device=dev())[:, :64]          # ld % 4 != 0
    short = torch.as_strided(torch.ones(T * 64, device=dev()), (T, 64), (60, 1))      # ld < d_pad
    for bad in (odd, short):
        with pytest.raises(adt_error):
            ops.drop_lanes(bad, lanes, out=torch.empty(T, 64, device=dev()))
        with pytest.raises(adt_error):
            ops.drop_lanes(good, lanes, out=bad)
        with pytest.raises(adt_error):
            ops.drop_lanes(good, lanes, R=bad)
        with pytest.raises(adt_error):
            ops.drop_lanes(good, lanes, R2=bad)
    assert float(good.min()) == 1.0 and float(odd.min()) == 1.0


# ---- lane_map ---------------------------------------------------------------------------------------------------------------------------
def lane_tables(d, H):
    from adt_amd import wide
    hd, hd_pad, d_pad = wide.padded_layout(d, H)
    ref = [("w", (d, d)), ("qkv", (3 * d, d)), ("b", (d,)), ("cls", (H, hd))]
    pad = [("w", (d_pad, d_pad)), ("qkv", (3 * d_pad, d_pad)), ("b", (d_pad,)), ("cls", (H, hd_pad))]
    offs, off = {}, 0
    for name, shape in pad:
        offs[name] = off
        off += int(np.prod(shape)) + 4          # tensors do not abut
    return wide.lane_index(ref, pad, offs, d, H), off


@pytest.mark.parametrize("d,H", [(50, 1), (50, 2), (100, 2)])
def test_lane_map(ops, d, H):
    r = np.random.RandomState(60)
    index, total = lane_tables(d, H)
    n = index.size
    padded = r.randn(total).astype(np.float32)
    idx_t, pt = T_(index), T_(padded)
    compact = torch.full((n,), SENT, device=dev())
    ops.lane_map(pt, compact, idx_t, False)
    assert same_bits(N_(compact), sr.lane_map_ref(padded, None, index, False)) and same_bits(N_(pt), padded)
    vals = r.randn(n).astype(np.float32)
    buf = torch.full((total,), SENT, device=dev())
    ops.lane_map(buf, T_(vals), idx_t, True)
    assert same_bits(N_(buf), sr.lane_map_ref(np.full(total, SENT, np.float32), vals, index, True))
    back = torch.empty(n, device=dev())
    ops.lane_map(buf, back, idx_t, False)
    assert same_bits(N_(back), vals)
    before = N_(buf)
    ops.lane_map(buf, back[:0], idx_t[:0], True)          # n = 0
    ops.lane_map(buf, back[:0], idx_t[:0], False)
    assert same_bits(N_(buf), before)


def test_lane_map_above_grid_cap(ops):
    n = 4096 * 1024 + 5
    g = torch.Generator(device="cpu").manual_seed(61)
    perm = torch.randperm(n, generator=g).to(torch.int32).to(dev())
    padded = torch.randn(n, generator=g).to(dev())
    compact = torch.full((n,), SENT, device=dev())
    ops.lane_map(padded, compact, perm, False)
    assert torch.equal(compact, padded[perm.long()])
    buf = torch.full((n,), SENT, device=dev())
    ops.lane_map(buf, compact, perm, True)
    assert torch.equal(buf, padded)


# ---- item_scatter + replica_reduce --------------------------------------------------------------------------------------------------------
def table_grad_ratio(got, prefill, want, mag, c):
    """A float32 table `got` = prefill + (atomic sums whose float64 value is `want`, magnitudes `mag`) against the bound
    c * 2**-24 * (|prefill| + mag) per entry (c: scalar or per entry): worst ratio, <= 1 passes.  Entries without an addend (mag == 0) must
    keep the prefill's bits."""
    assert got.shape == prefill.shape and np.isfinite(got).all()
    assert same_bits(got[mag == 0], prefill[mag == 0]), "entries that receive nothing changed"
    return sr.sum_excess(got, (prefill.astype(np.float64) + want, np.abs(prefill) + mag), c * U24)


@pytest.mark.parametrize("d", [64, 52, 256])
@pytest.mark.parametrize("hot", ["half", "all"])
def test_item_scatter_replica_reduce(ops, d, hot):
    """dE - prefill against np.add.at.  Bound per entry with c non-zero addends: (c + 3) * 2**-24 * (|prefill| + sum|addends|).  The c adds
    (the first add into a zeroed replica is exact, the fold adds one rounding per non-empty replica: c roundings of partial sums, in any
    order) give c * 2**-24; the addend itself is G * (rowscale * scale) * dropscale, three float32 products: 3 * 2**-24 of it.  Entries
    without an addend keep the prefill's bits."""
    r = np.random.RandomState(70)
    L, V = 43, 40
    T = 7 * L
    assert T == 301
    ids = r.randint(0, V + 1, size=T).astype(np.int32)
    ids[r.rand(T) < 0.1] = 0
    if hot == "half":
        ids[r.choice(T, T // 2, replace=False)] = 17
        ids[ids == 23] = 0                       # an item that never occurs
    else:
        ids[:] = 29
    ids[0] = 0
    gbuf = r.randn(T, d + 12).astype(np.float32)
    G = gbuf[:, 8:8 + d]
    rs = r.randn(T).astype(np.float32)
    rs[::5] = 0.0
    prefill = r.randn(V + 1, d).astype(np.float32)
    stride = (V + 1) * d + 8
    seed, site, row_offset = 777, 7, 3 * L
    Gt, ids_t, rs_t = T_(gbuf)[:, 8:8 + d], T_(ids), T_(rs)
    worst = 0.0
    for use_rs in (0, 1):
        for scale in (1.0, 8.0):
            for p in (0.0, 0.25):
                want, mag, cnt = sr.item_scatter_ref(ids, G, rs if use_rs else None, scale, p, seed, site, row_offset, V + 1)
                assert not cnt[0].any() and (hot == "all" or cnt.max() >= T // 4)
                for nrep in (1, 3, 7, 8, 9, 17):
                    rep = torch.full((nrep * stride,), 1e30, device=dev())
                    rv = rep.view(nrep, stride)
                    rv[:, :(V + 1) * d] = 0.0
                    ops.item_scatter(ids_t, Gt, rs_t if use_rs else None, scale, p, seed_t(seed), site, row_offset, rep, nrep, stride if nrep > 1 else 0)
                    dE = T_(prefill.copy())
                    ops.replica_reduce(dE, rep, nrep, stride if nrep > 1 else 0)
                    got = N_(dE)
                    assert (N_(rv[:, (V + 1) * d:]) == np.float32(1e30)).all(), "the gaps between the replicas were written"
                    assert ((mag == 0) == (cnt == 0)).all() and same_bits(got[0], prefill[0])
                    x = table_grad_ratio(got, prefill, want, mag, cnt + 3)
                    worst = max(worst, x)
                    assert x <= 1.0, (use_rs, scale, p, nrep, x)
    measure("item_scatter_bound_ratio_d%d_%s" % (d, hot), worst)


def test_replica_reduce_above_grid_cap_and_shapes(ops, adt_error):
    r = np.random.RandomState(71)
    n = 1024 * 1024 + 4 * 13
    stride = n + 8
    dst, rep = r.randn(n).astype(np.float32), r.randn(2 * stride).astype(np.float32)
    dt, rt = T_(dst), T_(rep)
    ops.replica_reduce(dt, rt, 2, stride)
    assert sr.ulp_close(N_(dt), [dst, rep[:n], rep[stride:stride + n]])
    assert same_bits(N_(rt), rep)
    before = N_(dt)
    with pytest.raises(adt_error):
        ops.replica_reduce(dt[:6], rt, 2, stride)
    with pytest.raises(adt_error):
        ops.replica_reduce(dt[:8], rt, 2, 6)
    assert same_bits(N_(dt), before)


# ---- posemb_bwd ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 5, 32, 33, 70])      # 32 batch slices: 33 leaves half of them empty, 70 gives a ragged last one
@pytest.mark.parametrize("d", [64, 52, 256])           # L * d / 4 is never a multiple of 256
def test_posemb_bwd(ops, B, d):
    """dP - prefill against the float64 column sums.  Bound per entry: (B + 1) * 2**-24 * (|prefill| + sum|addends|): at most B roundings of
    partial sums (register sums per batch slice, one atomic per slice), and each addend is the float32 product dX * dropscale (2**-24 of
    it).  Entries without an addend keep the prefill's bits."""
    r = np.random.RandomState(80 + B)
    L, seed, site = 37, 99, 3
    ids = r.randint(1, 50, size=(B, L)).astype(np.int32)
    for b in range(B):
        ids[b, : r.randint(0, L)] = 0           # left padding (row 0 may be padded entirely)
    ids[:, 5] = 0                               # a position that is padding in every sequence
    dX = r.randn(B * L, d).astype(np.float32)
    prefill = r.randn(L, d).astype(np.float32)
    for p, row_offset in ((0.0, 0), (0.25, 5 * L)):
        want, mag = sr.posemb_bwd_ref(ids, dX, L, p, seed, site, row_offset)
        dP = T_(prefill.copy())
        ops.posemb_bwd(T_(ids.reshape(-1)), T_(dX), L, p, seed_t(seed), site, row_offset, dP)
        got = N_(dP)
        assert (mag[5] == 0).all()
        x = measure("posemb_bound_ratio_B%d_d%d_p%g" % (B, d, p), table_grad_ratio(got, prefill, want, mag, B + 1))
        assert x <= 1.0


def test_posemb_bwd_rejects_shapes(ops, adt_error):
    ids = torch.ones(74, device=dev(), dtype=torch.int32)
    dP = torch.zeros(37, 64, device=dev())
    with pytest.raises(adt_error):
        ops.posemb_bwd(ids, torch.ones(74, 6, device=dev()), 37, 0.0, seed_t(1), 0, 0, dP)      # d % 4
    with pytest.raises(adt_error):
        ops.posemb_bwd(ids[:38], torch.ones(38, 64, device=dev()), 37, 0.0, seed_t(1), 0, 0, dP)      # T % L
    assert not dP.any()


# ---- logits_bwd_df ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 15, 16, 333])
@pytest.mark.parametrize("d", [64, 52, 128, 256])
def test_logits_bwd_df(ops, T, d):
    r = np.random.RandomState(90)
    V = 30
    E = (r.randn(V + 1, d) / 4).astype(np.float32)
    pos = r.randint(0, V + 1, size=T).astype(np.int32)
    neg = r.randint(0, V + 1, size=T).astype(np.int32)
    pos[0] = 0
    if T > 4:
        neg[1] = 0
        neg[2] = pos[2]
        neg[3] = pos[3] = 0
    dpos, dneg = r.randn(T).astype(np.float32), r.randn(T).astype(np.float32)
    dpos[::4] = 0.0
    dneg[1::4] = 0.0
    Et, pt, nt, gp, gn = T_(E), T_(pos), T_(neg), T_(dpos), T_(dneg)
    dF = ops.logits_bwd_df(Et, pt, nt, gp, gn)
    got = N_(dF)
    assert got.shape == (T, d)
    assert sr.ulp_close(got, sr.logits_bwd_df_terms(E, pos, neg, dpos, dneg))
    # adt_sasrec.hip swaps adt_logits_bwd for adt_logits_bwd_df when the deterministic table gradient is on: the same dF, bit for bit
    dE = torch.zeros(V + 1, d, device=dev())
    dF2 = ops.logits_bwd(T_(r.randn(T, d).astype(np.float32)), Et, pt, nt, gp, gn, dE)
    assert same_bits(N_(dF2), got)
