"""GPU: every arm of the dense layers of the wide C ABI (adt_dense_fwd, adt_dense_bwd) called directly, over the case table of tests/dense_cases.py.
tests/test_dense_cases_cpu.py proves on the CPU that the table reaches every kernel instantiation and loop regime the plan (adt_wide_plan.h) can
choose -- k_dense_fwd256<0..7>, k_dense_fwd_rows<KB, CH>, k_dense_fwd<PREC, BN>; k_dense_dx256<NB>, k_dense_dx_rows<KB, has_u>, k_dense_bwd_dx<PREC, BN>
with and without the split of N; k_dense_dw256 + reduce, k_dense_dw_rows, k_dense_dw64 with partials or atomics, k_dense_bwd_dw<PREC, BN> -- in one
stage and in several, and every fallback an unaligned operand or a missing workspace triggers.

(a), (b), (c): every output element against the float64 reference under the bounds derived in the docstring of dense_cases.py; dropped and masked
elements, rows at or beyond t_dev and the padding of strided outputs bit for bit.  (d): the same with ADT_STAGE256=0, in a child process (the switch
is read once).  (e): bit for bit, no reference."""
import contextlib
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import dense_cases as dc  # noqa: E402

DEV = "cuda:0"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOUD = 1e30      # what the padding columns of dY hold: a kernel that read them would not stay within any bound


def stage256_on_in_env():
    """adt_env_on("ADT_STAGE256"): on unless the value parses to 0."""
    e = os.environ.get("ADT_STAGE256")
    if e is None:
        return True
    digits = e.strip().lstrip("+-")
    n = 0
    for ch in digits:
        if not ch.isdigit():
            break
        n = n * 10 + int(ch)
    return n != 0


STAGE256 = stage256_on_in_env()


def T_(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class Buf:
    """An operand in the layout of a case: `store` is everything allocated, `view` the (rows, cols) window the kernel gets (row stride ld, base `off`
    floats into the storage)."""

    def __init__(self, c, op, rows, cols, fill):
        self.rows, self.cols, self.ld = rows, cols, dc.ld_of(c, op)
        self.off = 1 if c.layout == op + "+off" else 0
        self.store = torch.full((rows * self.ld + 4,), float(fill), device=DEV)
        self.view = self.store[self.off:self.off + rows * self.ld].view(rows, self.ld)[:, :cols]
        assert (self.view.data_ptr() % 16 == 0 and self.ld % 4 == 0) == bool(dc.operand_ok(c, op)) or op == "dY"

    def put(self, a, rows=None):
        self.view[:a.shape[0] if rows is None else rows].copy_(T_(a)[:a.shape[0] if rows is None else rows])
        return self

    def host(self):
        return self.view.cpu().numpy()

    def untouched(self, live, fill):
        """Everything but the first `live` rows of the window still holds `fill`, bit for bit."""
        s = self.store.cpu().numpy().view(np.uint32)
        body = s[self.off:self.off + self.rows * self.ld].reshape(self.rows, self.ld)
        rest = [s[:self.off], s[self.off + self.rows * self.ld:], body[live:].reshape(-1), body[:live, self.cols:].reshape(-1)]
        return all(bool(np.all(x == np.float32(fill).view(np.uint32))) for x in rest)


def vec(c, op, a):
    """bias: contiguous, or one float into a larger buffer."""
    off = 1 if c.layout == op + "+off" else 0
    store = torch.zeros(a.shape[0] + 4, device=DEV)
    store[off:off + a.shape[0]] = T_(a)
    return store[off:off + a.shape[0]]


def scalars(c, inp):
    seed = torch.tensor([dc.SEED], device=DEV, dtype=torch.int32)
    tdev = torch.tensor([inp["live"]], device=DEV, dtype=torch.int32) if c.t_dev else None
    ids = T_(inp["ids"]) if c.mask else None
    return seed, tdev, ids


def forward(c, inp):
    """adt_dense_fwd on the layout of the case.  Returns (Y, U) as Buf (U None unless saved)."""
    from adt_amd import _lib, ops
    seed, tdev, ids = scalars(c, inp)
    X, W = T_(inp["X"]), T_(inp["W"])
    b = vec(c, "bias", inp["b"]) if c.bias else None
    R = Buf(c, "R", c.T, c.N, 0.0).put(inp["R"]) if c.R else None
    R2 = Buf(c, "R2", c.T, c.N, 0.0).put(inp["R2"]) if c.R2 else None
    Y = Buf(c, "Y", c.T, c.N, dc.SENTINEL)
    U = Buf(c, "U", c.T, c.N, dc.SENTINEL) if c.save_u else None
    p, ld = ops._p, ops._ld
    v = lambda x: None if x is None else x.view      # noqa: E731
    _lib.check(_lib.load().adt_dense_fwd(c.prec, p(X), ld(X), p(W), ld(W), p(b), c.T, c.K, c.N, c.act, p(v(U)), ld(v(U)), float(c.p), p(seed), dc.SITE, dc.ROW_OFF,
                                         p(v(R)), ld(v(R)), p(v(R2)), ld(v(R2)), p(ids), p(Y.view), ld(Y.view), p(tdev), ops._stream()), "dense_fwd")
    torch.cuda.synchronize()
    return Y, U


@contextlib.contextmanager
def workspace(c):
    """ws == "none": unregister the workspace through the C ABI and keep ops.dense_bwd from registering it again; put everything back afterwards."""
    from adt_amd import _lib, ops
    if c.ws == "registered" or "w" not in c.want:
        yield
        return
    lib = _lib.load()
    assert lib.adt_dense_bwd_ws_bytes(c.prec, c.T, c.K, c.N) > 0, "the shape would not have used the workspace"
    saved = ops._ensure_dense_ws
    try:
        _lib.check(lib.adt_dense_workspace(None, 0), "dense_workspace")
        ops._ensure_dense_ws = lambda device: None
        yield
    finally:
        torch.cuda.synchronize()
        ops._ensure_dense_ws = saved
        ops._DENSE_WS.pop("current", None)
        saved(torch.device(DEV))


def backward(c, inp, U):
    """adt_dense_bwd on the layout of the case, dW and db accumulating into DW0 / DB0.  Returns (dX Buf or None, dW, db as arrays or None)."""
    from adt_amd import ops
    seed, tdev, ids = scalars(c, inp)
    X, W = T_(inp["X"]), T_(inp["W"])
    dY = Buf(c, "dY", c.T, c.N, LOUD).put(inp["dY"])
    dX = None
    if "x" in c.want:
        dX = Buf(c, "dX", c.T, c.K, dc.SENTINEL)
        if c.beta:
            dX.put(inp["dX0"], inp["live"])
    dW = torch.full((c.N, c.K), dc.DW0, device=DEV) if "w" in c.want else None
    db = torch.full((c.N,), dc.DB0, device=DEV) if "b" in c.want else None
    with workspace(c):
        ops.dense_bwd(c.prec, dY.view, X, W, dW, db, None if dX is None else dX.view, bool(c.beta), c.act, None if U is None else U.view, c.p, seed, dc.SITE, dc.ROW_OFF,
                      ids, tdev)
        torch.cuda.synchronize()
    return dX, None if dW is None else dW.cpu().numpy(), None if db is None else db.cpu().numpy()


def ratio(got, want, bound):
    """max |got - want| / bound; the bound is positive wherever something was summed."""
    err = np.abs(np.asarray(got, np.float64) - want)
    assert np.isfinite(got).all()
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err > 0, err / bound, 0.0)
    return float(r.max()) if r.size else 0.0


def check_forward(c, keep=None):
    """Runs the forward, holds it against the reference.  Returns (ratios {name: error / bound}, the saved U as a Buf or None); keep: a dictionary
    that receives {c: U} before anything is judged (the backward of the case runs on it whatever the forward's verdict)."""
    inp = dc.make_inputs(c)
    ref = dc.ref_fwd(c, inp)
    live = inp["live"]
    Y, U = forward(c, inp)
    if keep is not None:
        keep.clear()
        keep[c] = U
    y = Y.host()
    out = dict(Y=ratio(y[:live], ref["Y"][:live], ref["e_y"][:live]), Y_plain=ratio(y[:live], ref["Y_plain"][:live], ref["e_plain"][:live]))
    ex = ref["exact"][:live]
    assert np.array_equal(y[:live][ex], ref["exact_value"][:live][ex]), "a dropped or masked element is not exactly fl(R + R2) / 0"
    assert Y.untouched(live, dc.SENTINEL), "Y: a row at or beyond t_dev or a padding column was written"
    if U is not None:
        out["U"] = ratio(U.host()[:live], ref["U"][:live], ref["e_v"][:live])
        assert U.untouched(live, dc.SENTINEL), "U: a row at or beyond t_dev or a padding column was written"
    return out, U


def check_backward(c, U):
    inp = dc.make_inputs(c)
    live = inp["live"]
    ref = dc.ref_bwd(c, inp, None if U is None else U.host())
    dX, dW, db = backward(c, inp, U)
    out = {}
    if dX is not None:
        g = dX.host()
        out["dX"] = ratio(g[:live], ref["dX"][:live], ref["e_dx"][:live])
        out["dX_plain"] = ratio(g[:live], ref["dX_plain"][:live], ref["e_dx_plain"][:live])
        z = ref["zero_rows"][:live]
        assert np.array_equal(g[:live][z], inp["dX0"][:live][z] if c.beta else np.zeros((int(z.sum()), c.K), np.float32)), "dX of a masked row is not exactly the old value / 0"
        assert dX.untouched(live, dc.SENTINEL), "dX: a row at or beyond t_dev or a padding column was written"
    if dW is not None:
        out["dW"] = ratio(dW, ref["dW"] + dc.DW0, ref["e_dw"])
        out["dW_plain"] = ratio(dW, ref["dW_plain"] + dc.DW0, ref["e_dw_plain"])
    if db is not None:
        out["db"] = ratio(db, ref["db"] + dc.DB0, ref["e_db"])
    return out


def report(c, out, stage256_on=True):
    ks = {w: dc.key(c, w, int(stage256_on)) for w in ("fwd", "dx", "dw")}
    for name, r in sorted(out.items()):
        k = ks["fwd" if name[0] in "YU" else ("dx" if name.startswith("dX") else "dw")]
        print("RATIO %s %s %.4f %s" % (k[0], name, r, dc.case_id(c)))


def guard(c):
    """The stage kernels are what the F256 / DX256 cases are about: with ADT_STAGE256=0 in this process they would silently test other kernels."""
    if not STAGE256 and (dc.key(c, "fwd")[0] == "F256" or (dc.key(c, "dx") or ("",))[0] == "DX256"):
        pytest.fail("ADT_STAGE256=%s in the environment turns k_dense_fwd256 / k_dense_dx256 off; unset it (test (d) covers that switch in a child process)"
                    % os.environ.get("ADT_STAGE256"))


# ---- (a), (b): parity over the table ------------------------------------------------------------------------------------------------------------------
_SAVED = {}      # the forward's U of the last case, for its backward


PARITY = [(c, d) for c in dc.CASES for d in (("fwd", "bwd") if c.want else ("fwd",))]      # a case's backward right behind its forward


@pytest.mark.parametrize("c,direction", PARITY, ids=["%s-%s" % (d, dc.case_id(c)) for c, d in PARITY])
def test_parity_with_float64(c, direction):
    guard(c)
    if direction == "fwd":
        out, U = check_forward(c, _SAVED)
        report(c, out)
        assert max(out.values()) <= 1.0, out
        return
    U = _SAVED.pop(c) if c in _SAVED else forward(c, dc.make_inputs(c))[1]      # run alone: the forward unjudged
    out = check_backward(c, U)
    report(c, out)
    assert max(out.values()) <= 1.0, out


# ---- (c): the split input gradient and t_dev ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", [dc.F32, dc.BF16])
@pytest.mark.parametrize("K", [64, 256])
def test_split_dx_leaves_the_rows_beyond_t_dev_untouched(prec, K):
    """k_dense_bwd_dx with nt_z > 1 adds its splits with atomics onto a dX that a launch ahead of it cleared; that launch stops at *t_dev like every other
    arm (DenseFwdArgs::t_dev: rows at or beyond it are not computed).  No caller relies on zeros there: BERT4Rec-ADT scatters dhm under the same count."""
    c = dc.case(prec, 40, K, 4100, t_dev=1, mask=1, want="x")
    assert dc.key(c, "dx")[3:] == (True, True)
    out = check_backward(c, None)      # asserts the sentinel beyond t_dev and exact zeros on masked rows
    report(c, out)
    assert max(out.values()) <= 1.0, out


# ---- (d): ADT_STAGE256=0 ---------------------------------------------------------------------------------------------------------------------------------
def stage_off_cases():
    """The K = 256 cases of the table at N = 256, 512, 1024 (forward: 1, 2, 4 full panels of k_dense_fwd_rows<8, .>) and N <= 768 (input gradient:
    k_dense_dx_rows<8, false> / <4, true> at K = 256), one stage: the shapes are small."""
    return [c for c in dc.CASES if c.K == 256 and c.layout == "aligned" and c.T <= 300 and c.N in (256, 512, 768, 1024) and c.prec == dc.BF16]


def child_main():
    assert not STAGE256, "the child runs with ADT_STAGE256=0"
    worst, n = 0.0, 0
    for c in stage_off_cases():
        assert dc.key(c, "fwd", 0)[0] == "FROWS" and (dc.key(c, "dx", 0) or ("DXROWS",))[0] == "DXROWS", c
        out, U = check_forward(c)
        if "x" in c.want:
            out.update(check_backward(c._replace(want="x"), U))
        report(c, out, False)
        worst, n = max(worst, max(out.values())), n + 1
    print("CHILD cases %d max_ratio %.4f" % (n, worst))
    return 0


def test_stage_kernels_switched_off_in_a_child_process():
    cases = stage_off_cases()
    assert {c.N for c in cases} == {256, 512, 768, 1024} and len(cases) >= 16
    assert {dc.key(c, "fwd", 0)[:2] for c in cases} == {("FROWS", 8)} and {dc.key(c, "fwd", 0)[3:] for c in cases} == {(False, False), (True, False)}
    env = dict(os.environ, ADT_STAGE256="0")
    r = subprocess.run(["timeout", "-k", "10", "120", sys.executable, os.path.abspath(__file__), "--stage256-off"], env=env, capture_output=True, text=True, cwd=REPO)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    last = [line for line in r.stdout.splitlines() if line.startswith("CHILD")]
    assert len(last) == 1, r.stdout[-2000:]
    n, worst = int(last[0].split()[2]), float(last[0].split()[4])
    print(last[0])
    assert n == len(cases) and worst <= 1.0


# ---- (e): independence of the workgroups and leaks, bit for bit -------------------------------------------------------------------------------------------
def test_fwd256_rows_of_one_workgroup_stay_in_it():
    """k_dense_fwd256 at T = 8232, N = 768: 129 workgroups of two stages (chunk 64).  New X rows for workgroup j = 57 change rows 64 j .. 64 j + 63 of Y and U
    and no bit of any other row: a stage that read the other buffer's rows, or kept the first stage's registers, would show."""
    guard(dc.case(dc.BF16, 8232, 256, 768, want=""))
    c = dc.case(dc.BF16, 8232, 256, 768, act=dc.ACT_GELU, p=dc.P_DROP, R=1, mask=1, want="")
    assert dc.key(c, "fwd") == ("F256", 7, 3, True)
    inp = dc.make_inputs(c)
    Y0, U0 = forward(c, inp)
    j = 57
    rows = slice(64 * j, 64 * j + 64)
    inp["X"][rows] = np.random.RandomState(1).standard_normal((64, c.K)).astype(np.float32) * 3
    inp["ids"][rows] = 1
    Y1, U1 = forward(c, inp)
    for a, b in ((Y0.view, Y1.view), (U0.view, U1.view)):
        same = (a == b).all(1).cpu().numpy()
        assert same[:64 * j].all() and same[64 * j + 64:].all() and not same[rows].any()
    assert torch.equal(torch.cat([Y0.view[:64 * j], Y0.view[64 * j + 64:]]), torch.cat([Y1.view[:64 * j], Y1.view[64 * j + 64:]]))


def test_dx256_rows_of_one_workgroup_stay_in_it():
    """k_dense_dx256<3> at T = 8232: the same for dY and dX (beta: the old rows are read per stage)."""
    guard(dc.case(dc.BF16, 8232, 256, 768, want="x"))
    c = dc.case(dc.BF16, 8232, 256, 768, act=dc.ACT_ELU, p=dc.P_DROP, beta=1, want="x")
    assert dc.key(c, "dx") == ("DX256", 3, True)
    inp = dc.make_inputs(c)
    _, U = forward(c, inp)
    g0 = backward(c, inp, U)[0].view
    j = 100
    rows = slice(64 * j, 64 * j + 64)
    inp["dY"][rows] = np.random.RandomState(2).standard_normal((64, c.N)).astype(np.float32) * 3
    g1 = backward(c, inp, U)[0].view
    same = (g0 == g1).all(1).cpu().numpy()
    assert same[:64 * j].all() and same[64 * j + 64:].all() and not same[rows].any()


@pytest.mark.parametrize("K,N,T", [(256, 256, 8232), (512, 512, 2088), (64, 64, 16500)])
def test_masked_rows_leak_nothing_into_dw_and_db(K, N, T):
    """k_dense_dw256 (129 workgroups of three stages, per = 32; 512 x 512: four blocks, n0 and k0 both non-zero) and k_dense_dw64 (129 partials: two
    passes of the reduce): whatever dY holds on masked rows, dW and db do not change in any bit.  The partial sums are added in no fixed order
    (atomics), so the inputs are small integers -- X in -4 .. 4, dY in -2 .. 2, dropout at p = 0.5 (scale 2) -- and every sum is exact in fp32
    (at most 16,500 x 16 < 2^24): the order cannot show, and dW and db also equal the integer reference exactly."""
    c = dc.case(dc.BF16, T, K, N, p=0.5, mask=1, t_dev=1, want="wb", bias=0)
    assert dc.key(c, "dw")[0] == ("DW64" if K == 64 else "DW256")
    inp = dc.make_inputs(c)
    r = np.random.RandomState(T)
    inp["X"] = r.randint(-4, 5, size=(T, K)).astype(np.float32)
    inp["dY"] = r.randint(-2, 3, size=(T, N)).astype(np.float32)
    live = inp["live"]
    keep, scale = dc.drop_scale(c)
    assert float(scale) == 2.0
    G = np.where(keep, inp["dY"] * 2.0, 0.0) * (inp["ids"] != 0)[:, None]
    G[live:] = 0
    want_dw, want_db = G.T.astype(np.float64) @ inp["X"].astype(np.float64), G.sum(0)
    assert np.abs(want_dw).max() < 2 ** 24 and np.abs(want_dw).max() > 100
    base = backward(c, inp, None)
    assert np.array_equal(base[1], (want_dw + dc.DW0).astype(np.float32)) and np.array_equal(base[2], (want_db + dc.DB0).astype(np.float32))
    inp["dY"][inp["ids"] == 0] = 0.0
    quiet = backward(c, inp, None)
    assert np.array_equal(base[1].view(np.uint32), quiet[1].view(np.uint32)) and np.array_equal(base[2].view(np.uint32), quiet[2].view(np.uint32))
    inp["dY"][inp["ids"] == 0] = 1000.0      # and loud
    loud = backward(c, inp, None)
    assert np.array_equal(base[1].view(np.uint32), loud[1].view(np.uint32)) and np.array_equal(base[2].view(np.uint32), loud[2].view(np.uint32))


if __name__ == "__main__":
    sys.path.insert(0, REPO)
    assert sys.argv[1:] == ["--stage256-off"], sys.argv
    sys.exit(child_main())
