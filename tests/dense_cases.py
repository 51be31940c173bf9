"""Shared by test_dense_cases_cpu.py and test_dense_arms_hip.py: the case table of the dense layers of the wide C ABI (adt_dense_fwd, adt_dense_bwd;
adt_amd/csrc/adt_gemm.cuh, adt_dense_rows.cuh, dispatched by adt_wide_plan.h and launched from adt_wide.hip), the inputs of a case, the float64
reference and the bounds the GPU tests hold the kernels to.

A case is a Case tuple: prec, T, K, N, act, save_u, p; bias, R, R2, mask, t_dev (present or not); beta; want (a subset of "xwb": dX, dW, db);
layout ("aligned", or one operand of Y, U, R, R2, bias, dX made non-vectorisable: "+ld" an odd row stride, "+off" a base one float into a
larger buffer); ws ("registered" | "none": the workspace of the weight gradient).  facts() turns a case into the DenseFacts that dense_fwd_facts /
dense_bwd_facts of adt_wide.hip compute for it, key() names the kernel instantiation and loop regime it therefore gets (through the plan's
restatement in test_wide_plan_cpu.py).  Instead of a cross product, the epilogue features rotate over the shapes of one key (_rotate);
test_dense_cases_cpu.py proves that every key the plan can choose is hit and still sees every feature that can reach it.

The reference (ref64) is float64 throughout.  In bf16 mode it is computed from the operands rounded as the kernels round them (bf16_round: X and
W always; G after it was formed in fp32 -- dY * scale reproduced in float32, the activation's derivative in float64) and, for the values only,
from the unrounded operands.

Bounds (elementwise; u = 2^-24, the unit roundoff of fp32).  Against the rounded-operand reference -- and in exact-fp32 mode, whose operands are
not rounded -- the products are exact (8 x 8 significant bits in bf16; in fp32 mode they round once, u of each, counted below) and only the fp32
sums and the fp32 epilogue separate kernel and reference.
  * A sum of fp32 terms in which no term passes through more than D additions is off by at most D ulp-sized steps of the sum of the absolute
    terms.  The ISA does not promise round-to-nearest for the additions inside an MFMA, so a step is a whole unit in the last place, 2 u:
    |sum - exact| <= 2 D u * mag, mag the magnitude array (|X| |W|^T, |G| |W|, |G|^T |X|, sum |G|), plus |old| where the kernel accumulates into a
    buffer.  (fp32 mode: + 1 to D for the rounding of the products.)
  * D is the contraction length plus the partial sums that are added afterwards.  Forward: K + 1 (the bias).  dX: N + 33 (at most 16 row-streaming
    pieces or 32 splits, and the old value under beta).  dW and db contract over T, but no kernel adds T terms in a row: a workgroup sums its
    chunk of rows and the chunks' partial sums are added afterwards (the reduce kernels, or atomics, in any order), so D = chunk + number of
    chunks + 1 (the old value), both read from the plan.  With D = T the bound at T = 8232 would be thirty times looser and a dropped 32-row
    stage (about 2^-8 of mag) would pass.
  * Forward epilogue, on top of e_v = 2 (K + 1) u mag + u |v| for v = acc + bias: the activation is 1.13-Lipschitz at most (GELU) and the fp32
    erff / expf behind it are good to a few ulp of their result, which the cancellations in 0.5 v (1 + erf) and exp(v) - 1 turn into
    8 u (|a| + |v| + 1) at most: e_a = 1.13 e_v + 8 u (|a| + |v| + 1), nothing but e_v without an activation.  Dropout multiplies by the fp32 scale
    (one rounding), the residuals are added as fl(fl(R + R2) + .) (two): e_y = scale e_a + u (|d| + |R + R2| + |y|).  U is v: e_v.
  * Backward, G = dY * mask * keep * scale * act'(U): without an activation G is the float32 product dY * scale, which the reference reproduces
    bit for bit, so the rounded operand is the same.  With one, the kernel's fp32 act' and the reference's float64 act' differ in the last bits
    and can move a G across a bf16 rounding boundary: one bf16 ulp of that element.  The allowance is 2^-8 |G| |W| (dX), 2^-8 |G|^T |X| (dW) --
    every element moved by half its largest possible ulp, where only a handful can move at all -- and 2^-8 sum |G| for a db summed from the
    rounded tile (the tiled kernel); in fp32 mode and for the db that the other kernels sum before rounding it is 16 u of the same magnitude
    (act' good to a few ulp, two products).  The reference takes act' at the U the kernel's forward saved: a ReLU gate decided by the last
    bit of U is then the same on both sides.
  * Against the unrounded reference every operand is off by half a unit of its 8 significant bits, 2^-8 of itself at most, a product by less than
    1.01 * 2^-7: that much of mag more.
A dropped or masked element, a row at or beyond t_dev and the padding of a strided output are not bounded but exact: fl(R + R2) or 0.0, and the
sentinel the buffer was filled with.
"""
import zlib
from collections import namedtuple

import numpy as np

from test_wide_plan_cpu import BF16, F32, FACT_FIELDS, WS, expect_dw, expect_dx, expect_fwd

ACT_NONE, ACT_RELU, ACT_GELU, ACT_ELU, ACT_ELU1 = 0, 1, 2, 3, 4
SEED, SITE, ROW_OFF = 12345, 7, 11
P_DROP = 0.3
U32 = 2.0 ** -24
DW0, DB0 = 0.25, -0.5          # what dW and db hold before the call
SENTINEL = -7.25               # what Y, U and dX hold before the call

Case = namedtuple("Case", "prec T K N act save_u p bias R R2 mask t_dev beta want layout ws")
LAYOUTS = ("aligned", "Y+ld", "Y+off", "U+ld", "U+off", "R+ld", "R+off", "R2+ld", "R2+off", "bias+off", "dX+ld", "dX+off")


def case(prec, T, K, N, act=ACT_NONE, save_u=None, p=0.0, bias=1, R=0, R2=0, mask=0, t_dev=0, beta=0, want="xwb", layout="aligned", ws="registered"):
    """save_u defaults to "an activation is there" (what the models do)."""
    c = Case(prec, T, K, N, act, int(act != ACT_NONE if save_u is None else save_u), float(p), int(bias), int(R), int(R2), int(mask), int(t_dev), int(beta), want,
             layout, ws)
    assert layout in LAYOUTS and ws in ("registered", "none") and set(want) <= set("xwb") and ("b" not in want or "w" in want) and K % 4 == 0, c
    assert not (act != ACT_NONE and want and not c.save_u), "the backward of an activation needs the saved U"
    op = layout.split("+")[0]
    assert op == "aligned" or {"Y": 1, "U": c.save_u, "R": c.R, "R2": c.R2, "bias": c.bias, "dX": "x" in want}[op], "the tagged operand is absent: %r" % (c,)
    return c


def case_id(c):
    feats = "".join(s for s, on in (("b", c.bias), ("R", c.R), ("Q", c.R2), ("m", c.mask), ("t", c.t_dev), ("B", c.beta)) if on)
    return "%s-%dx%dx%d-a%d%s-p%g-%s-%s-%s%s" % ("bf16" if c.prec else "f32", c.T, c.K, c.N, c.act, "u" if c.save_u else "", c.p, feats or "0", c.want or "fwd",
                                                  c.layout, "" if c.ws == "registered" else "-nows")


def round4(n):
    return (n + 3) // 4 * 4


def ld_of(c, op):
    """Row stride of an operand as the GPU test lays it out: contiguous, or, tagged, the smallest wider stride that is odd modulo 4 ("+ld") or a
    multiple of 4 with four spare columns ("+off": the base is one float into the buffer).  dY is always padded to a multiple of 4 (the C ABI demands it)."""
    n = c.K if op == "dX" else c.N
    if op == "dY":
        return round4(n)
    if c.layout == op + "+ld":
        return n + 1 if (n + 1) % 4 else n + 2
    if c.layout == op + "+off":
        return round4(n) + 4
    return n


def operand_ok(c, op):
    """operand_ok of adt_wide.hip: a 16-byte aligned base and ld % 4 == 0."""
    return int(c.layout != op + "+off" and ld_of(c, op) % 4 == 0)


def has_drop(c):
    return int(int(c.p * 256.0 + 0.5) > 0)


def facts(c, direction, stage256_on=1):
    """The DenseFacts of a case, in the field order of FACT_FIELDS: what dense_fwd_facts ("fwd") / dense_bwd_facts ("bwd") of adt_wide.hip compute.
    An absent operand counts as aligned (operand_ok(NULL, 0)); the plan reads the *_ok of present operands only."""
    f = dict.fromkeys(FACT_FIELDS, 0)
    f.update(prec=c.prec, T=c.T, K=c.K, N=c.N, x_ok=1, w_ok=1, bias_ok=1, u_ok=1, r_ok=1, r2_ok=1, dx_ok=1, rows_on=1, stage256_on=int(stage256_on),
             ws_bytes=WS if c.ws == "registered" else 0, has_u=c.save_u, has_mask=c.mask, has_drop=has_drop(c), has_act=int(c.act != ACT_NONE))
    if c.save_u:
        f["u_ok"] = operand_ok(c, "U")
    if direction == "fwd":
        f.update(has_bias=c.bias, has_r=c.R, has_r2=c.R2, g_ok=operand_ok(c, "Y"), bias_ok=int(not (c.bias and c.layout == "bias+off")))
        if c.R:
            f["r_ok"] = operand_ok(c, "R")
        if c.R2:
            f["r2_ok"] = operand_ok(c, "R2")
    else:
        assert direction == "bwd", direction
        f.update(has_dx=int("x" in c.want), has_dw=int("w" in c.want), beta=c.beta, g_ok=1)
        if "x" in c.want:
            f["dx_ok"] = operand_ok(c, "dX")
    assert list(f) == list(FACT_FIELDS)
    return f


def key_fwd(f):
    e = expect_fwd(f)
    if e[0] == "F256":
        return ("F256", e[6], f["N"] // 256, e[5] > 32)
    if e[0] == "FROWS":
        return ("FROWS", e[10], e[11], e[8] > 1, e[7] < 256)
    return ("FTILED", f["prec"], e[12])


def key_dx(f):
    e = expect_dx(f)
    if e[0] == "DX256":
        return ("DX256", e[5], e[6] > 32)
    if e[0] == "DXROWS":
        pieces = [tuple(int(v) for v in p.split(":")) for p in e[11].split(",")]
        return ("DXROWS", frozenset((p[3], bool(e[10])) for p in pieces), len(pieces) > 1, bool(f["beta"]))
    return None if e[0] == "DXNONE" else ("DXTILED", f["prec"], e[12], e[15] > 1, bool(e[17]))


def key_dw(f):
    e = expect_dw(f)
    if e[0] == "DW256":
        return ("DW256", e[7], e[8], e[9], e[5] > 32, e[6] % e[9] != 0)
    if e[0] == "DWROWS":
        return ("DWROWS", e[14] > 1, e[15] > 1)
    if e[0] == "DW64":
        return ("DW64", e[7], e[8], bool(e[12]), e[6] > 128)
    return None if e[0] == "DWNONE" else ("DWTILED", f["prec"], e[16])


def key(c, which, stage256_on=1):
    """The instantiation and loop regime of one third of a case: which = "fwd" | "dx" | "dw".  None when the case does not ask for that output."""
    if which == "fwd":
        return key_fwd(facts(c, "fwd", stage256_on))
    return (key_dx if which == "dx" else key_dw)(facts(c, "bwd", stage256_on))


def keys(c):
    return [k for k in (key(c, w) for w in ("fwd", "dx", "dw")) if k is not None]


def rows_live(c):
    """t_dev: a few dozen rows short of T."""
    return c.T - min(37, c.T // 3) if c.t_dev else c.T


def dw_depth(c):
    """chunk + number of chunks + 1 of the weight gradient's plan (the module docstring: D of dW and db), and whether db is summed from the rounded tile."""
    e = expect_dw(facts(c, "bwd"))
    chunk = e[5]
    if e[0] == "DWNONE":
        return 0, False
    return chunk + (c.T + chunk - 1) // chunk + 1, e[0] == "DWTILED"


# ---- numbers ------------------------------------------------------------------------------------------------------------------------------------
def bf16_round(x):
    """float32 -> the nearest value with 8 significant bits, ties to even, on the bit pattern: what (__bf16)x compiles to (v_cvt_pk_bf16_f32) in
    tile_commit, rows_pack and the staging code of the stage kernels.  Finite inputs."""
    b = np.ascontiguousarray(x, np.float32).view(np.uint32)
    b = (b + (np.uint32(0x7FFF) + ((b >> np.uint32(16)) & np.uint32(1)))) & np.uint32(0xFFFF0000)
    return b.view(np.float32)


def act64(act, v):
    from scipy.special import erf
    if act == ACT_RELU:
        return np.maximum(v, 0.0)
    if act == ACT_GELU:
        return 0.5 * v * (1.0 + erf(v * 0.7071067811865476))
    if act in (ACT_ELU, ACT_ELU1):
        return np.where(v > 0, v, np.expm1(np.minimum(v, 0.0))) + (1.0 if act == ACT_ELU1 else 0.0)
    return v


def act_grad64(act, v):
    from scipy.special import erf
    if act == ACT_RELU:
        return (v > 0).astype(np.float64)
    if act == ACT_GELU:
        return 0.5 * (1.0 + erf(v * 0.7071067811865476)) + v * 0.3989422804014327 * np.exp(-0.5 * v * v)
    if act in (ACT_ELU, ACT_ELU1):
        return np.where(v > 0, 1.0, np.exp(np.minimum(v, 0.0)))
    return np.ones_like(v)


def make_inputs(c):
    """Seeded per case, float32: X (T, K), W (N, K) of 1 / sqrt(K), b of 0.1, R, R2, dY (T, N), ids (T,) with about a fifth zero, dX0 (T, K) the
    old input gradient under beta, live = the device row count."""
    r = np.random.default_rng(zlib.crc32(repr(tuple(c)).encode()))

    def normal(shape, on=True):
        return r.standard_normal(shape, dtype=np.float32) if on else None
    return dict(X=normal((c.T, c.K)), W=normal((c.N, c.K)) / np.float32(np.sqrt(c.K)), b=np.float32(0.1) * normal(c.N) if c.bias else None, R=normal((c.T, c.N), c.R),
                R2=normal((c.T, c.N), c.R2), dY=normal((c.T, c.N), bool(c.want)), ids=(r.random(c.T) > 0.2).astype(np.int32) if c.mask else None,
                dX0=normal((c.T, c.K), c.beta), live=rows_live(c))


def drop_scale(c):
    """(keep (T, N) bool, the fp32 scale 1 / (1 - thr / 256)) or (None, 1)."""
    from oracle import rng
    if not has_drop(c):
        return None, np.float32(1.0)
    idx = (np.arange(c.T, dtype=np.int64)[:, None] + ROW_OFF) * c.N + np.arange(c.N, dtype=np.int64)[None, :]
    return rng.keep_mask(SEED, SITE, idx, c.p), np.float32(1.0 / (1.0 - rng.drop_prob(c.p)))


def _operands(c, x, rounded):
    return bf16_round(x).astype(np.float64) if (rounded and c.prec == BF16) else x.astype(np.float64)


def ref_fwd(c, inp=None):
    """Forward half of ref64: Y, U (pre-activation, every row), their bounds e_y, e_v against the rounded-operand reference, and Y_plain / e_plain:
    the same from the unrounded operands (bf16 mode; equal to Y / e_y in fp32 mode).  Rows at or beyond inp["live"] are not part of the contract."""
    inp = inp or make_inputs(c)
    keep, scale = drop_scale(c)
    s64 = float(scale)
    out = {}
    for rounded in (True, False):
        X, W = _operands(c, inp["X"], rounded), _operands(c, inp["W"], rounded)
        v = X @ W.T + (inp["b"].astype(np.float64) if c.bias else 0.0)
        a = act64(c.act, v)
        d = a * s64 * keep if keep is not None else a
        res = (inp["R"].astype(np.float64) if c.R else 0.0) + (inp["R2"].astype(np.float64) if c.R2 else 0.0)
        y = d + res
        if c.mask:
            y = y * (inp["ids"] != 0)[:, None]
        if rounded:
            mag = np.abs(X) @ np.abs(W.T) + (np.abs(inp["b"]).astype(np.float64) if c.bias else 0.0)
            D = c.K + 1 + (1 if c.prec == F32 else 0)
            e_v = 2 * D * U32 * mag + U32 * np.abs(v)
            e_a = 1.13 * e_v + 8 * U32 * (np.abs(a) + np.abs(v) + 1.0) if c.act != ACT_NONE else e_v
            e_y = s64 * e_a + U32 * (np.abs(d) + np.abs(res) + np.abs(y))
            out.update(Y=y, U=v, e_y=e_y, e_v=e_v, mag_y=mag)
        else:
            out.update(Y_plain=y, e_plain=out["e_y"] + (1.01 * 2.0 ** -7 * 1.13 * s64 * out["mag_y"] if c.prec == BF16 else 0.0))
        if c.prec == F32:
            out.update(Y_plain=out["Y"], e_plain=out["e_y"])
            break
    # what a dropped or masked element must be, exactly: fl(R + R2), 0.0 under the mask
    exact = np.zeros((c.T, c.N), bool)
    if keep is not None:
        exact |= ~keep
    if c.mask:
        exact |= (inp["ids"] == 0)[:, None]
    res32 = (inp["R"] if c.R else np.float32(0)) + (inp["R2"] if c.R2 else np.float32(0)) + np.zeros((c.T, c.N), np.float32)
    if c.mask:
        res32 = res32 * (inp["ids"] != 0)[:, None].astype(np.float32)
    out.update(exact=exact, exact_value=res32.astype(np.float32))
    return out


def grad_source(c, inp, U, rounded):
    """G = dY * mask * keep * scale * act'(U) on the live rows, zero beyond them: the float32 product dY * scale as the kernels form it, act' in float64
    at the given U; rounded to bf16 afterwards where asked."""
    keep, scale = drop_scale(c)
    g = inp["dY"].copy()
    if keep is not None:
        g = np.where(keep, g * scale, np.float32(0)).astype(np.float32)      # float32 x float32, as GradSrc::at
    g = g.astype(np.float64)
    if c.act != ACT_NONE:
        g = g * act_grad64(c.act, np.asarray(U, np.float64))
    if c.mask:
        g = g * (inp["ids"] != 0)[:, None]
    g[inp["live"]:] = 0.0
    if rounded and c.prec == BF16:
        g = bf16_round(g.astype(np.float32)).astype(np.float64)
    return g


def ref_bwd(c, inp=None, U=None):
    """Backward half of ref64 at the saved pre-activation U (default: the reference's own, as float32): dX (T, K; the old value included under beta),
    dW (N, K), db (N,) -- increments, the caller adds what the buffers held -- with their bounds e_dx, e_dw, e_db, the *_plain values from unrounded
    operands with e_*_plain, and zero_rows: the live rows whose dX is exactly the old value (or 0.0)."""
    inp = inp or make_inputs(c)
    if U is None and c.act != ACT_NONE:
        U = ref_fwd(c, inp)["U"].astype(np.float32)
    live = inp["live"]
    depth, db_rounded = dw_depth(c)
    slack = (2.0 ** -8 if c.prec == BF16 else 16 * U32) if c.act != ACT_NONE else 0.0      # one bf16 ulp of G | the fp32 act'
    f32 = 1 if c.prec == F32 else 0
    out = {}
    G_plain = grad_source(c, inp, U, False)
    for rounded in (True, False):
        G = bf16_round(G_plain.astype(np.float32)).astype(np.float64) if (rounded and c.prec == BF16) else G_plain
        X, W = _operands(c, inp["X"], rounded), _operands(c, inp["W"], rounded)
        sfx = "" if rounded else "_plain"
        extra = 0.0 if rounded else 1.01 * 2.0 ** -7
        if "x" in c.want:
            old = inp["dX0"].astype(np.float64) if c.beta else 0.0
            mag = np.abs(G) @ np.abs(W)
            out["dX" + sfx] = G @ W + old
            out["e_dx" + sfx] = (2 * (c.N + 33 + f32) * U32 + slack + extra) * mag + 2 * (c.N + 33) * U32 * np.abs(old) + U32 * np.abs(out["dX" + sfx])
        if "w" in c.want:
            mag = np.abs(G[:live]).T @ np.abs(X[:live])
            out["dW" + sfx] = G[:live].T @ X[:live]
            out["e_dw" + sfx] = (2 * (depth + f32) * U32 + slack + extra) * mag + 2 * depth * U32 * DW0 + U32 * np.abs(out["dW" + sfx] + DW0)
        if "b" in c.want:
            Gb = G if (rounded and db_rounded) else G_plain      # the tiled kernel sums the tile it rounded, the others the fp32 values
            mag = np.abs(Gb).sum(0)
            out["db" + sfx] = Gb.sum(0)
            sl = slack if (db_rounded and c.prec == BF16) or c.act == ACT_NONE else 16 * U32
            out["e_db" + sfx] = (2 * depth * U32 + sl + (extra if db_rounded else 0.0)) * mag + 2 * depth * U32 * abs(DB0) + U32 * np.abs(out["db" + sfx] + DB0)
        if c.prec == F32:
            for name in ("dX", "dW", "db"):
                if name in out:
                    out[name + "_plain"], out["e_" + name.lower() + "_plain"] = out[name], out["e_" + name.lower()]
            break
    zero = np.zeros(c.T, bool)
    if c.mask:
        zero[:live] = inp["ids"][:live] == 0
    out["zero_rows"] = zero
    return out


def ref64(c, U=None):
    """Y, U, dX, dW, db of a case in float64 with the magnitude-scaled bounds of the module docstring (ref_fwd and ref_bwd in one dictionary)."""
    inp = make_inputs(c)
    out = ref_fwd(c, inp)
    if c.want:
        out.update(ref_bwd(c, inp, out["U"].astype(np.float32) if U is None else U))
    return out


def tape_oracle(c, inp):
    """The float32 tape of oracle/tape.py, as test_wide_kernels.test_dense_forward_backward builds it, extended with the second residual and the
    row mask: (Y, dX, dW, db).  No t_dev, no beta."""
    from oracle import tape as tp
    acts = {0: lambda v: v, 1: tp.relu, 2: tp.gelu, 3: tp.elu, 4: lambda v: tp.elu(v, True)}
    vx, vw, vb = tp.leaf(inp["X"]), tp.leaf(inp["W"]), tp.leaf(inp["b"] if c.bias else np.zeros(c.N, np.float32))
    y = acts[c.act](tp.linear(vx, vw, vb))
    y = tp.dropout(y, c.p, SEED, SITE, tp.idx_rows(c.T, c.N, ROW_OFF))
    if c.R:
        y = tp.add(y, tp.const(inp["R"]))
    if c.R2:
        y = tp.add(y, tp.const(inp["R2"]))
    if c.mask:
        y = tp.mul_mask(y, np.broadcast_to((inp["ids"] != 0)[:, None], (c.T, c.N)))
    tp.backward(y, inp["dY"])
    return y.v, vx.g, vw.g, vb.g


# ---- the table ------------------------------------------------------------------------------------------------------------------------------------
T_REGIMES = (40, 300, 2088, 4136, 8232, 16500)
K_SET = (64, 100, 128, 256, 512, 1024)
N_SET = (36, 64, 100, 128, 256, 260, 448, 512, 768, 1024, 4100)


# the rotation: (act, save_u alone, p, R, R2, mask, t_dev, beta, bias).  Every activation, "saved U without an activation", and each flag on and off
# against the others; a group of shapes walks through it from its own starting point.
FEATS = ((ACT_NONE, 0, 0.0, 0, 0, 0, 0, 0, 1), (ACT_GELU, 0, P_DROP, 1, 0, 1, 1, 1, 1), (ACT_NONE, 0, P_DROP, 0, 1, 0, 1, 0, 0), (ACT_RELU, 0, 0.0, 1, 1, 0, 0, 1, 1),
         (ACT_NONE, 0, 0.0, 0, 0, 1, 1, 1, 1), (ACT_ELU, 0, P_DROP, 0, 1, 1, 0, 0, 1), (ACT_NONE, 1, P_DROP, 1, 0, 0, 0, 1, 1), (ACT_ELU1, 0, 0.0, 0, 0, 0, 1, 0, 0),
         (ACT_GELU, 0, 0.0, 0, 1, 0, 0, 0, 1), (ACT_NONE, 0, P_DROP, 1, 0, 1, 1, 1, 1), (ACT_RELU, 0, P_DROP, 0, 0, 0, 1, 1, 0))


def _rotate(shapes, start, **fixed):
    """One case per shape (prec, T, K, N); the features advance through FEATS with the shape, from `start`.  fixed: what the group's key pins
    (R2 for the CH = 4 build of the row-streaming forward, the workspace, what is wanted)."""
    out = []
    for i, shape in enumerate(shapes):
        act, su, p, R, R2, mask, t_dev, beta, bias = FEATS[(start + i) % len(FEATS)]
        kw = dict(act=act, p=p, R=R, R2=R2, mask=mask, t_dev=t_dev, beta=beta, bias=bias)
        kw.update(fixed)
        kw.setdefault("save_u", int(su or kw["act"] != ACT_NONE))
        out.append(case(*shape, **kw))
    return out


def _f256(N, T, epi, i, want, beta=0, ws="registered"):
    """The k_dense_fwd256<epi> case of a (T, 256, N) layer: bit 0 rotates over R | the row mask | R2 | all three, bit 2 over the four activations and,
    once per N, the saved U alone."""
    R, R2, mask = ((1, 0, 0), (0, 0, 1), (0, 1, 0), (1, 1, 1))[i % 4] if epi & 1 else (0, 0, 0)
    act = (ACT_GELU, ACT_RELU, ACT_ELU, ACT_ELU1)[i % 4] if epi & 4 else ACT_NONE
    if epi == 4 and i % 2 == 0:
        act = ACT_NONE
    return case(BF16, T, 256, N, act=act, save_u=int(bool(epi & 4)), p=P_DROP if epi & 2 else 0.0, R=R, R2=R2, mask=mask, t_dev=(i + epi) % 2, beta=beta, bias=(i + epi) % 3 != 0,
                want=want, ws=ws)


# what the backward of the eight epilogues of one N asks for: dX with and without beta, with and without an activation (epi & 4); dW and db
WANT_TWO_STAGE = (("xwb", 0), ("x", 1), ("", 0), ("wb", 0), ("x", 0), ("xwb", 0), ("", 0), ("x", 1))


def _table():
    cases = []
    # k_dense_fwd256, two stages with a ragged second one (chunk 64, 40 rows in the last workgroup), all eight epilogues at every N; their backward is
    # k_dense_dx256<NB> in two stages (N <= 768), three-piece row streaming (N = 1024), and k_dense_dw256 in two stages with per = 32 (N = 256: 129
    # workgroups, five reduce groups, a lone partial in the last) and per = 16
    for n, (N, T) in enumerate(((256, 8232), (512, 8232), (768, 8232), (1024, 4136))):
        cases += [_f256(N, T, epi, n + epi, *WANT_TWO_STAGE[epi]) for epi in range(8)]
    # ... one stage; T = 4136 at N = 256: 130 workgroups of one stage, per = 32.  One 256 x 256 layer without a workspace: the tiled weight gradient
    for n, N in enumerate((256, 512, 768, 1024)):
        for epi in range(8):
            T = 4136 if (N == 256 and epi in (0, 5)) else (40, 300)[(epi + n) % 2]
            cases.append(_f256(N, T, epi, n + epi + 1, "xwb", beta=(epi + n) % 2, ws="none" if (N, epi) == (256, 3) else "registered"))
    # k_dense_dw64: the six block layouts x partials | atomics x one | two passes of the reduce (T = 16,500: 129 partials); their forwards are
    # k_dense_fwd_rows<2 | 4 | 8, 4 | 8> on one panel (pc < 256 at N = 64, 128), their input gradients k_dense_dx_rows<2 | 4 | 8, has_u> in one piece or two
    for n, (N, K) in enumerate(((64, 64), (128, 64), (64, 128), (256, 64), (64, 256), (128, 128))):
        shapes = [(BF16, T, K, N) for T in (300, 16500, 428, 16500)]
        ws = ("registered", "registered", "none", "none")
        for j, (shape, w) in enumerate(zip(shapes, ws)):
            fixed = dict(ws=w)
            if N == 256:      # the four cases of the one-piece k_dense_dx_rows<8, false> / two-piece <4, true>: beta both ways under each
                fixed.update(beta=j % 2, act=(ACT_NONE, ACT_NONE, ACT_GELU, ACT_ELU)[j], save_u=int(j >= 2))
            cases += _rotate([shape], 3 * n + 5 * j, **fixed)
    # k_dense_dw256 at two blocks along K (256 x 512), along both (512 x 512: n0 and k0 both non-zero) and four along K (256 x 1024), one and two stages;
    # the tiled bf16 forward at BN = 128, row-streaming input gradients at K = 512 and 1024
    cases += _rotate([(BF16, T, K, N) for (N, K) in ((256, 512), (512, 512), (256, 1024)) for T in (300, 4136 if K == 512 and N == 256 else 2088)], 1)
    # without a workspace 256 x 1024 goes to k_dense_dw_rows (one block along N, eight along K)
    cases += _rotate([(BF16, 300, 1024, 256)], 4, ws="none")
    # the split input gradient: 26 splits of N = 4100, zero fill or beta, BN = 64 (K = 64) and 128 (K = 256: two K tiles), both precisions; forward:
    # 17 panels of k_dense_fwd_rows<2 | 8, .>, the last one ragged; weight gradient: k_dense_dw_rows with a ragged last block along N
    for prec in (F32, BF16):
        cases += _rotate([(prec, 40, 64, 4100), (prec, 40, 256, 4100)], 2 + prec, beta=0) + _rotate([(prec, 40, 64, 4100), (prec, 40, 256, 4100)], 5 + prec, beta=1)
    # N = 448 = 256 + 128 + 64: three pieces of k_dense_dx_rows<8 | 4 | 2, false>, four of <4 | 2, true>, each with and without beta; two panels of
    # k_dense_fwd_rows<2 | 4 | 8, .> (the last ragged: 192 columns)
    cases += [case(BF16, 300, 128, 448, R2=1, mask=1, t_dev=1, p=P_DROP), case(BF16, 300, 128, 448, act=ACT_GELU, R=1, bias=0),
              case(BF16, 300, 64, 448, beta=1, R=1, R2=1, save_u=1), case(BF16, 300, 256, 448, act=ACT_RELU, beta=1, mask=1, t_dev=1, p=P_DROP, R2=1)]
    # N = 260: a last panel of four columns, the tiled input gradient; k_dense_dw_rows with a ragged block along N (260), along K (100)
    cases += _rotate([(BF16, 300, 256, 260), (BF16, 300, 100, 1024)], 6)
    # a single ragged panel (pc = 48, 112); the tiled arms at a K that is no multiple of 32 and a T that is no multiple of 128, <PREC, 64 | 128>
    cases += [case(BF16, 300, 64, 36, act=ACT_ELU1, p=P_DROP, mask=1, t_dev=1, beta=1), case(BF16, 300, 256, 100, R=1, R2=1, t_dev=1, bias=0),
              case(BF16, 300, 100, 64, R=1, R2=1, mask=1, t_dev=1), case(F32, 300, 100, 64, R=1, p=P_DROP, mask=1, beta=1),
              case(F32, 300, 100, 100, R2=1, t_dev=1, save_u=1)]
    # fallbacks: one operand not vectorisable, on shapes whose aligned twins take k_dense_fwd256 / k_dense_fwd_rows / k_dense_dx_rows
    cases += [case(BF16, 300, 256, 256, layout="Y+ld", act=ACT_GELU, p=P_DROP, R=1, t_dev=1), case(BF16, 300, 256, 256, layout="U+off", act=ACT_ELU, R2=1, mask=1),
              case(BF16, 300, 256, 512, layout="R+ld", R=1, R2=1, p=P_DROP, beta=1), case(BF16, 300, 256, 256, layout="R2+off", act=ACT_RELU, R2=1, t_dev=1, mask=1),
              case(BF16, 300, 128, 448, layout="Y+off", p=P_DROP, mask=1, save_u=1), case(BF16, 300, 128, 448, layout="U+ld", act=ACT_GELU, p=P_DROP, mask=1, t_dev=1),
              case(BF16, 300, 128, 64, layout="R+off", act=ACT_ELU1, R=1, beta=1), case(BF16, 300, 64, 64, layout="R2+ld", R=1, R2=1, mask=1, t_dev=1, save_u=1),
              case(BF16, 300, 64, 64, layout="bias+off", act=ACT_GELU, p=P_DROP, t_dev=1),
              case(BF16, 300, 128, 256, layout="dX+ld", beta=1, act=ACT_RELU, p=P_DROP, mask=1, R2=1), case(BF16, 300, 128, 256, layout="dX+off", t_dev=1, R=1)]
    # N % 4 != 0: the tiled forward (Y and U rows at odd offsets), the backward under a padded dY (the scalar tails of GradSrc::at and PlainSrc::at)
    cases += [case(BF16, 300, 100, 102, act=ACT_ELU, p=P_DROP, mask=1, t_dev=1, R=1), case(F32, 300, 64, 50, act=ACT_GELU, beta=1, R2=1, mask=1, t_dev=1)]
    return cases


CASES = _table()
