"""Shared by test_seq_layer_cases_cpu.py and test_seq_layer_hip.py: the case table of the four one-layer-per-call entry points of the bf16 SASRec
supernet (adt_seq_enc_layer_fwd / _bwd, adt_seq_dec_layer_fwd / _bwd; include/adt_hip.h), the inputs of a case, its float64 reference and the
bounds the GPU tests hold the kernels to.  No supernet model is involved: one layer's tensors are laid into a flat buffer here.

A case is a Case tuple: kind ("enc" | "dec"), H, L, B, p, b_offset, group.  d is 64.

Reference: oracle/sasrec_oracle.py's encoder_layer / encoder_layer_bwd / decoder_layer / decoder_layer_bwd on float64 inputs, under
so.operands("bf16x64"): every matrix product rounds both operands to bfloat16 and is formed in float64.  The same functions without operand rounding
("plain") give, per compared tensor k, D_k = dist(plain, bf16x64): the size of ONE pass of bf16 operand rounding at this shape and these values.
The rounded run also takes the oracle's bias_as_product option: the kernels form every linear layer's bias gradient as a product of the rounded dY
image with a ones column, i.e. they sum the ROUNDED dY.  Without it the bias gradient of the feed-forward's second layer, which has no matrix
product upstream, would have D_k = 0 exactly while the kernel is 1e-3 away (measured on the MI355X: 1.7e-3 at enc H 1 L 4).
And it takes saved_o_bf16: the kernels form the softmax backward's delta as dO . o from the attention output they saved as bf16.  Without it one
case missed 2 D_k (enc H 2 L 4 with drec: gx 0.0124 at D_k 0.0034 -- the classifier's gradient reaches the QUERY side of padding rows, whose
LayerNorm backward multiplies by 1 / sqrt(eps) = 1e4, so those rows are all of gx, and their dq is the cancelling difference dP - delta).

Bounds.  dist is relative Frobenius for gradients and max-abs over the tensor's max for activations (y, rec).  The kernels round where the bf16x64
reference rounds and once more for the tensors they save or hand over as bf16 (o, h, u, a1, q2, kv2, o2, dO, dq2 / dkv2): at most a second pass of
independent roundings of the same size, so the bound is 2 D_k -- and never more than what test_lean_step_vs_bf16_operand_oracle_cfga_shape holds
for the same comparison: 0.05 for a gradient tensor, 1e-2 for an activation.  A gradient tensor whose norm is under 1e-3 of the case's largest
gradient tensor is measured against that scale instead of its own (a sum that cancels to nearly nothing has no relative error to speak of), in
D_k and in the kernel's error alike.

The ReLU gate.  The feed-forward's ReLU is the one discontinuity of a layer: a pre-activation within rounding distance of zero is "on" in one
evaluation and "off" in another, and in the backward that gate moves a whole element of the upstream gradient -- with a few dozen live rows ONE
such gate is 0.03 of every gradient tensor behind it (measured on the MI355X: enc H 1 L 20, 40 live rows, all of its gradients 0.025 - 0.047 away
at D_k = 0.006 - 0.015).  That is no rounding of the arithmetic, and modelling the kernels' roundings more closely cannot remove it, only move it to
another element.  So the backward is compared at the gates the KERNEL's forward saved (its bf16 u rows, u > 0; so.*_layer_bwd(gate=)), the way
dense_cases.py takes act' at the U the kernel saved -- and the GPU test first holds the saved u itself to the reference's u within the activation
bound, so a gate can differ from the reference's only where u is within that bound of zero.  D_k is not touched by this: it is computed
from the two reference runs alone, each with its own gates, and is the same number on a machine without a GPU.
"""
import zlib
from collections import namedtuple

import numpy as np

from oracle import sasrec_oracle as so

D = 64
SEED = 0x5EED1234
GY_SCALE = 0.75                 # the mixing weight every backward of the table runs with (the reference gets 0.75 * gy)
CAP_GRAD, CAP_ACT, FACTOR = 0.05, 1e-2, 2.0
SMALL = 1e-3

ENC_NAMES = ("attention_layernorm.weight", "attention_layernorm.bias", "attention_layer.in_proj_weight", "attention_layer.in_proj_bias",
             "attention_layer.out_proj.weight", "attention_layer.out_proj.bias", "forward_layernorm.weight", "forward_layernorm.bias",
             "forward_layer.conv1.weight", "forward_layer.conv1.bias", "forward_layer.conv2.weight", "forward_layer.conv2.bias", "sparse.weight", "sparse.bias")
DEC_NAMES = ("layer_norm.weight", "layer_norm.bias", "slf_attn.in_proj_weight", "slf_attn.in_proj_bias", "slf_attn.out_proj.weight", "slf_attn.out_proj.bias",
             "enc_attn.in_proj_weight", "enc_attn.in_proj_bias", "enc_attn.out_proj.weight", "enc_attn.out_proj.bias", "pos_ffn.conv1.weight",
             "pos_ffn.conv1.bias", "pos_ffn.conv2.weight", "pos_ffn.conv2.bias")
ENC_PRE, DEC_PRE = "encoder.encoder_layers.0.", "decoder.decoder_layers.0."
CLS = ("sparse.weight", "sparse.bias")
# the 64 x 64 blocks adt_pack_wimg packs: (tensor, number of blocks)
ENC_BLOCKS = (("attention_layer.in_proj_weight", 3), ("attention_layer.out_proj.weight", 1), ("forward_layer.conv1.weight", 1), ("forward_layer.conv2.weight", 1))
DEC_BLOCKS = (("slf_attn.in_proj_weight", 3), ("enc_attn.in_proj_weight", 3), ("slf_attn.out_proj.weight", 1), ("enc_attn.out_proj.weight", 1),
              ("pos_ffn.conv1.weight", 1), ("pos_ffn.conv2.weight", 1))
PADS = (0, 1, 15, 16, 17, -1, -2)      # pad prefix per sequence; -1: L - 1, -2: L (an all-padding sequence); clipped to L

Case = namedtuple("Case", "kind H L B p b_offset group")


def _table():
    cases = []
    for kind in ("enc", "dec"):
        for H in (1, 2, 4):
            for L in (4, 20, 64, 224 if H < 4 else 192):      # head size 16 is covered up to L 192 (adt_seq_layer_supported); 224 is in the rejection test
                cases.append(Case(kind, H, L, 3, 0.3, 5, "shape"))
            cases.append(Case(kind, H, 20, 3, 0.0, 0, "shape"))
        for B in (3, 20, 40, 70):          # seq_split 8, 4, 2, 1 (adt_step_plan.h: B >= 17, 33, 65)
            cases.append(Case(kind, 2, 12, B, 0.3, 5, "split"))
    return cases


CASES = _table()
CONTRACT = [Case(kind, 2, 20, 3, 0.3, 5, "contract") for kind in ("enc", "dec")]
SHARD = [Case(kind, 2, 20, 6, 0.3, 0, "shard") for kind in ("enc", "dec")]


def case_id(c):
    return "%s-H%d-L%d-B%d-p%g-o%d" % (c.kind, c.H, c.L, c.B, c.p, c.b_offset)


def names(kind):
    return ENC_NAMES if kind == "enc" else DEC_NAMES


def sites(kind):
    return so.enc_sites(3) if kind == "enc" else so.dec_sites(2)


def shapes(kind, H):
    cfg = so.Cfg(1, 4, D, H, 1)
    pre = ENC_PRE if kind == "enc" else DEC_PRE
    table = dict(so.param_shapes(cfg))
    return [(n, table[pre + n]) for n in names(kind)]


def layout(kind, H):
    """{name: (offset, shape)} of one layer in a flat fp32 buffer, every tensor at a 64-float-aligned offset; and the buffer's length."""
    off, out = 0, {}
    for n, shp in shapes(kind, H):
        out[n] = (off, shp)
        off += (int(np.prod(shp)) + 63) // 64 * 64
    return out, off


def block_offsets(kind, H):
    lay, _ = layout(kind, H)
    return [lay[n][0] + j * D * D for n, nb in (ENC_BLOCKS if kind == "enc" else DEC_BLOCKS) for j in range(nb)]


def make_ids(c, r):
    """(B, L) int32.  Sequence 0 has a prefix of 0 or 1, so that every case keeps at least L - 1 live rows (with three live rows a single ReLU
    gate that flips under rounding is a tenth of a gradient tensor, and D_k measures that flip, not the arithmetic); the other sequences walk
    through PADS (clipped to L, duplicates dropped) from a start that depends on the case, so a group of cases sees every prefix.  Live ids
    are non-zero except one interior zero, in the first sequence that has three live positions."""
    h = zlib.crc32(repr(tuple(c)).encode())
    pads = []
    for pad in PADS:
        pad = min(c.L, c.L + 1 + pad if pad < 0 else pad)
        if pad not in pads:
            pads.append(pad)
    ids = r.integers(1, 1000, size=(c.B, c.L)).astype(np.int32)
    interior = False
    for b in range(c.B):
        pad = (h >> 8) % 2 if b == 0 else pads[(h + b) % len(pads)]
        ids[b, :pad] = 0
        if not interior and c.L - pad >= 3:
            ids[b, pad + 1] = 0
            interior = True
    return ids


def pad_prefixes(ids):
    return [int(np.argmax(row != 0)) if row.any() else len(row) for row in ids]


def make_inputs(c):
    """Seeded per case.  float32 values (what the device gets), so the float64 reference starts from exactly the same numbers.  x has zero rows
    where the id is 0, as every layer input of the model has (the embedding and every layer mask their output); feats is last_layernorm's output
    in the model, which is not zero there.  drec is in the reference's row order (row l * B + b), as the header states."""
    r = np.random.default_rng(zlib.crc32(repr(tuple(c)).encode()))
    ids = make_ids(c, r)
    m = (ids != 0)[..., None].astype(np.float32)
    P = so.init_params(so.Cfg(1, 4, D, c.H, 1), seed=int(r.integers(1 << 30)))
    pre = ENC_PRE if c.kind == "enc" else DEC_PRE
    P = {n: P[pre + n] for n in names(c.kind)}
    f = lambda *s: r.standard_normal(s, dtype=np.float32)
    out = dict(ids=ids, P=P, x=f(c.B, c.L, D) * m, gy=f(c.B, c.L, D))
    if c.kind == "enc":
        out["drec"] = np.float32(0.1) * f(c.B, c.L, c.H, c.H)
    else:
        out["feats"] = f(c.B, c.L, D)
    return out


def _f64(P):
    return {k: v.astype(np.float64) for k, v in P.items()}


def run_oracle(c, inp, mode, b_offset=None, rows=None, gate=None, rec_given=None, kernel_roundings=True):
    """One mode of the reference: every tensor the GPU test compares, float64.  Keys: y, rec (reference row order; H > 1), y_eval (encoder: the
    eval forward, p = 0), gx, gfeats, g.<name> per parameter, and for the encoder at H > 1 the same backward without drec under n.gx /
    n.g.<name>.
    rows: a (lo, hi) slice of sequences to return activations and input gradients of (the shard contract).
    kernel_roundings=False: the bare operand-rounding mode, without the two oracle options of the module docstring.
    "_u": the feed-forward's relu(dropout(conv1 .)) of the same rows.  gate: boolean, shaped like "_u": the backward takes the ReLU's derivative
    from there for those rows (the kernel's saved u > 0) instead of from this run's own u > 0.  rec_given (encoder): the head-classifier
    log-probabilities the backward starts from, for those rows, in the reference's row order -- the kernel's forward output, which the caller hands
    back to the kernel's backward: dz = drec - exp(rec) * sum(drec) is then formed from the same numbers on both sides, and the forward's own
    distance (checked under "rec") is not counted a second time in the classifier's gradients."""
    b_offset = c.b_offset if b_offset is None else b_offset
    P = _f64(inp["P"])
    ids = inp["ids"]
    m = (ids != 0)[..., None].astype(np.float64)
    x, gy = inp["x"].astype(np.float64), inp["gy"].astype(np.float64) * GY_SCALE
    sl = slice(*rows) if rows else slice(None)
    out = {}

    def put_gx(prefix, gx):
        out[prefix + "gx"] = gx[sl]

    def gate_of(cache):
        out["_u"] = cache["fc"][1][sl]
        if gate is None:
            return None
        full = cache["fc"][1] > 0
        full[sl] = np.asarray(gate, bool).reshape(full[sl].shape)
        return full

    with so.operands(mode, bias_as_product=kernel_roundings, saved_o_bf16=kernel_roundings):
        if c.kind == "enc":
            y, rec, cache = so.encoder_layer(x, m, P, "", c.H, c.p, SEED, sites("enc"), b_offset)
            out["y"] = y[sl]
            out["y_eval"] = so.encoder_layer(x, m, P, "", c.H, 0.0, SEED, sites("enc"), b_offset)[0][sl]
            gt = gate_of(cache)
            if rec_given is not None and c.H > 1:
                cache = dict(cache, rec=cache["rec"].copy())
                cache["rec"][sl] = so.rec_token_order(np.asarray(rec_given, np.float64).reshape(cache["rec"][sl].shape))
            if c.H > 1:
                out["rec"] = so.rec_reference_order(rec[sl])
                G = {}
                put_gx("", so.encoder_layer_bwd(gy, so.rec_token_order(inp["drec"].astype(np.float64)), cache, P, "", c.H, G, gt))
                out.update({"g." + k: np.asarray(v) for k, v in G.items()})
            G = {}
            put_gx("n." if c.H > 1 else "", so.encoder_layer_bwd(gy, None, cache, P, "", c.H, G, gt))
            out.update({("n.g." if c.H > 1 else "g.") + k: np.asarray(v) for k, v in G.items() if v is not None})
        else:
            y, cache = so.decoder_layer(x, inp["feats"].astype(np.float64), m, P, "", c.H, c.p, SEED, sites("dec"), b_offset)
            out["y"] = y[sl]
            G = {}
            gx, gf = so.decoder_layer_bwd(gy, cache, P, "", c.H, G, gate_of(cache))
            put_gx("", gx)
            out["gfeats"] = gf[sl]
            out.update({"g." + k: np.asarray(v) for k, v in G.items()})
    return out


def is_act(key):
    return key in ("y", "rec", "y_eval")


def tensor_class(key):
    if is_act(key):
        return key
    k = key[2:] if key.startswith("n.") else key
    if not k.startswith("g."):
        return k
    return "cls" if "sparse" in k else "layernorm" if "norm" in k else "bias" if k.endswith("bias") else "weight"


def grad_scale(want):
    """The largest gradient-tensor norm of a case: the floor of the small-tensor rule."""
    return max(float(np.linalg.norm(v)) for k, v in want.items() if not is_act(k))


def dist(key, got, want, gmax):
    got, want = np.asarray(got, np.float64).reshape(want.shape), np.asarray(want, np.float64)
    if is_act(key):
        return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-30))
    return float(np.linalg.norm(got - want) / max(np.linalg.norm(want), SMALL * gmax))


_REF = {}


def reference(c, b_offset=None, rows=None):
    """(inputs, want, D, bound, u) of a case, computed once and shared: want = the bf16x64 reference, D[k] = dist(plain, want), bound[k] =
    min(2 D[k], cap), u = the reference's relu output ("_u" of run_oracle)."""
    key = (c, b_offset, rows)
    if key not in _REF:
        inp = make_inputs(c)
        want, plain = run_oracle(c, inp, "bf16x64", b_offset, rows), run_oracle(c, inp, None, b_offset, rows)
        u = want.pop("_u")
        plain.pop("_u")
        gmax = grad_scale(want)
        Dk = {k: dist(k, plain[k], want[k], gmax) for k in want}
        bound = {k: min(FACTOR * Dk[k], CAP_ACT if is_act(k) else CAP_GRAD) for k in want}
        for v in want.values():
            v.setflags(write=False)
        _REF[key] = (inp, want, Dk, bound, u)
    return _REF[key]


# ---- the device side (imported by the GPU test only) ----------------------------------------------------------------------------------------------
class Layer:
    """One layer on the device: flat parameter buffer, its gradient twin, the packed weight images (3 x the flat buffer, as
    SuperSASRecModel.pack_selected lays them out) and the two pointer structs."""

    def __init__(self, c, inp, dev="cuda:0"):
        import ctypes
        import torch
        from adt_amd import _lib, ops
        self.c, self.lib, self.dev = c, _lib.load(), dev
        self.lay, n = layout(c.kind, c.H)
        flat = np.zeros(n, np.float32)
        for k, (o, shp) in self.lay.items():
            flat[o:o + int(np.prod(shp))] = inp["P"][k].ravel()
        self.flat = torch.from_numpy(flat).to(dev)
        self.grad = torch.zeros_like(self.flat)
        self.wimg = torch.zeros(3 * n, device=dev, dtype=torch.float32)
        offs = block_offsets(c.kind, c.H)
        assert len(offs) == (6 if c.kind == "enc" else 10)
        arr = (ctypes.c_int * len(offs))(*offs)
        _lib.check(self.lib.adt_pack_wimg(ops._p(self.flat), ops._p(self.wimg), arr, len(offs), ops._stream()), "pack_wimg")
        cls = _lib.EncLayerPtrs if c.kind == "enc" else _lib.DecLayerPtrs
        mk = lambda buf: cls(**{f: buf.data_ptr() + 4 * self.lay[k][0] for f, k in zip(cls.NAMES, names(c.kind))})
        self.P, self.G = mk(self.flat), mk(self.grad)
        self.seed = torch.tensor([SEED - (1 << 32) if SEED >= (1 << 31) else SEED], dtype=torch.int32, device=dev)
        T = c.B * c.L
        self.T = T
        self.nsave = int(self.lib.adt_seq_layer_save_floats(c.B, c.L, c.H, int(c.kind == "dec")))
        self.nscratch = (2 if c.kind == "enc" else 4) * ((T * D + 63) // 64 * 64)
        self.ids = torch.from_numpy(inp["ids"].reshape(-1)).to(dev)
        self.x = torch.from_numpy(inp["x"].reshape(T, D)).to(dev)
        self.feats = torch.from_numpy(inp["feats"].reshape(T, D)).to(dev) if c.kind == "dec" else None
        self.save = None

    @staticmethod
    def supported(c):
        from adt_amd import _lib
        return _lib.load().adt_seq_layer_supported(1, c.L, D, D // c.H) == 1

    def nan(self, *shape):
        import torch
        return torch.full(shape, float("nan"), device=self.dev, dtype=torch.float32)

    def saved_u(self):
        """(T, 64) float32: the relu(dropout(conv1 .)) rows the last training forward saved for the backward -- bf16 rows in the third row block
        of `save` (adt_sasrec.hip: layer_save: o, h, u, ...; each block T * 32 floats rounded up to 64).  Within a row the 16 values of lane group
        g sit together (adt_tt.cuh: tt_store_bf16): position 16 g + 4 nt + r holds column 16 nt + 4 g + r."""
        import torch
        row = (self.T * 32 + 63) // 64 * 64
        u = self.save[2 * row:2 * row + self.T * 32].view(torch.bfloat16).view(self.T, 4, 4, 4).float()
        return u.permute(0, 2, 1, 3).reshape(self.T, D)

    def g(self, name):
        o, shp = self.lay[name]
        return self.grad[o:o + int(np.prod(shp))].view(*shp)

    def fwd(self, y=None, y_scale=1.0, y_acc=0, training=1, p=None, want_rec=True, b_offset=None):
        """-> (y, rec | None).  save and (without y_acc) y are NaN-filled first."""
        import ctypes
        from adt_amd import _lib, ops
        c, st = self.c, sites(self.c.kind)
        p = c.p if p is None else p
        b_offset = c.b_offset if b_offset is None else b_offset
        self.save = self.nan(self.nsave)
        if y is None:
            assert not y_acc
            y = self.nan(self.T, D)
        rec = None
        if c.kind == "enc":
            rec = self.nan(self.T, c.H * c.H) if want_rec else None
            rc = self.lib.adt_seq_enc_layer_fwd(c.B, c.L, c.H, ops._p(self.ids), ops._p(self.x), ctypes.byref(self.P), ops._p(self.flat), ops._p(self.wimg),
                                                float(p), ops._p(self.seed), st["attn"], st["ffn1"], st["ffn2"], b_offset, int(training), ops._p(self.save),
                                                ops._p(y), float(y_scale), int(y_acc), ops._p(rec), ops._stream())
        else:
            rc = self.lib.adt_seq_dec_layer_fwd(c.B, c.L, c.H, ops._p(self.ids), ops._p(self.x), ops._p(self.feats), ctypes.byref(self.P), ops._p(self.flat),
                                                ops._p(self.wimg), float(p), ops._p(self.seed), st["slf"], st["enc"], st["ffn1"], st["ffn2"], b_offset,
                                                ops._p(self.save), ops._p(y), float(y_scale), int(y_acc), ops._stream())
        _lib.check(rc, "seq_%s_layer_fwd" % c.kind)
        return y, rec

    def bwd(self, gy, rec=None, drec=None, gx=None, gx_acc=0, gfeats=None, gy_scale=GY_SCALE, b_offset=None):
        """-> (gx, gfeats | None) after the forward that filled self.save.  Scratch and (without gx_acc) gx are NaN-filled first; gfeats is added
        to (zeros unless given).  Parameter gradients are added into self.grad."""
        import ctypes
        import torch
        from adt_amd import _lib, ops
        c, st = self.c, sites(self.c.kind)
        b_offset = c.b_offset if b_offset is None else b_offset
        scratch = self.nan(self.nscratch)
        if gx is None:
            assert not gx_acc
            gx = self.nan(self.T, D)
        if c.kind == "enc":
            rc = self.lib.adt_seq_enc_layer_bwd(c.B, c.L, c.H, ops._p(self.ids), ops._p(self.x), ctypes.byref(self.P), ctypes.byref(self.G), ops._p(self.flat),
                                                ops._p(self.wimg), float(c.p), ops._p(self.seed), st["attn"], st["ffn1"], st["ffn2"], b_offset, ops._p(self.save),
                                                ops._p(gy), float(gy_scale), ops._p(rec), ops._p(drec), ops._p(gx), int(gx_acc), ops._p(scratch), ops._stream())
        else:
            if gfeats is None:
                gfeats = torch.zeros(self.T, D, device=self.dev, dtype=torch.float32)
            rc = self.lib.adt_seq_dec_layer_bwd(c.B, c.L, c.H, ops._p(self.ids), ops._p(self.x), ops._p(self.feats), ctypes.byref(self.P), ctypes.byref(self.G),
                                                ops._p(self.flat), ops._p(self.wimg), float(c.p), ops._p(self.seed), st["slf"], st["enc"], st["ffn1"], st["ffn2"],
                                                b_offset, ops._p(self.save), ops._p(gy), float(gy_scale), ops._p(gx), int(gx_acc), ops._p(gfeats), ops._p(scratch),
                                                ops._stream())
        _lib.check(rc, "seq_%s_layer_bwd" % c.kind)
        return gx, gfeats
