"""Host-side plumbing shared by the BERT4Rec-ADT and STOSA-ADT models: one flat fp32 parameter buffer with the
reference's state_dict names as views, and a small launch tape that strings the C-ABI stage kernels
(include/adt_hip.h, "wide" section) into a forward pass and its reverse.

Nothing here computes on the host or through torch operators: tensors are allocated with torch (device memory,
streams, HIP-graph capture) and every arithmetic step is a kernel of libadt_hip.so.  A missing library raises.
"""
import numpy as np
import torch

from . import _lib, ops
from .dp import GradBuckets, capture, reduce_sum


class _Holder(torch.nn.Module):
    """Plain container so that named_parameters()/state_dict() reproduce the reference's dotted names.  A holder of exactly one
    2-D `weight` (an embedding table) is callable like the reference's nn.Embedding: the reference's trainers look item / user
    rows up through the module (stosa/trainer.py:361-364, stosa/models.py:236), a plain torch gather outside the hot path."""

    def forward(self, ids):
        w = self._parameters.get("weight")
        if w is None or w.dim() != 2:
            raise TypeError("this container holds parameters only; it is not a layer")
        ids = ids if isinstance(ids, torch.Tensor) else torch.as_tensor(np.asarray(ids))
        return torch.nn.functional.embedding(ids.to(device=w.device, dtype=torch.long), w)


def _set_nested(root, dotted, param):
    parts = dotted.split(".")
    m = root
    for p in parts[:-1]:
        if not hasattr(m, p):
            m.add_module(p, _Holder())
        m = getattr(m, p)
    m.register_parameter(parts[-1], param)


def ref_sorted(names, order):
    """`names` (dotted parameter names) in the order the reference's nn.Module tree registers them, which is the order of
    model.parameters() and therefore the key order of torch.optim.Adam.state_dict().  `order` lists path components in the
    order the reference's constructors create them (siblings only are ever compared); numeric components sort as integers.
    Pinned by tests/golden/param_order.json (tests/test_utils_cpu.py)."""
    rank = {c: i for i, c in enumerate(order)}

    def key(n):
        return tuple((0, int(c)) if c.isdigit() else (1, rank[c]) for c in n.split("."))
    return sorted(names, key=key)


HEAD_PADS = (16, 32, 64, 128, 256)
WIDTH_PADS = (64, 128, 192, 256)


def padded_layout(d, H):
    """(hd, hd_pad, d_pad) of hidden width d with H heads on the stage kernels: hd = d / H, hd_pad the smallest of 16, 32, 64, 128, 256
    that holds hd, d_pad = H * hd_pad, which must be 64, 128, 192 or 256.  Head h occupies columns [h * hd_pad, h * hd_pad + hd) of a
    padded row; the other lanes are zero.  Pure arithmetic (no GPU, no library); raises AdtError for a shape the kernels do not tile."""
    d, H = int(d), int(H)
    rule = "hd = d / H, hd_pad = smallest of %s >= hd, d_pad = H * hd_pad must be one of %s" % (list(HEAD_PADS), list(WIDTH_PADS))
    if d < 1 or H < 1 or d % H:
        raise _lib.AdtError("hidden_units d=%d is not a positive multiple of num_heads H=%d (%s)" % (d, H, rule))
    hd = d // H
    pads = [p for p in HEAD_PADS if p >= hd]
    if not pads:
        raise _lib.AdtError("d=%d H=%d: head size hd=%d exceeds hd_pad=%d (%s)" % (d, H, hd, HEAD_PADS[-1], rule))
    hd_pad = pads[0]
    d_pad = H * hd_pad
    if d_pad not in WIDTH_PADS:
        raise _lib.AdtError("d=%d H=%d: hd=%d pads to hd_pad=%d, d_pad=%d is not supported (%s)" % (d, H, hd, hd_pad, d_pad, rule))
    return hd, hd_pad, d_pad


def lane_index(ref_table, pad_table, pad_offsets, d, H, prefix=()):
    """For every element of the reference-shaped parameters (ref_table order, packed densely) its position in the padded flat buffer.
    A dimension of size d (or 3d, or hd) that the padded table widens to d_pad (3 d_pad, hd_pad) maps channel h * hd + j to
    h * hd_pad + j; equal dimensions map to themselves.  prefix: (name, axis) pairs whose dimension the padded table widens by a
    zero-filled TAIL (BERT4Rec-ADT's inner_units rounded up to a multiple of 4): element j stays at j."""
    hd, hd_pad, d_pad = padded_layout(d, H)
    chan = (np.arange(d) // hd) * hd_pad + np.arange(d) % hd
    maps = {(d, d_pad): chan, (3 * d, 3 * d_pad): np.concatenate([chan + k * d_pad for k in range(3)]), (hd, hd_pad): np.arange(hd)}
    pad_shapes = dict(pad_table)
    out = []
    for name, shape in ref_table:
        pshape = pad_shapes[name]
        assert len(pshape) == len(shape), (name, shape, pshape)
        idx = np.zeros((), dtype=np.int64)
        stride = 1
        for ax, (r, q) in enumerate(zip(shape[::-1], pshape[::-1])):
            m = np.arange(r) if r == q or (name, len(shape) - 1 - ax) in prefix else maps[(r, q)]
            idx = m.reshape((-1,) + (1,) * idx.ndim) * stride + idx
            stride *= q
        out.append((idx + pad_offsets[name]).reshape(-1))
    idx = np.concatenate(out)
    assert idx.max() < (1 << 31) and np.unique(idx).size == idx.size
    return idx.astype(np.int32)


class FlatModule(torch.nn.Module):
    """nn.Module whose parameters are views into ONE flat fp32 GPU buffer (`flat`), with an identically laid-out
    gradient buffer (`flat_grad`): the optimizer and the gradient all-reduce see one array.  Tensors start on 16-byte
    boundaries; tensors listed consecutively with sizes that are multiples of 4 floats are contiguous, which is what
    lets q/k/v projections run as one GEMM over a (3d, d) view."""

    def _build_flat(self, table, device, ref_order=None, ref_table=None, width=None, prefix=()):
        """ref_table / width=(d, H): `table` is the PADDED layout of a width the kernels do not tile (padded_layout); the registered
        parameters then have the reference's shapes and live in a second, densely packed buffer `ref_flat`, copied to and from the
        live lanes of `flat` by push() / pull() (one kernel each).  Between steps ref_flat is the truth; the pad lanes of `flat`
        are zero and nothing ever writes them."""
        self.lib = _lib.load()   # raises when the HIP library is missing: no fallback
        self.dev = torch.device(device)
        if self.dev.type != "cuda":
            raise _lib.AdtError("%s (adt_amd) needs a GPU device, got %r" % (type(self).__name__, device))
        self.table = list(table)
        off = 0
        self._views = {}
        for name, shape in self.table:
            n = int(np.prod(shape))
            self._views[name] = (off, n, tuple(shape))
            off += (n + 3) // 4 * 4
        self.n_flat = off
        self.flat = torch.zeros(off, device=self.dev, dtype=torch.float32)
        self.flat_grad = torch.zeros_like(self.flat)
        # The flat layout follows `table` (what the kernels want: q/k/v consecutive, never-trained tensors last); the nn.Module
        # registration follows the reference's constructor order so that parameters() lines up with the reference's optimizer.
        names = [n for n, _ in self.table]
        self.ref_flat, self.lane_idx, self._ref_views = None, None, None
        if ref_table is not None:
            ref_table = [(n, tuple(s)) for n, s in ref_table]
            assert [n for n, _ in ref_table] == names
            index = lane_index(ref_table, self.table, {n: v[0] for n, v in self._views.items()}, *width, prefix=prefix)
            self.lane_idx = torch.from_numpy(index).to(self.dev)
            self._lane_host = index      # ascending (the two tables list the same tensors in the same order): ref_range() searches it
            self.ref_flat = torch.zeros(index.size, device=self.dev, dtype=torch.float32)
            self._ref_views, o = {}, 0
            for name, shape in ref_table:
                n = int(np.prod(shape))
                self._ref_views[name] = (o, n, shape)
                o += n
        for name in (ref_sorted(names, ref_order) if ref_order else names):
            o, n, shape = (self._ref_views or self._views)[name]
            src = self.flat if self.ref_flat is None else self.ref_flat
            _set_nested(self, name, torch.nn.Parameter(src[o:o + n].view(shape), requires_grad=True))
        self._seed = torch.zeros(1, device=self.dev, dtype=torch.int32)   # uint32 bits of the dropout seed, device resident
        self._step_seed = 0
        self.dp_hook = None       # see Tape.mark_decoder_start

    def offset_of(self, name):
        """Flat offset (floats) of a parameter: bucket boundaries of the gradient all-reduce."""
        return self._views[name][0]

    def _apply(self, fn, recurse=True):
        probe = fn(self.flat)
        if probe.device != self.flat.device or probe.dtype != self.flat.dtype:
            raise _lib.AdtError("%s (adt_amd) parameters live in one flat fp32 GPU buffer; .to(%s, %s) is unsupported"
                                % (type(self).__name__, probe.device, probe.dtype))
        return self

    def P(self, name):
        o, n, shape = self._views[name]
        return self.flat[o:o + n].view(shape)

    def G(self, name):
        o, n, shape = self._views[name]
        return self.flat_grad[o:o + n].view(shape)

    def R(self, name):
        """The parameter in the reference's shape (a view of ref_flat for a padded layout, of flat otherwise)."""
        o, n, shape = (self._ref_views or self._views)[name]
        return (self.flat if self.ref_flat is None else self.ref_flat)[o:o + n].view(shape)

    def GR(self, name):
        """The gradient in the reference's shape (for a padded layout a compacted copy of flat_grad, not a view)."""
        if self.ref_flat is None:
            return self.G(name)
        o, n, shape = self._ref_views[name]
        return self.compact(self.flat_grad)[o:o + n].view(shape)

    @property
    def master(self):
        """The buffer that holds the weights between steps (what a data-parallel run broadcasts from rank 0)."""
        return self.flat if self.ref_flat is None else self.ref_flat

    def push(self):
        """Reference-shaped parameters -> live lanes of the padded flat buffer (no-op without padding)."""
        if self.ref_flat is not None:
            ops.lane_map(self.flat, self.ref_flat, self.lane_idx, True)

    def pull(self):
        """Live lanes of the padded flat buffer -> reference-shaped parameters (no-op without padding)."""
        if self.ref_flat is not None:
            ops.lane_map(self.flat, self.ref_flat, self.lane_idx, False)

    def ref_range(self, lo, hi):
        """[lo, hi) of the padded flat buffer as the range of ref_flat whose elements live there.  lane_idx ascends, so a range that holds
        whole tensors of the padded table holds a contiguous run of the reference-shaped ones.  Kept per range: a supernet has a few dozen,
        and numpy converts the whole int32 index for every search with an int key -- milliseconds of host time per range and step."""
        cache = self.__dict__.setdefault("_ref_ranges", {})
        if (lo, hi) not in cache:
            idx = self._lane_host
            cache[(lo, hi)] = tuple(int(np.searchsorted(idx, idx.dtype.type(min(x, np.iinfo(idx.dtype).max)))) for x in (lo, hi))
        return cache[(lo, hi)]

    def push_ranges(self, ranges):
        """push() of the flat ranges [(lo, hi)] only (a supernet step trains a few of its candidate layers)."""
        if self.ref_flat is not None:
            for r0, r1 in (self.ref_range(lo, hi) for lo, hi in ranges):
                ops.lane_map(self.flat, self.ref_flat[r0:r1], self.lane_idx[r0:r1], True)

    def pull_ranges(self, ranges):
        if self.ref_flat is not None:
            for r0, r1 in (self.ref_range(lo, hi) for lo, hi in ranges):
                ops.lane_map(self.flat, self.ref_flat[r0:r1], self.lane_idx[r0:r1], False)

    def compact(self, padded):
        """The live lanes of a buffer laid out like `flat` (an Adam moment), packed like ref_flat."""
        out = torch.empty_like(self.ref_flat)
        ops.lane_map(padded, out, self.lane_idx, False)
        return out

    def expand_into(self, padded, compact):
        ops.lane_map(padded, compact.to(device=self.dev, dtype=torch.float32).contiguous(), self.lane_idx, True)

    def load_state_dict(self, *a, **kw):
        r = super().load_state_dict(*a, **kw)
        self.push()
        return r

    def span(self, first, last, shape, grad=False):
        """One view over the consecutive tensors first..last (e.g. query/key/value weights as (3d, d))."""
        o0 = self._views[first][0]
        o1, n1, _ = self._views[last]
        buf = self.flat_grad if grad else self.flat
        v = buf[o0:o1 + n1]
        assert v.numel() == int(np.prod(shape)), (first, last, shape, v.numel())
        return v.view(shape)

    def set_seed(self, seed):
        self._seed.fill_(int(np.array([seed & 0xFFFFFFFF], dtype=np.uint32).view(np.int32)[0]))

    def next_seed(self):
        self._step_seed += 1
        self.set_seed(self._step_seed * 2654435761 + 12345)

    def seed_trainer(self, seed):
        """The dropout stream a trainer constructed with `seed` starts from."""
        self.set_seed(seed * 1000003 + 12345)

    def advance_seed(self):
        self._seed.add_(-1640531535)    # += 0x9E3779B1 (mod 2^32): a fresh dropout stream every step, on the device

    def ids(self, a):
        if isinstance(a, torch.Tensor):
            return a.to(device=self.dev, dtype=torch.int32).contiguous()
        return torch.from_numpy(np.ascontiguousarray(np.asarray(a), dtype=np.int32)).to(self.dev)

    def load_numpy(self, P):
        for k, v in P.items():
            self.R(k).copy_(torch.from_numpy(np.ascontiguousarray(v)))
        self.push()


def loss_norms(model, T, n_bce=0.0, scale=1):
    """Device normalisers {n_bce, n_mse, n_nll} of the loss seeds for T = B * L token rows: the BCE count (0 where the loss has no BCE
    term), T * d and T * H.  `scale`: the factor from a data-parallel shard's rows to the GLOBAL batch (adt_amd/dp.py, rule 1)."""
    return torch.tensor([float(n_bce), float(scale * T * model.hidden_units), float(scale * T * model.num_heads)], device=model.dev,
                        dtype=torch.float32)


class Act:
    """An activation and (lazily) its gradient buffer."""
    __slots__ = ("t", "g")

    def __init__(self, t):
        self.t = t
        self.g = None


def add_into(dst, src):
    """dst += src through the library's elementwise kernel (dropout off, identity activation)."""
    ops.dropact_bwd(src, src, 0.0, None, 0, dst, True)


def give(a, g):
    """Hand gradient `g` (complete, not used again by the caller) to activation `a`."""
    if a.g is None:
        a.g = g
    else:
        add_into(a.g, g)


class Tape:
    """Forward launches + the closures that undo them.  `prec`: ops.PREC_*; `seed`: device uint32; `row_offset`: first
    global token row of this data-parallel shard (dropout indices are global)."""

    def __init__(self, model, prec, training, row_offset=0, b_offset=0):
        self.m, self.prec, self.training = model, prec, training
        self.seed = model._seed
        self.row_offset, self.b_offset = row_offset, b_offset
        self.bw = []
        self.marks = {}
        self.lanes = getattr(model, "lanes", None)      # (H, hd, hd_pad) of a padded width (padded_layout), else None

    def p_eff(self, p):
        return float(p) if self.training else 0.0

    def mark_decoder_start(self):
        """Called by a model's forward where its decoder stack begins: every closure recorded from here on belongs to the decoder
        (and the output head after it), whose parameters sit at the END of the flat buffer.  In the backward, `model.dp_hook`
        (the data-parallel trainers set it to GradBuckets.tail_ready) fires as soon as those closures have run, so that bucket's
        all-reduce overlaps the encoder's backward and the embedding scatter."""
        hook = getattr(self.m, "dp_hook", None)
        if hook is not None:
            self.marks[len(self.bw)] = hook

    def backward(self):
        for i in range(len(self.bw) - 1, -1, -1):
            self.bw[i]()
            hook = self.marks.get(i)
            if hook is not None:
                hook()
        self.bw, self.marks = [], {}

    # ---- Linear (+ activation, dropout, residual) -------------------------------------------------------------------
    def dense(self, x, W, b, gW, gb, act=ops.ACT_NONE, p=0.0, site=0, R=None, t_dev=None, ldy=None, R2=None, mask_ids=None):
        """y = mask(R + R2 + dropout(act(x W^T + b))).  With a row mask the residuals receive the masked gradient."""
        p = self.p_eff(p)
        if self.lanes is not None and p > 0.0:
            assert t_dev is None and ldy is None, "padded widths: a device row count / output stride is not carried through the dropout pass"
            return self._dense_lanes(x, W, b, gW, gb, act, p, site, R, R2, mask_ids)
        Y, U = ops.dense_fwd(self.prec, x.t, W, b, act, act != ops.ACT_NONE, p, self.seed, site, self.row_offset, None if R is None else R.t,
                             mask_ids, None, t_dev, ldy, None if R2 is None else R2.t)
        y = Act(Y)

        def bw():
            if y.g is None:
                return
            if x.g is None:
                x.g = torch.empty_like(x.t)
                beta = False
            else:
                beta = True
            if act != ops.ACT_NONE and y.g.shape[1] >= 256:
                # wide layers with an activation: pull the gradient through the epilogue once (one elementwise pass) instead of
                # inside every column tile of the two backward GEMMs
                G = ops.dense_gradsrc(y.g, act, U, p, self.seed, site, self.row_offset, mask_ids, t_dev)
                ops.dense_bwd(self.prec, G, x.t, W, gW, gb, x.g, beta, ops.ACT_NONE, None, 0.0, None, 0, 0, None, t_dev)
            else:
                ops.dense_bwd(self.prec, y.g, x.t, W, gW, gb, x.g, beta, act, U, p, self.seed, site, self.row_offset, mask_ids, t_dev)
            for res in (R, R2):
                if res is None:
                    continue
                if mask_ids is None and R2 is None:
                    give(res, y.g)          # y.g is not used again: hand the buffer over
                else:
                    g = torch.empty_like(y.g)
                    ops.axpy(g, y.g, 1.0, False, mask_ids, y.g.shape[1])
                    give(res, g)
        self.bw.append(bw)
        return y

    def _dense_lanes(self, x, W, b, gW, gb, act, p, site, R, R2, mask_ids):
        """dense() on a padded width with dropout on.  The GEMM epilogues index the dropout RNG by row * N + column with the PADDED N;
        the oracle's index runs over the true width.  So the layer runs without its dropout, residuals and row mask, and one
        elementwise pass (adt_drop_lanes) applies them with true-width indices; the backward pulls the gradient through the same pass
        first.  relu(dropout(u)) == dropout(relu(u)) (the scale is positive), so the activation stays in the GEMM."""
        Y, U = ops.dense_fwd(self.prec, x.t, W, b, act, act != ops.ACT_NONE)
        ops.drop_lanes(Y, self.lanes, p, self.seed, site, self.row_offset, None if R is None else R.t, None if R2 is None else R2.t, mask_ids, out=Y)
        y = Act(Y)

        def bw():
            if y.g is None:
                return
            beta = x.g is not None
            if not beta:
                x.g = torch.empty_like(x.t)
            G = ops.drop_lanes(y.g, self.lanes, p, self.seed, site, self.row_offset, mask_ids=mask_ids)
            ops.dense_bwd(self.prec, G, x.t, W, gW, gb, x.g, beta, act, U)
            for res in (R, R2):
                if res is None:
                    continue
                if mask_ids is None and R2 is None:
                    give(res, y.g)
                else:
                    g = torch.empty_like(y.g)
                    ops.axpy(g, y.g, 1.0, False, mask_ids, y.g.shape[1])
                    give(res, g)
        self.bw.append(bw)
        return y

    def mix(self, parts):
        """sum_k w_k * a_k (supernet candidate mixing, sasrec/super_modules.py:42-49)."""
        out = torch.empty_like(parts[0][0].t)
        for k, (a, w) in enumerate(parts):
            ops.axpy(out, a.t, w, k > 0)
        y = Act(out)

        def bw():
            if y.g is None:
                return
            for a, w in parts:
                if a.g is None:
                    a.g = torch.empty_like(a.t)
                    ops.axpy(a.g, y.g, w, False)
                else:
                    ops.axpy(a.g, y.g, w, True)
        self.bw.append(bw)
        return y

    def log_softmax(self, x, H):
        y = Act(ops.log_softmax_fwd(x.t, H))

        def bw():
            if y.g is None:
                return
            acc = x.g is not None
            if not acc:
                x.g = torch.empty_like(x.t)
            ops.log_softmax_bwd(y.t, y.g, H, x.g, acc)
        self.bw.append(bw)
        return y

    def layernorm(self, x, w, b, gw, gb, eps):
        if self.lanes is not None:
            return self._layernorm_lanes(x, w, b, gw, gb, eps)
        y = Act(ops.layernorm_fwd(x.t, w, b, eps))

        def bw():
            if y.g is None:
                return
            acc = x.g is not None
            if not acc:
                x.g = torch.empty_like(x.t)
            ops.layernorm_bwd(y.g, x.t, w, eps, x.g, acc, gw, gb)
        self.bw.append(bw)
        return y

    def _layernorm_lanes(self, x, w, b, gw, gb, eps):
        y = Act(ops.layernorm_lanes_fwd(x.t, w, b, eps, self.lanes))

        def bw():
            if y.g is None:
                return
            acc = x.g is not None
            if not acc:
                x.g = torch.empty_like(x.t)
            ops.layernorm_lanes_bwd(y.g, x.t, w, eps, x.g, acc, gw, gb, self.lanes)
        self.bw.append(bw)
        return y

    def dropact(self, x, p, site, act=ops.ACT_NONE):
        p = self.p_eff(p)
        if p == 0.0 and act == ops.ACT_NONE:
            return x
        if self.lanes is not None:
            return self._drop_lanes(x, p, site) if act == ops.ACT_NONE else self.act_lanes(x, act, p, site)
        off = self.row_offset * x.t.shape[1]
        y = Act(ops.dropact_fwd(x.t, p, self.seed, site, off, act))

        def bw():
            if y.g is None:
                return
            acc = x.g is not None
            if not acc:
                x.g = torch.empty_like(x.t)
            ops.dropact_bwd(y.g, x.t, p, self.seed, site, x.g, acc, off, act)
        self.bw.append(bw)
        return y

    def _drop_lanes(self, x, p, site):
        """dropact() on a padded width: the dropout index runs over the true width (adt_drop_lanes)."""
        y = Act(ops.drop_lanes(x.t, self.lanes, p, self.seed, site, self.row_offset))

        def bw():
            if y.g is None:
                return
            give(x, ops.drop_lanes(y.g, self.lanes, p, self.seed, site, self.row_offset))
        self.bw.append(bw)
        return y

    def act_lanes(self, x, act, p=0.0, site=0):
        """act(dropout(x)) on a padded width: the activation on the live lanes only (ELU(0) + 1 = 1 must not reach a pad lane), the dropout
        index over the true width (adt_act_lanes_fwd / _bwd).  x may be n padded rows side by side (the q / k / v projections) when p = 0."""
        p = self.p_eff(p)
        y = Act(ops.act_lanes_fwd(x.t, self.lanes, act, p, self.seed, site, self.row_offset))

        def bw():
            if y.g is None:
                return
            acc = x.g is not None
            if not acc:
                x.g = torch.empty_like(x.t)
            ops.act_lanes_bwd(y.g, x.t, self.lanes, act, x.g, acc, p, self.seed, site, self.row_offset)
        self.bw.append(bw)
        return y

    def drn_lanes(self, x, W, b, gW, gb, p, site, R, w, bn, gw, gbn, eps):
        """LN(R + dropout(x W^T + b)) on a padded width with dropout on: the GEMM without an epilogue, then ONE pass that drops (indexed
        at the true width), adds the residual and normalises over the live lanes (adt_drn_lanes_fwd; Z overwrites the GEMM's output).
        The backward is one pass too: dZ into the residual's gradient, dS for the two backward GEMMs."""
        p = self.p_eff(p)
        S, _ = ops.dense_fwd(self.prec, x.t, W, b)
        Z, Y = ops.drn_lanes_fwd(S, R.t, w, bn, eps, self.lanes, p, self.seed, site, self.row_offset, Z=S)
        y = Act(Y)

        def bw():
            if y.g is None:
                return
            acc = R.g is not None
            if not acc:
                R.g = torch.empty_like(R.t)
            dS = torch.empty_like(Z)
            ops.drn_lanes_bwd(y.g, Z, w, eps, self.lanes, p, self.seed, site, self.row_offset, R.g, acc, dS, gw, gbn)
            beta = x.g is not None
            if not beta:
                x.g = torch.empty_like(x.t)
            ops.dense_bwd(self.prec, dS, x.t, W, gW, gb, x.g, beta)
        self.bw.append(bw)
        return y

    def headcls(self, o, Ws, bs, gWs, gbs):
        """Independence head classifier + log_softmax on (T, H*hd) attention outputs, natural (b, l) row order."""
        T = o.t.shape[0]
        rec = Act(ops.headcls_fwd(o.t, Ws, bs, 1, T))

        def bw():
            if rec.g is None:
                return
            if o.g is None:
                o.g = torch.zeros_like(o.t)
            ops.headcls_bwd(o.t, Ws, rec.t, rec.g, 1, T, o.g, gWs, gbs)
        self.bw.append(bw)
        return rec


class TapeTrainer:
    """What the fused trainers of the tape models share (sasrec/model_wide.py, bert4rec/trainer.py, stosa/trainer.py): the flat Adam
    moments and device scalars, the data-parallel gradient buckets, the staged-batch buffers a HIP graph replays from, and the step
    protocol around one launch sequence.  A subclass supplies `stage(...)` (one batch -> dict of device tensors + "B"), `_body(st, b_offset)`
    (forward, loss, backward, `_buckets.finish()`, optimiser) and a `step(...)` with its own batch signature."""

    def __init__(self, model, loss_w, boundary, lr, betas, eps, weight_decay, clip, process_group, use_graph, n=None):
        """loss_w: the weight of every loss slot row in loss(); boundary: the first parameter of the gradient's tail bucket (the decoder, whose
        backward runs first); n: the trained prefix of the flat buffer when it is not all of it."""
        self.model = model
        self.lr, self.betas, self.eps, self.wd, self.clip = lr, betas, eps, weight_decay, clip
        self.pg = process_group
        self.world = 1 if process_group is None else torch.distributed.get_world_size(process_group)
        self.rank = 0 if process_group is None else torch.distributed.get_rank(process_group)
        self.use_graph = use_graph       # data-parallel steps are captured too (RCCL collectives are graph nodes)
        self._buckets = GradBuckets(model.flat_grad, model.offset_of(boundary), process_group, n=n)
        dev = model.dev
        self.m, self.v = torch.zeros_like(model.flat), torch.zeros_like(model.flat)
        self.scal = torch.zeros(192, device=dev, dtype=torch.float32)
        self.loss_slots = torch.zeros(len(loss_w), 64, device=dev, dtype=torch.float32)
        self._loss_w = torch.tensor(loss_w, device=dev, dtype=torch.float32)
        self.nstep = 0
        self._graph, self._st = None, None

    def _launch(self, b_offset):
        m = self.model
        m.advance_seed()
        self.loss_slots.zero_()
        m.flat_grad.zero_()
        m.dp_hook = self._buckets.tail_ready if self._buckets.active else None
        self._body(self._st, b_offset)

    def _copy_stage(self, st):
        """Graph replays read fixed buffers: copy the new batch into the captured ones."""
        if self._st is None or self._st["B"] != st["B"]:
            self._st = {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in st.items()}
            self._graph = None
            return
        for k, v in st.items():
            if isinstance(v, torch.Tensor):
                self._st[k].copy_(v, non_blocking=True)
            else:
                self._st[k] = v

    def step_staged(self, st, b_offset=0):
        self.model.train()
        self._copy_stage(st)
        self.nstep += 1
        if not self.use_graph:
            self._launch(b_offset)
            return
        if self._graph is None:
            self._launch(b_offset)          # warm up eagerly (hipFuncSetAttribute is not capturable), then capture
            torch.cuda.synchronize()
            self._graph = torch.cuda.CUDAGraph()
            with capture(self._graph):
                self._launch(b_offset)
            return
        self._graph.replay()

    def loss_parts(self):
        """The loss slots of the last step, one sum per row (summed over the ranks: each holds its shard's partial sums)."""
        slots = self.loss_slots.sum(1)
        return reduce_sum(slots, self.pg) if self.world > 1 else slots

    def loss(self):
        """Device scalar: the loss of the last step as the reference's training loop reports it."""
        return (self.loss_parts() * self._loss_w).sum()

    def grad_norm(self):
        return self.scal[1].sqrt()
