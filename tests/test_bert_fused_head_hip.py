"""GPU: the fused all-item logits + cross-entropy head at hidden width 64 (adt_lce.cuh at KD 64), opt-in through args.fused_head.

With the flag a d 64, bf16 model's gradients are held to tests/test_bert_hip.py's bf16 gradient bounds against the numpy oracle (relative
Frobenius 0.1; the key biases, whose gradient is zero up to rounding, below 1e-3 of the largest gradient) at L 20 and L 272.  Without the
flag the model is the one it was: it runs the dense head, as forced with ADT_LCE=0 (same entry points called, loss slots bit-equal;
flat_grad within the suite's bound for one gradient summed in two orders, since float atomics make it differ between two runs of the
same model).  Under f32 the flag changes nothing.  Graph replay is held to the suite's graph-against-eager bound
(tests/test_bert_hip.py::test_graph_replay_equals_eager)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import bert_oracle as bo  # noqa: E402
from tests.test_bert_hip import Args, rel  # noqa: E402
from tests.test_bert_long_hip import LAM1, LAM2, grads_of, oracle_case  # noqa: E402


def build(cfg, P, prec, fused_head=None, dropout=0.0, attention_dropout=0.0):
    from adt_amd.bert4rec.model import BertModel
    a = Args()
    a.device, a.maxlen, a.num_heads, a.num_layers, a.hidden_units, a.inner_units = "cuda:0", cfg.maxlen, cfg.num_heads, cfg.num_layers, cfg.hidden_units, cfg.inner_units
    a.dropout, a.attention_dropout, a.type_vocab_size, a.precision = dropout, attention_dropout, 2, prec
    if fused_head is not None:
        a.fused_head = fused_head
    m = BertModel(1, cfg.item_num, a)
    m.load_numpy(P)
    return m


def small_case(L, seed):
    """oracle_case's weights with a batch of three at any L: full, half padded, and a short row."""
    cfg, P, _, _, _ = oracle_case(64, 2, max(L, 246), seed)
    cfg = bo.Cfg(40, L, 64, 2, 1, 96)
    P = dict(P, **{"item_emb.pos_emb.weight": P["item_emb.pos_emb.weight"][:L].copy()})
    r = np.random.RandomState(seed + 2)
    src, dec, lab = (np.zeros((3, L), np.int64) for _ in range(3))
    for b, n in enumerate((L, L // 2, 3)):
        items = r.randint(1, 41, size=n)
        m = r.rand(n) < 0.3
        m[-1] = True
        dec[b, L - n:] = items
        src[b, L - n:] = np.where(m, 41, items)
        lab[b, L - n:] = np.where(m, items, 0)
    return cfg, P, src, dec, lab


def run(m, cfg, batch):
    m.train()
    slots = grads_of(m, cfg, *batch)
    return slots.cpu().numpy().copy(), m.flat_grad.cpu().numpy().copy()


@pytest.mark.parametrize("L", [20, 272])
def test_fused_head_gradients_match_oracle(L):
    cfg, P, src, dec, lab = small_case(L, seed=21) if L < 246 else oracle_case(64, 2, L, seed=21)
    m = build(cfg, P, "bf16", fused_head=True)
    assert m.fused_head
    slots, _ = run(m, cfg, (src, dec, lab))
    loss, _, G = bo.loss_and_grads(P, cfg, src, dec, lab, LAM1, LAM2, training=True, seed=0)
    got = float((slots.sum(1) * np.array([1.0] + LAM1 + LAM2)).sum())
    gmax = max(float(np.abs(G[k]).max()) for k in P)
    worst = (0.0, None)
    for k in P:
        g, want = m.G(k).cpu().numpy(), G[k]
        if "key_transfer.bias" in k:
            assert np.abs(g).max() < 1e-3 * gmax, k
        else:
            fro = np.linalg.norm(g - want) / max(np.linalg.norm(want), 1e-6)
            worst = max(worst, (fro, k))
            assert fro < 0.1, (k, fro)
    print("L %d: loss %.6f (oracle %.6f), worst gradient %s" % (L, got, loss, worst))
    assert abs(got - loss) < 3e-2 * abs(loss)          # the bf16 loss bound of the smoke run (__graft_entry__.py)


def head_calls(monkeypatch):
    """Counts the calls of the two heads' entry points (adt_amd.ops.lce_fwd_bwd: fused; ops.ce_rows: dense)."""
    from adt_amd import ops
    n = {"fused": 0, "dense": 0}
    lce, ce = ops.lce_fwd_bwd, ops.ce_rows

    def spy_lce(*a, **k):
        n["fused"] += 1
        return lce(*a, **k)

    def spy_ce(*a, **k):
        n["dense"] += 1
        return ce(*a, **k)
    monkeypatch.setattr(ops, "lce_fwd_bwd", spy_lce)
    monkeypatch.setattr(ops, "ce_rows", spy_ce)
    return n


def same_path(a, b, what):
    """Two runs of one kernel sequence: the loss slots (no atomics on the way) bit for bit.  flat_grad is NOT reproducible bit for bit even
    between two runs of the same model -- the dense layers' weight gradients are summed with float atomics (tests/test_bert_hip.py:177;
    measured here: an f32 model run twice differs in its last bits) -- so it is held to the bound the suite has for one gradient summed in
    two orders, 1e-4 (tests/test_bert_hip.py::test_dp_shard_equals_slice_of_global_batch); the number of differing entries is printed."""
    assert np.array_equal(a[0], b[0]), what
    print("%s: %d of %d gradient entries differ, rel %.3g" % (what, int((a[1] != b[1]).sum()), a[1].size, rel(a[1], b[1])))
    assert rel(a[1], b[1]) < 1e-4, what


def test_without_the_flag_the_dense_head_runs(monkeypatch):
    """The gate: a d 64 bf16 model without the flag (absent or False) runs the dense head, as with ADT_LCE=0; with it, the fused one."""
    n = head_calls(monkeypatch)
    cfg, P, src, dec, lab = small_case(20, seed=22)
    plain = run(build(cfg, P, "bf16"), cfg, (src, dec, lab))
    off = run(build(cfg, P, "bf16", fused_head=False), cfg, (src, dec, lab))
    assert n == {"fused": 0, "dense": 2}
    monkeypatch.setenv("ADT_LCE", "0")
    m = build(cfg, P, "bf16")
    assert not m.use_lce
    dense = run(m, cfg, (src, dec, lab))
    dense2 = run(build(cfg, P, "bf16", fused_head=True), cfg, (src, dec, lab))          # ADT_LCE=0 overrides the flag
    monkeypatch.delenv("ADT_LCE")
    assert n == {"fused": 0, "dense": 4}
    same_path(dense2, dense, "dense head twice")
    same_path(plain, dense, "no flag against ADT_LCE=0")
    same_path(off, dense, "flag off against ADT_LCE=0")
    fused = run(build(cfg, P, "bf16", fused_head=True), cfg, (src, dec, lab))
    assert n == {"fused": 1, "dense": 4}
    assert not np.array_equal(fused[0][0], dense[0][0])          # another head: the cross-entropy slots differ in their last bits


def test_f32_ignores_the_flag(monkeypatch):
    n = head_calls(monkeypatch)
    cfg, P, src, dec, lab = small_case(20, seed=23)
    a = run(build(cfg, P, "f32"), cfg, (src, dec, lab))
    b = run(build(cfg, P, "f32", fused_head=True), cfg, (src, dec, lab))
    assert n == {"fused": 0, "dense": 2}
    same_path(b, a, "f32 with the flag against without")


def test_graph_replay_equals_eager_with_the_fused_head():
    from adt_amd.bert4rec.trainer import FusedBertTrainer
    cfg, P, src, dec, lab = small_case(20, seed=24)
    outs = []
    for use_graph in (False, True):
        m = build(cfg, P, "bf16", True, 0.3, 0.2)
        tr = FusedBertTrainer(m, LAM1, LAM2, weight_decay=1e-4, use_graph=use_graph, seed=5)
        for _ in range(4):
            tr.step(src, dec, lab)
        torch.cuda.synchronize()
        outs.append((float(tr.loss()), m.flat.cpu().numpy().copy()))
    print("loss %.7f / %.7f, weights %.3g" % (outs[0][0], outs[1][0], rel(outs[1][1], outs[0][1])))
    assert abs(outs[0][0] - outs[1][0]) < 1e-5 * abs(outs[0][0])
    assert rel(outs[1][1], outs[0][1]) < 5e-4
