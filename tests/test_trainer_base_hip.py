"""GPU: the step protocol the trainers inherit -- adt_amd/wide.py:TapeTrainer (WideSasrecTrainer, FusedBertTrainer, FusedStosaTrainer) and
adt_amd/supersearch.py:SupernetTrainer (SuperTrainer, SuperBertTrainer, SuperStosaTrainer) -- at the smallest shapes of the families' own
tests (tools/trainer_launch_sequence.py builds them: one layer, two heads, L = 16), B = 4 and 6, dropout 0.

A first step's loss is a pure forward pass (no float atomics), so where two trainers start from the same seed it is compared bit for bit."""
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tools.trainer_launch_sequence import batches, make  # noqa: E402

TAPE = ["wide", "bert", "stosa"]
SUPER = {"super": ("encoder", "decoder"), "superbert": ("encoder", "decoder"), "superstosa": ("item_encoder", "item_decoder")}


def _loss(tr):
    torch.cuda.synchronize()
    return float(tr.loss())


def _addresses(tr):
    return {k: v.data_ptr() for k, v in tr._st.items() if isinstance(v, torch.Tensor)}


@pytest.mark.parametrize("name", TAPE)
def test_graph_is_rebuilt_when_the_batch_size_changes(name):
    b4, b6 = batches(name, 4, 3), batches(name, 6, 1)
    eager = make(name, False, 0.0)
    eager.step(*b4[0])
    tr = make(name, True, 0.0)
    tr.step(*b4[0])                    # eager warm-up + capture
    assert _loss(tr) == _loss(eager)
    g4, at4 = tr._graph, _addresses(tr)
    assert g4 is not None and tr._st["B"] == 4 and len(at4) >= 4
    tr.step(*b4[1])                    # replay from the same buffers
    assert tr._graph is g4 and _addresses(tr) == at4
    tr.step(*b6[0])
    g6 = tr._graph
    assert g6 is not None and g6 is not g4 and tr._st["B"] == 6
    tr.step(*b4[2])
    assert tr._graph is not None and tr._graph is not g6 and tr._st["B"] == 4
    assert tr.nstep == 4 and float(tr.scal[2]) == 4.0          # every step reached the optimiser once, warm-ups included


@pytest.mark.parametrize("name", sorted(SUPER))
def test_supernet_step_counts_follow_the_block_choice(name):
    from adt_amd import checkpoint as ck
    tr = make(name, dropout=0.0)
    m = tr.model
    data = batches(name, 4, 2)
    selected = []
    for cand, batch in zip(([0.2, 0.7], [0.9, 0.7]), data):       # the same ind interval, neighbouring rec intervals: two of four layers in common
        tr.set_choice(cand)
        selected.append({m.layer_range(kind, 0, idx) for idx in m.shared[0][0] for kind in SUPER[name]})
        tr.step(*batch)
    a, b = selected
    assert a & b and a - b and b - a and (a | b) <= set(tr.steps)
    assert len(tr.steps) > len(a | b)                             # the tensors outside the candidate layers (embeddings, ...)
    for rng, t in tr.steps.items():
        assert t == (1 if rng in a ^ b else 2), (rng, t)

    tr2 = make(name, dropout=0.0)
    tr2.model.set_seed(99)
    ck.load_trainer_state_dict(tr2, ck.trainer_state_dict(tr))
    assert tr2.steps == tr.steps
    assert torch.equal(tr2.m, tr.m) and torch.equal(tr2.v, tr.v) and bool(tr.v.any())
    assert torch.equal(tr2.model._seed, m._seed)


def test_wide_step_staged_equals_step():
    batch = batches("wide", 4, 1)[0]
    a, b = make("wide", dropout=0.0), make("wide", dropout=0.0)
    a.step(*batch)
    b.step_staged(b.stage(*batch))
    assert _loss(a) == _loss(b) and a.nstep == b.nstep == 1
