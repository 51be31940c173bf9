#!/usr/bin/env python3
"""What the device sees from three steps of one trainer: the evidence that a change to the trainers' HOST code left the launches alone.

    python tools/trainer_launch_sequence.py NAME            # NAME: wide bert stosa super superbert superstosa flagship flagship-ring
    rocprofv3 --kernel-trace --output-format csv -d out -o NAME -- python3 tools/trainer_launch_sequence.py NAME
    python tools/trainer_launch_sequence.py --digest out/NAME_kernel_trace.csv

The run seeds torch, builds the smallest model of the family (one layer, two heads, B = 4, L = 16, dropout on), and steps three times on
fixed random ids, printing the loss after every step as decimal and as float.hex() (bit-for-bit comparable).  The three launch-tape
trainers run twice in the process, eagerly and with use_graph=True (eager warm-up, capture, replay, replay); the supernet trainers
have no graph mode and change their block choice between the steps.  Only public constructors and step() are used, so the same file
runs on an older checkout.  --digest prints the length and the SHA-256 of the trace's ordered kernel list, by name alone and with grid
and workgroup sizes (and the LDS bytes of each dispatch, where the trace has the column); two checkouts launched the same work when the
digests agree.  One trainer per process.

flagship / flagship-ring: the fused SASRec-ADT step (FusedTrainer, width 64) on ids resident in HBM (stage_ring / step_staged), and through the
pinned id ring (slot / publish / commit) with every batch published one ahead, so each step prefetches its successor and the next takes it
from the staging buffer.  After each step they also print a SHA-256 of the gradient behind the two tables (float atomics order the table
rows' sums by arrival; the learning rate is 0 there, so that order does not reach the weights) -- under ADT_ITEM_SORT=1, where the whole step
is deterministic and Adam runs, of the whole gradient and of the weights instead.
A step that launches kernels on two streams has no fixed dispatch order across them: --digest therefore prints a second, order-independent
pair of hashes, taken over the sorted lines.
"""
import csv
import hashlib
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

V, L, B, STEPS = 40, 16, 4, 3
NAMES = ("wide", "bert", "stosa", "super", "superbert", "superstosa", "flagship", "flagship-ring")
CHOICE = [0.0, 0.5, 1.0]
CANDS = [[0.2, 0.7], [0.9, 0.1], [0.2, 0.7]]         # steps 1 and 3 share a block choice, step 2 selects other candidate layers


class Args:
    pass


def _args(dropout, **kw):
    a = Args()
    a.device, a.maxlen, a.num_heads, a.num_layers, a.precision = "cuda:0", L, 2, 1, "bf16"
    a.dropout, a.attention_dropout = dropout, dropout
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def sasrec_batches(r, B, n):
    out = []
    for _ in range(n):
        seq = r.randint(1, V + 1, size=(B, L))
        seq[:, :3] = 0
        dec = np.roll(seq, 1, 1)
        dec[:, 0] = 0
        out.append((seq, dec, r.randint(1, V + 1, size=(B, L)) * (seq > 0), r.randint(1, V + 1, size=(B, L)) * (seq > 0)))
    return out


def bert_batches(r, B, n):
    out = []
    for _ in range(n):
        items = r.randint(1, V + 1, size=(B, L))
        mask = r.rand(B, L) < 0.3
        mask[:, -1] = True
        out.append((np.where(mask, V + 1, items), items, np.where(mask, items, 0)))
    return out


def batches(name, B=B, n=STEPS, seed=7):
    """n batches of B sequences in the argument order of the trainer's step()."""
    return (bert_batches if "bert" in name else sasrec_batches)(np.random.RandomState(seed), B, n)


def make(name, use_graph=False, dropout=0.2):
    """A fresh model and trainer of one family; every call starts from the same torch seed."""
    import torch
    torch.manual_seed(23)
    if name == "wide":          # width 50 runs padded to 64 lanes: the push / pull of the reference-shaped parameters is part of the step
        from adt_amd.sasrec.model_wide import SASRecADTWide, WideSasrecTrainer
        m = SASRecADTWide(1, V, _args(dropout, hidden_units=50))
        return WideSasrecTrainer(m, [0.1], [0.05], weight_decay=1e-3, use_graph=use_graph, seed=3)
    if name.startswith("flagship"):
        from adt_amd.sasrec.model import SASRecADT
        from adt_amd.sasrec.trainer import FusedTrainer
        m = SASRecADT(1, V, _args(dropout, hidden_units=64))
        # (the table rows are summed by float atomics in arrival order: with a learning rate they would carry that order into the weights and
        # so into every later gradient; the sorted form is deterministic and keeps Adam on)
        lr = 1e-3 if os.environ.get("ADT_ITEM_SORT", "0") != "0" else 0.0
        return FusedTrainer(m, [0.1], [0.05], lr=lr, weight_decay=1e-3, use_graph=use_graph, seed=3)
    if name == "bert":
        from adt_amd.bert4rec.model import BertModel
        from adt_amd.bert4rec.trainer import FusedBertTrainer
        m = BertModel(1, V, _args(dropout, hidden_units=64, inner_units=128, type_vocab_size=2))
        return FusedBertTrainer(m, [0.2], [0.1], weight_decay=1e-4, use_graph=use_graph, seed=3)
    if name == "stosa":
        from adt_amd.stosa.models import DisenDistSAModel
        from adt_amd.stosa.trainer import FusedStosaTrainer
        m = DisenDistSAModel(_args(dropout, hidden_units=64, item_size=V + 2, num_users=4, pvn_weight=0.005, distance_metric="wasserstein"))
        return FusedStosaTrainer(m, [0.2], [0.1], use_graph=use_graph, seed=3)
    if name == "super":
        from adt_amd.sasrec.supersasrec import SuperSASRecModel, SuperTrainer
        m = SuperSASRecModel(1, V, CHOICE, CHOICE, _args(dropout, hidden_units=64))
        return SuperTrainer(m, weight_decay=1e-4, seed=3)
    if name == "superbert":
        from adt_amd.bert4rec.superbert import SuperBertModel, SuperBertTrainer
        m = SuperBertModel(1, V, CHOICE, CHOICE, _args(dropout, hidden_units=64, inner_units=256, type_vocab_size=2))
        return SuperBertTrainer(m, seed=3)
    if name == "superstosa":
        from adt_amd.stosa.supernet import DisenDistSASupernet, SuperStosaTrainer
        m = DisenDistSASupernet(_args(dropout, hidden_units=64, item_size=V + 2, num_users=4, pvn_weight=0.005, distance_metric="wasserstein"), CHOICE, CHOICE)
        return SuperStosaTrainer(m, seed=3)
    raise SystemExit("unknown trainer %r" % name)


def run(name):
    import torch
    supernet = name.startswith("super")
    for mode in (("eager",) if supernet else ("eager", "graph")):
        tr = make(name, mode == "graph")
        for i, batch in enumerate(batches(name)):
            if supernet:
                tr.set_choice(CANDS[i])
            tr.step(*batch)
            torch.cuda.synchronize()
            loss = float(tr.loss())
            print("%s %s step %d loss %.9g %s" % (name, mode, i + 1, loss, loss.hex()), flush=True)


def run_flagship(name):
    import torch
    sort = os.environ.get("ADT_ITEM_SORT", "0") != "0"
    sha = lambda t: hashlib.sha256(t.detach().cpu().numpy().tobytes()).hexdigest()
    for mode in ("eager", "graph"):
        tr = make(name, mode == "graph")
        m, bs = tr.model, batches(name)
        if name == "flagship":
            ring = tr.stage_ring(bs)

        def produce(i):
            views, _ = tr.slot(B, i)
            for v, a in zip(views, bs[i]):
                v[...] = a
            tr.publish(B, i, (float(np.count_nonzero(bs[i][2])), float(B * L * m.hidden_units), float(B * L * m.num_heads)))
        if name == "flagship-ring":
            produce(0)
        for i in range(STEPS):
            if name == "flagship":
                tr.step_staged(ring)
            else:
                if i + 1 < STEPS:
                    produce(i + 1)      # published before this step is committed: the step prefetches it
                tr.commit(B)
            torch.cuda.synchronize()
            loss = float(tr.loss())
            print("%s %s step %d loss %.9g %s" % (name, mode, i + 1, loss, loss.hex()), flush=True)
            if sort:
                print("%s %s step %d grad sha256 %s weights sha256 %s" % (name, mode, i + 1, sha(m.flat_grad), sha(m.flat)), flush=True)
            else:
                print("%s %s step %d non-table grad sha256 %s" % (name, mode, i + 1, sha(m.flat_grad[m.offsets[2]:])), flush=True)
        if name == "flagship-ring":
            print("%s %s batches taken from staging %d" % (name, mode, int(tr._st["state"][5])), flush=True)


def digest(path):
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Dispatch_Id"]))
    names = [r["Kernel_Name"] for r in rows]
    sized = ["%s grid %s,%s,%s workgroup %s,%s,%s" % ((r["Kernel_Name"],) + tuple(r[k + a] for k in ("Grid_Size_", "Workgroup_Size_") for a in "XYZ"))
             for r in rows]
    lds = next((k for k in ("LDS_Block_Size", "Group_Segment_Size") if rows and k in rows[0]), None)      # static + dynamic LDS of the dispatch, where the trace has it
    if lds:
        sized = ["%s lds %s" % (line, r[lds]) for line, r in zip(sized, rows)]
    sha = lambda lines: hashlib.sha256("\n".join(lines).encode()).hexdigest()
    what = "names+grid+workgroup+lds" if lds else "names+grid+workgroup"
    print("%s: %d kernels, names sha256 %s, %s sha256 %s" % (os.path.basename(path), len(rows), sha(names), what, sha(sized)))
    print("%s: order-independent: names sha256 %s, %s sha256 %s" % (os.path.basename(path), sha(sorted(names)), what, sha(sorted(sized))))


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--digest":
        digest(sys.argv[2])
    elif len(sys.argv) == 2:
        (run_flagship if sys.argv[1].startswith("flagship") else run)(sys.argv[1])
    else:
        raise SystemExit(__doc__)
