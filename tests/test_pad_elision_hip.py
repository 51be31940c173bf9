"""The pad prefix handed to the per-sequence chain kernels (SeqFwdArgs / SeqBwdArgs / BwdChainArgs / AttnArgs::pad_pre; StepPlan::pad_elide,
ADT_PAD_ELIDE) against the same step without it (ADT_PAD_ELIDE=0).  A kernel that knows the prefix requests no row of a 16-token tile inside it
whose value is an exact zero or only ever multiplies one ("Pad prefix": the table of streams), so the standard is EQUALITY of
everything a training step leaves behind -- loss, gradient, gradient norm, weights, both Adam moments -- not a tolerance.  Equality is that of
numpy.array_equal (a substituted +0.0 equals a stored -0.0): the hashes compared are those of the arrays with +0.0 added; whether the raw bytes
agree as well is printed.

ADT_PAD_ELIDE is read once per process, so each arm is a fresh child process (ADT_ITEM_SORT=1: bit-reproducible table gradients).  A child
builds small SASRecADT bf16 models, runs three FusedTrainer steps per case and reports the hashes after every step and how many launches of a
chain kernel were given the prefixes.

Shapes: L 48 is three whole tiles, L 40 has a partial last tile (l < L and the prefix meet in one tile); eight rows, each with its own prefix
length, among them 0, a whole tile, one short of and one beyond a tile boundary, and an all-padding row; one row has a zero id in the middle
of its history (it must not extend the prefix); the decoder ids are the encoder's shifted by one, as the sampler makes them, so the two
stacks' prefixes differ by one and lie on two sides of a tile boundary in the rows with 15, 31 / 32 and 47 leading zeros."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NITEMS, NSTEPS, NL, B = 50, 3, 2, 8
PREFIX = {48: [0, 1, 15, 16, 17, 32, 47, 48], 40: [0, 7, 16, 24, 32, 39, 40, 15]}
HOLE_ROW = 1          # the row whose history holds a zero id (prefix 1 at L 48, 7 at L 40)
# (H, L, dropout): head sizes 64, 32 and 16 are separate instantiations
DROP = [(H, L, 0.5) for L in (48, 40) for H in (1, 2, 4)]
NODROP = [(2, 48, 0.0), (1, 40, 0.0)]
# setting -> (ADT_SEQ_SPLIT or None, cases).  The benchmarked batch runs one workgroup per sequence, where the decoder's cross-attention
# backward and its mid chain are one launch (k_seqtt_xattn_mid_bwd); a batch of eight would run eight per sequence if left alone.
SETTINGS = {
    "one_wg": ("1", DROP + NODROP),
    "split2": ("2", [(2, 48, 0.5), (1, 40, 0.5), (4, 40, 0.5)]),      # two workgroups per sequence in every chain kernel, k_seqtt_attn_pre_bwd included
    "split_by_batch": (None, [(2, 48, 0.5), (2, 40, 0.5)]),           # eight per sequence: more workgroups than tiles
}
KEYS = ("loss", "grad", "grad_norm", "weights", "adam_m", "adam_v")


def _batch(r, L):
    seq, dec, pos, neg = (np.zeros((B, L), np.int32) for _ in range(4))
    for b, pre in enumerate(PREFIX[L]):
        n = L - pre
        items = r.randint(1, NITEMS + 1, size=n + 1)
        seq[b, pre:] = items[:-1]
        pos[b, pre:] = items[1:]
        neg[b, pre:] = r.randint(1, NITEMS + 1, size=n)
    hole = (PREFIX[L][HOLE_ROW] + L) // 2
    seq[HOLE_ROW, hole] = 0
    dec[:, 1:] = seq[:, :-1]
    lead = lambda ids: [int(np.argmax(row != 0)) if row.any() else L for row in ids]      # noqa: E731
    assert lead(seq) == PREFIX[L] and lead(dec) == [min(L, p + 1) for p in PREFIX[L]] and np.count_nonzero(seq[HOLE_ROW, hole:]) > 0
    return seq, dec, pos, neg


def _hashes(t):
    a = np.ascontiguousarray(t.detach().float().cpu().numpy())
    return hashlib.sha256((a + 0.0).tobytes()).hexdigest(), hashlib.sha256(a.tobytes()).hexdigest()


def _child(runs, out_path):
    """Runs in the child process: every (case, poison) of `runs`, three steps each.  poison: the whole workspace is NaN before every step, but
    for the optimizer's scalars (the step count lives there from step to step)."""
    import ctypes
    import torch
    from adt_amd import _lib
    from adt_amd.sasrec import model as mm
    from adt_amd.sasrec.trainer import FusedTrainer

    lib = _lib.load()
    lib.adt_seq_pad_elide_launches.restype = ctypes.c_ulonglong
    lib.adt_seq_pad_elide_launches.argtypes = []
    result = {"runs": [], "launches": []}
    for (H, L, p), poison in runs:
        class Args:
            device, maxlen, num_heads, num_layers, precision, hidden_units, dropout = "cuda:0", L, H, NL, "bf16", 64, p
        ci = 100 * H + L
        torch.manual_seed(ci)
        m = mm.SASRecADT(1, NITEMS, Args())
        assert m.lib.adt_seq_layer_supported(1, L, 64, 64 // H) == 1, (H, L)
        m.train()
        tr = FusedTrainer(m, [0.1] * NL, [0.05] * NL, weight_decay=1e-3, seed=7 + ci)
        r = np.random.RandomState(1000 + ci)
        before = int(lib.adt_seq_pad_elide_launches())
        steps = []
        for _ in range(NSTEPS):
            if poison:
                torch.cuda.synchronize()
                scal = m.ws_view(B, mm.WS_SCAL, 0, 192).clone()
                m.workspace(B).fill_(float("nan"))
                m.ws_view(B, mm.WS_SCAL, 0, 192).copy_(scal)
            tr.step(*_batch(r, L))
            torch.cuda.synchronize()
            got = {"loss": tr.loss(), "grad": m.flat_grad, "grad_norm": tr.grad_norm(), "weights": m.flat, "adam_m": tr.m, "adam_v": tr.v}
            step = {"finite": all(bool(torch.isfinite(v).all()) for v in got.values())}
            for k, v in got.items():
                step[k], step[k + "_raw"] = _hashes(v)
            steps.append(step)
        result["runs"].append(steps)
        result["launches"].append(int(lib.adt_seq_pad_elide_launches()) - before)
    with open(out_path, "w") as f:
        json.dump(result, f)
    return True


def _run_arm(elide, split, runs, tmp, tag):
    out = os.path.join(str(tmp), "pad_%s.json" % tag)
    env = dict(os.environ, ADT_ITEM_SORT="1")
    for k in ("ADT_PAD_ELIDE", "ADT_SEQ_SPLIT", "ADT_XATTN_FUSED", "ADT_DO_BF16"):
        env.pop(k, None)
    if split is not None:
        env["ADT_SEQ_SPLIT"] = split
    if not elide:
        env["ADT_PAD_ELIDE"] = "0"
    code = ("import sys; sys.path.insert(0, %r); from tests.test_pad_elision_hip import _child; assert _child(%r, %r); print('pad-child-ok')"
            % (REPO, runs, out))
    p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "pad-child-ok" in p.stdout, p.stdout[-2000:] + p.stderr[-3000:]
    with open(out) as f:
        return json.load(f)


_ARMS = {}


def _arms(setting, tmp_path_factory):
    """Both arms of a setting, run once and shared by the tests that read them."""
    if setting not in _ARMS:
        split, cases = SETTINGS[setting]
        tmp = tmp_path_factory.mktemp("pad_" + setting)
        runs = [(c, False) for c in cases]
        _ARMS[setting] = (_run_arm(False, split, runs, tmp, "off"), _run_arm(True, split, runs, tmp, "on"))
    return _ARMS[setting]


def _compare(name, cases, a, b):
    raw_equal = True
    for case, ra, rb in zip(cases, a, b):
        for k, (sa, sb) in enumerate(zip(ra, rb)):
            assert sa["finite"] and sb["finite"], (name, case, k)
            diff = [key for key in KEYS if sa[key] != sb[key]]
            raw = [key for key in KEYS if sa[key + "_raw"] != sb[key + "_raw"]]
            raw_equal = raw_equal and not raw
            if raw and not diff:
                print("%s case %s step %d: equal, raw bytes differ (the sign of a zero) in %s" % (name, case, k + 1, raw))
            assert not diff, "%s case %s step %d: %s differ" % (name, case, k + 1, diff)
    print("%s: every array equal; raw bytes %s" % (name, "agree too" if raw_equal else "differ in the sign of zeros"))


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_step_is_equal_with_and_without_pad_elision(setting, tmp_path_factory):
    """Loss, gradient, gradient norm, weights and both Adam moments after each of three steps of every case are equal between ADT_PAD_ELIDE=0
    and the default."""
    off, on = _arms(setting, tmp_path_factory)
    _compare(setting, SETTINGS[setting][1], off["runs"], on["runs"])


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_counter_shows_elision_in_the_default_arm_only(setting, tmp_path_factory):
    """The launches that were given the prefixes: none with ADT_PAD_ELIDE=0; in the default arm both stacks' forward kernels of every layer and,
    per layer, k_seqtt_post_bwd of both stacks, k_seqtt_attn_pre_bwd of both and -- one workgroup per sequence only -- k_seqtt_xattn_mid_bwd, in
    every step.  Not with 16-wide heads: StepPlan::pad_elide leaves those instantiations as they are (adt_step_plan.h)."""
    off, on = _arms(setting, tmp_path_factory)
    split, cases = SETTINGS[setting]
    per_step = NL * (7 if split == "1" else 6)
    print("launches with the prefixes: %s (default arm), %s (ADT_PAD_ELIDE=0 arm)" % (on["launches"], off["launches"]))
    assert off["launches"] == [0] * len(cases)
    assert on["launches"] == [0 if H == 4 else NSTEPS * per_step for (H, _, _) in cases]


def test_poisoned_workspace_changes_nothing(tmp_path_factory):
    """Default arm, the whole workspace NaN before every step (but the optimizer's scalars): equal to a clean workspace.  A store dropped while a
    reader still loads, or a load replaced by anything but its known value, leaves a NaN or a stale row behind: this is the test that sees it."""
    cases = [(2, 48, 0.5), (2, 40, 0.5), (1, 48, 0.5), (2, 40, 0.0)]
    tmp = tmp_path_factory.mktemp("pad_poison")
    res = _run_arm(True, "1", [(c, False) for c in cases] + [(c, True) for c in cases], tmp, "poison")
    assert all(n > 0 for n in res["launches"])
    _compare("poisoned workspace", cases, res["runs"][:len(cases)], res["runs"][len(cases):])
