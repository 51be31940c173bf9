"""CPU: the distance attention at head size 128 where no GPU is needed.

 * adt_wattn_hd128_plan of adt_amd/csrc/adt_wide_plan.h (what adt_wattn_hd128_* / adt_klattn_hd128_* launch with): a stand-alone host
   program (plain g++, no HIP) prints one line per case; the expected lines are restated here from the rules of the header's comment.
   Built and run a second time with -fsanitize=address,undefined, as test_wattn_long_plan_cpu.py does.  adt_wattn_long_plan keeps refusing
   head size 128.
 * oracle/stosa_oracle.py reproduces the five fixtures recorded from the imported reference (tools/gen_golden_stosa.py:main_hd128) at the
   bounds of tests/test_stosa_long_cpu.py: outputs, full-sort distances and the loss 2e-5, gradients 1e-4.
 * _lib.SIGNATURES holds the four new symbols with the argument lists of the *_long_scaled_* entry points."""
import os
import subprocess

import numpy as np
import pytest

from oracle import stosa_oracle as so
from tests.test_stosa_long_cpu import kl_predict_full, oracle_for
from tools.gen_golden_inputs import golden_err

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, "tests", "golden")
F32, BF16 = 0, 1
LDS_MAX = 160 * 1024
HEADS = (64, 128, 256)
LENGTHS = (0, 1, 16, 17, 64, 65, 1024, 1025)
CASES = [(prec, hd, L, bwd) for prec in (F32, BF16) for hd in HEADS for L in LENGTHS for bwd in (0, 1)]
K = 320          # samples per compacted tensor (tools/gen_golden_stosa.py:STOSA_ODD_COMPACT)
FIXTURES = {"hd128": ("stosa_hd128.npz", "wasserstein", (12, 128, 1, 1, 4)), "kl_hd128": ("stosa_kl_hd128.npz", "kl", (12, 128, 1, 1, 4)),
            "w100_h1": ("stosa_w100_h1.npz", "wasserstein", (12, 100, 1, 1, 4)), "kl_w100_h1": ("stosa_kl_w100_h1.npz", "kl", (12, 100, 1, 1, 4)),
            "hd128_h2": ("stosa_hd128_h2.npz", "wasserstein", (20, 256, 2, 2, 3))}

MAIN = r"""
#include <stdio.h>
#include "adt_wide_plan.h"
using namespace adt;
static const int CASES[][4] = {%(cases)s};
int main() {
  for (int i = 0; i < %(ncases)d; ++i) {
    const int* c = CASES[i];
    const AttnPlan p = adt_wattn_hd128_plan(c[0], c[1], c[2], c[3] != 0);
    if (p.error[0]) printf("A %%d error %%s\n", i, p.error);
    else printf("A %%d %%d %%d %%d %%d %%d %%zu\n", i, (int)p.family, p.kc, p.waves, (int)p.csk, p.grid_y, p.lds_bytes);
    const AttnPlan q = adt_wattn_long_plan(c[0], 128, c[2], c[3] != 0);
    printf("L %%d %%s\n", i, q.error[0] ? q.error : "no error");
  }
  const AttnPlan bad = adt_wattn_hd128_plan(7, 128, 64, false);
  printf("P %%s\n", bad.error[0] ? bad.error : "no error");
  return 0;
}
"""


def lds(kc, bwd, hd=128):
    """wattn_long_lds: the cross-term image and its norms, two transposed images (forward); the image, its transpose, two natural and two
    transposed images, LSE and delta of 1024 rows (backward); then 1024 key-validity bytes + 32.  fp32 whatever the precision."""
    cat, t, nat = kc * (2 * hd + 4) + kc, hd * (kc + 4), kc * (hd + 4)
    return 4 * (cat + 2 * t + 2 * nat + 2 * t + 2 * 1024 if bwd else cat + 2 * t) + 1024 + 32


def chunk(bwd):
    """The largest of 64 / 32 rows that leaves room for two workgroups on a CU, else the largest that fits at all."""
    for bound in (LDS_MAX // 2, LDS_MAX):
        for kc in (64, 32):
            if lds(kc, bwd) <= bound:
                return kc
    raise AssertionError("no chunk fits")


def expect(prec, hd, L, bwd):
    """The header's rules: head size, then length; always streamed (family 2), four waves of one 16-row tile, the causal skip on."""
    if hd != 128:
        return "error distance attention at head size 128: head_dim=%d unsupported" % hd
    if L < 1 or L > 1024:
        return "error distance attention at head size 128: L=%d outside 1..1024" % L
    kc = chunk(bwd)
    return "2 %d 4 1 %d %d" % (kc, -(-(-(-L // 16)) // 4), lds(kc, bwd))


@pytest.fixture(scope="module", params=[[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g", "-O1"]], ids=["plain", "asan-ubsan"])
def table(request, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("wattn_hd128_plan")
    src, exe = tmp / "wattn_hd128_plan_main.cpp", tmp / "wattn_hd128_plan_main"
    src.write_text(MAIN % dict(cases=", ".join("{%d, %d, %d, %d}" % c for c in CASES), ncases=len(CASES)))
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(REPO, "adt_amd", "csrc")] +
                          request.param + ["-o", str(exe), str(src)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60,
                         env=dict(os.environ, ASAN_OPTIONS="abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1"))
    assert out.returncode == 0 and "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-3000:]
    lines = {}
    for line in out.stdout.splitlines():
        lines.setdefault(line[0], []).append(line)
    return lines


def test_plan_matches_the_restated_rules(table):
    assert len(table["A"]) == len(CASES)
    for i, (case, line) in enumerate(zip(CASES, table["A"])):
        want = "A %d %s" % (i, expect(*case))
        assert line.startswith(want) if " error " in want else line == want, (case, line)
    assert table["P"] == ["P distance attention at head size 128: prec=7 unsupported"]


def test_errors_exactly_at_head_sizes_64_and_256_and_lengths_0_and_1025(table):
    for case, line in zip(CASES, table["A"]):
        assert (" error " in line) == (case[1] in (64, 256) or case[2] in (0, 1025)), (case, line)
    # head size 256 says why it is refused; 64 where it runs
    assert all("LDS" in line and "registers" in line for case, line in zip(CASES, table["A"]) if case[1] == 256)
    assert all("_long" in line for case, line in zip(CASES, table["A"]) if case[1] == 64)


def test_every_footprint_fits_the_lds_and_does_not_depend_on_the_precision(table):
    sizes = {case: int(line.split()[-1]) for case, line in zip(CASES, table["A"]) if " error " not in line}
    assert sizes and max(sizes.values()) <= LDS_MAX
    for (prec, hd, L, bwd), n in sizes.items():
        assert n == sizes[(1 - prec, hd, L, bwd)]
    # the three footprints a chunk of whole tile pairs can have at this head size; the backward has no choice
    assert (lds(64, False), lds(32, False), lds(32, True)) == (137504, 71328, 150176) and lds(64, True) > LDS_MAX
    assert set(sizes.values()) == {lds(chunk(False), False), lds(32, True)}


def test_grid_covers_the_tiles_four_per_workgroup(table):
    got = {case[2]: int(line.split()[-2]) for case, line in zip(CASES, table["A"]) if " error " not in line}
    assert got == {1: 1, 16: 1, 17: 1, 64: 1, 65: 2, 1024: 16}
    for L, gy in got.items():
        assert gy * 4 * 16 >= L > (gy - 1) * 4 * 16


def test_the_long_plan_still_refuses_head_size_128(table):
    assert len(table["L"]) == len(CASES)
    for line in table["L"]:
        assert "head_dim=128 unsupported (16/32/64)" in line, line


# ---- the fixtures ---------------------------------------------------------------------------------------------------------------------
def load_case(tag):
    """The seeded weights of tools/gen_golden_stosa.py:reference_model: Linear biases away from zero, cov_query / cov_key biases shifted by
    the fixture's cov_qk_bias where it has one (stosa_kl_hd128: the reference's product of 128 covariances overflows without it)."""
    g = np.load(os.path.join(GOLD, FIXTURES[tag][0]))
    V, L, d, H, nl, nu = [int(x) for x in g["cfg"]]
    cfg = so.Cfg(V, L, d, H, nl, num_users=nu, pvn_weight=float(g["pvn_weight"]))
    P = so.init_params(cfg, int(g["seed"]))
    r = np.random.RandomState(int(g["seed"]) + 1)
    shift = np.float32(g["cov_qk_bias"]) if "cov_qk_bias" in g.files else np.float32(0)
    for k in P:
        if k.endswith(".bias") and "LayerNorm" not in k:
            P[k] = (0.02 * r.standard_normal(P[k].shape)).astype(np.float32)
            if k.endswith(("cov_query.bias", "cov_key.bias")):
                P[k] += shift
    return g, cfg, P


@pytest.fixture(scope="module", params=list(FIXTURES))
def run(request):
    """One forward and one loss / gradient pass of the oracle per fixture, shared by the tests below."""
    tag = request.param
    metric = FIXTURES[tag][1]
    g, cfg, P = load_case(tag)
    lam1, lam2 = list(g["lambda1"]), list(g["lambda2"])
    with oracle_for(metric):
        fin = so.finetune(P, cfg, g["input_ids"], g["dec_ids"], training=False)
        if metric == "kl":
            full = kl_predict_full(fin[0][:, -1, :], fin[1][:, -1, :], P["item_mean_embeddings.weight"], P["item_cov_embeddings.weight"])
        else:
            full = so.predict_full(P, cfg, g["input_ids"], g["dec_ids"])
        lg = so.loss_and_grads(P, cfg, g["input_ids"], g["dec_ids"], g["pos_ids"], g["neg_ids"], lam1, lam2, training=True, seed=0)
    return tag, g, cfg, P, fin, full, lg


def test_fixture_shape_and_size(run):
    tag, g, cfg, P, _, _, _ = run
    name, metric, (L, d, H, nl, B) = FIXTURES[tag]
    assert (cfg.maxlen, cfg.hidden_units, cfg.num_heads, cfg.num_layers) == (L, d, H, nl) and g["input_ids"].shape == (B, L)
    assert cfg.item_size == (33 if tag == "hd128_h2" else 42)
    assert os.path.getsize(os.path.join(GOLD, name)) < 300 * 1024
    assert all(np.isfinite(g[k]).all() for k in g.files if g[k].dtype.kind == "f")
    assert ("cov_qk_bias" in g.files) == (tag == "kl_hd128")


def test_finetune_and_full_sort_match_reference(run):
    tag, g, cfg, P, (m, c, enc_in, enc_rec, dec_out), full, _ = run
    figs = {"mean_out": golden_err(m, g, "mean_out", K), "cov_out": golden_err(c, g, "cov_out", K), "full_dist": golden_err(full, g, "full_dist", K)}
    for i in range(cfg.num_layers):
        for nm, pair in (("enc_in", enc_in[i]), ("rec", enc_rec[i]), ("dec_out", dec_out[i])):
            for t, which in enumerate(("mean", "cov")):
                figs["%s_%s_%d" % (nm, which, i)] = golden_err(pair[t], g, "%s_%s_%d" % (nm, which, i), K)
    print(tag, figs)
    for k, e in figs.items():
        assert e < 2e-5, (k, e)


def test_loss_and_gradients_match_reference(run):
    tag, g, cfg, P, _, _, (loss, parts, G) = run
    assert abs(loss - float(g["loss"])) < 2e-5 * abs(float(g["loss"]))
    assert abs(parts["bpr"] - float(g["bpr"])) < 2e-5 * abs(float(g["bpr"])) and abs(parts["auc"] - float(g["auc"])) < 1e-6
    assert abs(parts["pvn"] - float(g["pvn"])) < 2e-5 * max(abs(float(g["pvn"])), 1e-6)
    assert sorted(k for k in P if G[k] is None) == sorted(str(x) for x in g["grad_none"])
    figs = {k: golden_err(G[k], g, "grad." + k, K) for k in P if G[k] is not None}
    print(tag, "largest gradient error", max(figs.values()))
    for k, e in figs.items():
        assert e < 1e-4, (k, e)


# ---- the C ABI's Python side ------------------------------------------------------------------------------------------------------------
def test_signatures_are_the_scaled_argument_lists():
    from adt_amd import _lib
    S = _lib.SIGNATURES
    for d in ("fwd", "bwd"):
        for new, old in (("adt_wattn_hd128_%s" % d, "adt_wattn_long_scaled_%s" % d), ("adt_klattn_hd128_%s" % d, "adt_klattn_long_scaled_%s" % d)):
            assert new in S and S[new] == S[old], new
    header = open(os.path.join(REPO, "include", "adt_hip.h")).read()
    for name in ("adt_wattn_hd128_fwd", "adt_wattn_hd128_bwd", "adt_klattn_hd128_fwd", "adt_klattn_hd128_bwd"):
        assert "int %s(int prec," % name in header
        decl = header[header.index("int %s(" % name):]
        assert "float scale, int hd_live" in decl[:decl.index(";")]


def test_constructor_takes_the_flag_off_by_default():
    import inspect
    from adt_amd.stosa import main as stosa_main
    from adt_amd.stosa.models import DisenDistSAModel
    assert inspect.signature(DisenDistSAModel.__init__).parameters["allow_wide_heads"].default is False
    assert "allow_wide_heads=True" in inspect.getsource(stosa_main.main)
