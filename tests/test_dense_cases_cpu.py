"""CPU: the case table of tests/dense_cases.py reaches every dense-layer kernel instantiation and loop regime that adt_dense_fwd_plan / adt_dense_bwd_plan
can choose.  The plan is read through its Python restatement (expect_fwd, expect_dx, expect_dw of test_wide_plan_cpu.py); a stand-alone program
holds the restatement against adt_wide_plan.h at every point of the domain the enumeration walks.  Also: the float64 reference of the GPU tests
against the float32 tape oracle, and bf16_round against torch.

Keys and instantiations.  A key (dense_cases.key) names the kernel template instantiation and the loop regime; every reachable key must be hit by a
case.  The epilogue features rotate over the shapes of one instantiation (inst() below: the key without its loop-regime part), so what the
rotation must still deliver is asserted per instantiation: every value of a feature that can reach it in the domain -- dropout off and on, an
activation and none, beta both ways, R, R2, the row mask and t_dev present -- and "saved U without an activation" once per forward arm."""
import itertools
import os
import subprocess

import numpy as np
import pytest

import dense_cases as dc
from test_wide_plan_cpu import BF16, F32, FACT_FIELDS, expect_dw, expect_dx, expect_fwd

MAX_CASES = 128      # "about 120"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FWD_LAYOUTS = ("aligned", "Y+ld", "Y+off", "U+ld", "U+off", "R+ld", "R+off", "R2+ld", "R2+off", "bias+off")
BWD_LAYOUTS = ("aligned", "U+ld", "U+off", "dX+ld", "dX+off")
ROW_TILE = {"F256": 32, "FROWS": 16, "FTILED": 128, "DX256": 32, "DXROWS": 16, "DXTILED": 128, "DW256": 32, "DWROWS": 64, "DW64": 128, "DWTILED": 32}


def present(kw, layout):
    op = layout.split("+")[0]
    return op == "aligned" or {"Y": 1, "U": kw["save_u"], "R": kw["R"], "R2": kw["R2"], "bias": kw["bias"], "dX": 1}[op]


def domain():
    """Every (case, direction) of prec x K x N x the T regimes x presence flags x layout tags x workspace on / off.  Forward cases ask for no gradient;
    backward cases for all three (the two halves of the backward plan are independent).  The forward key depends on T at K = 256 only
    (k_dense_fwd256's chunk), so the other K run at one T.  t_dev is no fact of the plan: it is put on for half of the points."""
    n = 0
    for prec, K, N in itertools.product((F32, BF16), dc.K_SET, dc.N_SET):
        for T in (dc.T_REGIMES if K == 256 else dc.T_REGIMES[1:2]):
            for act, save_u, p, bias, R, R2, mask in itertools.product((dc.ACT_NONE, dc.ACT_GELU), (0, 1), (0.0, dc.P_DROP), (0, 1), (0, 1), (0, 1), (0, 1)):
                kw = dict(act=act, save_u=save_u, p=p, bias=bias, R=R, R2=R2, mask=mask)
                for layout in FWD_LAYOUTS:
                    if present(kw, layout):
                        n += 1
                        yield dc.case(prec, T, K, N, want="", layout=layout, t_dev=n & 1, **kw), "fwd"
        for T in dc.T_REGIMES:
            for act, save_u, p, mask, beta, ws in itertools.product((dc.ACT_NONE, dc.ACT_GELU), (0, 1), (0.0, dc.P_DROP), (0, 1), (0, 1), ("registered", "none")):
                if act and not save_u:
                    continue
                kw = dict(act=act, save_u=save_u, p=p, mask=mask, beta=beta, ws=ws, R=0, R2=0, bias=0)
                for layout in BWD_LAYOUTS:
                    if present(kw, layout):
                        n += 1
                        yield dc.case(prec, T, K, N, want="xwb", layout=layout, t_dev=n & 1, **kw), "bwd"


def inst(key):
    """The template instantiation of a key: the key without its loop regime (and, for the two stage kernels of the weight gradient and the
    256 x 128-block one, without the block layout: one kernel each; k_dense_dw64 with and without partials)."""
    n = {"F256": 2, "FROWS": 3, "FTILED": 3, "DX256": 2, "DXROWS": 2, "DXTILED": 3, "DW256": 1, "DWROWS": 1, "DWTILED": 3}.get(key[0])
    return ("DW64", key[3]) if key[0] == "DW64" else key[:n]


def features(c, which):
    """What a case shows the kernel of one of its thirds: {feature: value}."""
    act = c.act != dc.ACT_NONE
    f = dict(drop=bool(dc.has_drop(c)), mask=bool(c.mask), t_dev=bool(c.t_dev))
    if which == "fwd":
        f.update(act="act" if act else ("save_u" if c.save_u else "none"), R=bool(c.R), R2=bool(c.R2))
    else:
        f.update(act="act" if act else "none")
        if which == "dx":
            f.update(beta=bool(c.beta))
    return f


_KEYS = {}


def thirds(c):
    """[(which, key)] of a case, memoised."""
    if c not in _KEYS:
        _KEYS[c] = [(w, k) for w, k in ((w, dc.key(c, w)) for w in (("fwd",) if not c.want else ("fwd", "dx", "dw"))) if k is not None]
    return _KEYS[c]


def walk(points):
    """({key: {feature: values seen}}, {direction: the distinct facts}) of (case, direction) points."""
    reach, seen = {}, {"fwd": set(), "bwd": set()}
    for c, direction in points:
        f = dc.facts(c, direction)
        seen[direction].add(tuple(f[k] for k in FACT_FIELDS))
        for which, k in ((("fwd", dc.key_fwd(f)),) if direction == "fwd" else (("dx", dc.key_dx(f)), ("dw", dc.key_dw(f)))):
            if k is None:
                continue
            slot = reach.setdefault(k, {})
            for name, v in features(c, which).items():
                slot.setdefault(name, set()).add(v)
    return reach, seen


def hits(cases):
    return walk((c, d) for c in cases for d in (("fwd", "bwd") if c.want else ("fwd",)))[0]


def merged(by_key):
    """{instantiation: {feature: values}} of a {key: {feature: values}}."""
    out = {}
    for k, feats in by_key.items():
        slot = out.setdefault(inst(k), {})
        for name, vals in feats.items():
            slot.setdefault(name, set()).update(vals)
    return out


def gaps(reach, cases):
    """What the case list leaves uncovered: (key, "no case"), (instantiation, feature, value), (arm, "act", "save_u")."""
    seen = hits(cases)
    out = [(k, "no case") for k in sorted(reach, key=repr) if k not in seen]
    want, got = merged(reach), merged(seen)
    for i in sorted(want, key=repr):
        for name, vals in sorted(want[i].items()):
            for v in sorted(vals, key=repr):
                if name == "act" and v == "save_u":
                    continue      # once per arm, below
                if name in ("R", "R2", "mask", "t_dev") and v is False:
                    continue      # present at least once; absent is the default everywhere
                if v not in got.get(i, {}).get(name, ()):
                    out.append((i, name, v))
    for arm in ("F256", "FROWS", "FTILED"):
        if not any("save_u" in f.get("act", ()) for k, f in seen.items() if k[0] == arm):
            out.append((arm, "act", "save_u"))
    return out


@pytest.fixture(scope="module")
def world():
    return walk(domain())


@pytest.fixture(scope="module")
def reach(world):
    return world[0]


PLAN_MAIN = r"""
#include <stdio.h>
#include "adt_wide_plan.h"
using namespace adt;
int main() {
  static const char* const FA[] = {"F256", "FROWS", "FTILED"};
  static const char* const DX[] = {"DXNONE", "DX256", "DXROWS", "DXTILED"};
  static const char* const DW[] = {"DWNONE", "DW256", "DWROWS", "DW64", "DWTILED"};
  char dir;
  long long v[25];
  for (;;) {
    if (scanf(" %c", &dir) != 1) break;
    for (int i = 0; i < 25; ++i) if (scanf("%lld", &v[i]) != 1) return 2;
    DenseFacts f{};
    f.prec = (int)v[0]; f.T = (int)v[1]; f.K = (int)v[2]; f.N = (int)v[3];
    f.has_bias = v[4]; f.has_u = v[5]; f.has_r = v[6]; f.has_r2 = v[7]; f.has_mask = v[8]; f.has_drop = v[9]; f.has_act = v[10]; f.has_dx = v[11];
    f.has_dw = v[12]; f.beta = v[13]; f.x_ok = v[14]; f.w_ok = v[15]; f.g_ok = v[16]; f.bias_ok = v[17]; f.u_ok = v[18]; f.r_ok = v[19]; f.r2_ok = v[20];
    f.dx_ok = v[21]; f.rows_on = v[22]; f.stage256_on = v[23]; f.ws_bytes = v[24];
    if (dir == 'F') {
      const DenseFwdPlan p = adt_dense_fwd_plan(f);
      printf("%s %d %d %d %zu %d %d %d %d %d %d %d %d %d %d\n", FA[p.arm], p.grid_x, p.grid_y, p.block, p.lds_bytes, p.chunk, p.epi, p.pc, p.n_panels, p.row_groups, p.kb, p.ch,
             p.bn, p.nt_m, p.nt_n);
    } else {
      const DenseBwdPlan p = adt_dense_bwd_plan(f);
      printf("%s %d %d %d %zu %d %d %d %d %d %d ", DX[p.dx], p.dx_grid_x, p.dx_grid_y, p.dx_block, p.dx_lds_bytes, p.nb, p.dx_chunk, p.n_pieces, p.pc, p.n_panels, (int)p.has_u);
      for (int j = 0; j < p.n_pieces; ++j)
        printf("%s%d:%d:%d:%d:%d:%zu", j ? "," : "", p.piece[j].n0, p.piece[j].chunk, p.piece[j].beta, p.piece[j].kb, p.piece[j].row_groups, p.piece[j].lds_bytes);
      printf("%s %d %d %d %d %d %d | ", p.n_pieces ? "" : "-", p.dx_bn, p.gx, p.gy, p.dx_splits, p.n_chunk, (int)p.dx_zero_fill);
      printf("%s %d %d %d %zu %d %d %d %d %d %d %lld %d %d %d %d %d %d %d\n", DW[p.dw], p.dw_grid_x, p.dw_grid_y, p.dw_block, p.dw_lds_bytes, p.dw_chunk, p.nwg, p.blocks, p.kblocks,
             p.per, p.reduce_groups, (long long)p.ws_used, (int)p.partials, p.dw_splits, p.n_blocks, p.k_blocks, p.dw_bn, p.dw_gx, p.dw_gy);
    }
  }
  return 0;
}
"""


def test_the_restatements_are_the_header_over_the_whole_domain(world, tmp_path):
    """test_wide_plan_cpu.py holds expect_fwd, expect_dx and expect_dw against adt_wide_plan.h at chosen points; the enumeration relies on them at
    every point it visits, the case table at every case, and the child-process test at ADT_STAGE256=0.  All of those facts go through the header here."""
    points = [("F", f) for f in sorted(world[1]["fwd"])] + [("B", f) for f in sorted(world[1]["bwd"])]
    for c in dc.CASES:
        for on in (0, 1):
            points.append(("F", tuple(dc.facts(c, "fwd", on)[k] for k in FACT_FIELDS)))
            if c.want:
                points.append(("B", tuple(dc.facts(c, "bwd", on)[k] for k in FACT_FIELDS)))
    src, exe = tmp_path / "dense_domain.cpp", tmp_path / "dense_domain"
    src.write_text(PLAN_MAIN)
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(REPO, "adt_amd", "csrc"), "-o", str(exe), str(src)])
    text = "".join("%s %s\n" % (d, " ".join(str(int(v)) for v in f)) for d, f in points)
    got = subprocess.run([str(exe)], input=text, capture_output=True, text=True, timeout=120, check=True).stdout.splitlines()
    assert len(got) == len(points) > 10000

    def line(fields):
        return " ".join(str(int(v)) if isinstance(v, bool) else str(v) for v in fields)
    bad = []
    for (d, t), g in zip(points, got):
        f = dict(zip(FACT_FIELDS, t))
        want = line(expect_fwd(f)) if d == "F" else line(expect_dx(f)) + " | " + line(expect_dw(f))
        if g != want:
            bad.append((f, g, want))
    assert not bad, bad[:3]


def test_reachable_keys_are_the_instantiations_named_in_adt_wide(reach):
    """The launchers of adt_wide.hip, by hand.  Loop regimes: `stages` is "a workgroup runs more than one 32-row stage" (adt_t_chunk), which every
    stage kernel reaches at the T regimes of the domain."""
    want = set()
    # launch_dense_fwd256: k_dense_fwd256<0..7>, grid.y = N / 256 = 1..4, one stage or more
    want |= {("F256", epi, nblk, stages) for epi in range(8) for nblk in (1, 2, 3, 4) for stages in (False, True)}
    # launch_dense_fwd_rows: k_dense_fwd_rows<2 | 4 | 8, 4 | 8>; one narrow panel, one full panel, several panels.  At K = 256 the full single panel
    # (N = 256) belongs to k_dense_fwd256 while ADT_STAGE256 is on
    want |= {("FROWS", kb, ch, panels, narrow) for kb in (2, 4, 8) for ch in (4, 8) for panels, narrow in ((False, True), (False, False), (True, False))
             if not (kb == 8 and not panels and not narrow)}
    # launch_dense_fwd: k_dense_fwd<PREC, 64 | 128>
    want |= {("FTILED", prec, bn) for prec in (F32, BF16) for bn in (64, 128)}
    # launch_dense_dx256: k_dense_dx256<1 | 2 | 3>
    want |= {("DX256", nb, stages) for nb in (1, 2, 3) for stages in (False, True)}
    # launch_dense_dx_rows: k_dense_dx_rows<2 | 4, true> (chunks of 128 and 64 under an activation), <2 | 4 | 8, false>; one piece or several
    # (N = 448: all three widths; 256 and up: the widest only), the first piece with and without beta
    pieces = [({(2, True)}, False), ({(4, True)}, False), ({(4, True)}, True), ({(4, True), (2, True)}, True),
              ({(2, False)}, False), ({(4, False)}, False), ({(8, False)}, False), ({(8, False)}, True), ({(8, False), (4, False), (2, False)}, True)]
    want |= {("DXROWS", frozenset(s), several, beta) for s, several in pieces for beta in (False, True)}
    # launch_dense_dx_tiled: k_dense_bwd_dx<PREC, 64 | 128>; one split, or several with the zero fill (beta off) or without (beta on)
    want |= {("DXTILED", prec, bn, split, zero) for prec in (F32, BF16) for bn in (64, 128) for split, zero in ((False, False), (True, True), (True, False))}
    # launch_dense_dw256: k_dense_dw256 + k_dense_dw256_reduce over (blocks, blocks along K); per = 32 from 128 workgroups on, which only one block
    # reaches in the domain (T = 4136: one stage, 8232: three); the last reduce group is incomplete at every T of the domain
    want |= {("DW256", b, kb, 16, stages, True) for b, kb in ((1, 1), (2, 1), (3, 1), (4, 1), (2, 2), (4, 2), (4, 4)) for stages in (False, True)} - {("DW256", 1, 1, 16, True, True)}
    want |= {("DW256", 1, 1, 32, False, True), ("DW256", 1, 1, 32, True, True)}
    # launch_dense_dw_rows: k_dense_dw_rows; four blocks at least: several along N, along K, or both
    want |= {("DWROWS", True, False), ("DWROWS", False, True), ("DWROWS", True, True)}
    # launch_dense_dw64: k_dense_dw64 with partials + k_dense_dw64_reduce in one pass or two, or with atomics; six layouts of up to four 64 x 64 blocks
    want |= {("DW64", b, kb, part, two) for b, kb in ((1, 1), (2, 1), (2, 2), (4, 1), (4, 2), (4, 4)) for part in (False, True) for two in (False, True)}
    # launch_dense_dw_tiled: k_dense_bwd_dw<PREC, 64 | 128>
    want |= {("DWTILED", prec, bn) for prec in (F32, BF16) for bn in (64, 128)}
    assert set(reach) == want, (sorted(set(reach) - want, key=repr), sorted(want - set(reach), key=repr))


def test_table_hits_every_key_and_rotates_every_feature(reach):
    seen = hits(dc.CASES)
    assert gaps(reach, dc.CASES) == []
    assert len(dc.CASES) <= MAX_CASES and len(set(dc.CASES)) == len(dc.CASES)
    # a T that is no multiple of the arm's row tile, t_dev or not, under every key
    for c in dc.CASES:
        for which, k in thirds(c):
            assert c.T % ROW_TILE[k[0]] and dc.rows_live(c) % ROW_TILE[k[0]], (c, k)
    # keys outside the domain's reach are fallbacks of shapes outside its sets (N % 4 != 0, N = 320), never a new instantiation
    assert {inst(k) for k in seen} <= {inst(k) for k in reach}


def test_table_holds_the_regimes_of_the_issue():
    by = {}
    for c in dc.CASES:
        for which, k in thirds(c):
            by.setdefault(k, []).append(c)
    # two stages with a ragged second one: chunk 64, 40 rows in the last workgroup
    for N, T in ((256, 8232), (512, 8232), (768, 8232), (1024, 4136)):
        for epi in range(8):
            assert any(c.T == T for c in by[("F256", epi, N // 256, True)])
        chunk = expect_fwd(dc.facts(dc.case(BF16, T, 256, N, want=""), "fwd"))[5]
        assert chunk == 64 and T % chunk == 40
    assert any(c.act == dc.ACT_NONE and c.save_u for c in by[("F256", 4, 1, True)])
    for nb in (1, 2, 3):
        cs = by[("DX256", nb, True)]
        assert {(bool(c.beta), c.act != dc.ACT_NONE) for c in cs} == {(False, False), (False, True), (True, False), (True, True)}
    e = expect_dw(dc.facts(dc.case(BF16, 8232, 256, 256), "bwd"))
    assert e[:1] + e[6:7] + e[9:11] == ("DW256", 129, 32, 5) and by[("DW256", 1, 1, 32, True, True)]
    e = expect_dw(dc.facts(dc.case(BF16, 2088, 512, 512), "bwd"))
    assert e[:1] + e[5:6] + e[7:9] == ("DW256", 64, 4, 2) and any((c.K, c.N) == (512, 512) for c in by[("DW256", 4, 2, 16, True, True)])
    e = expect_dw(dc.facts(dc.case(BF16, 16500, 64, 64), "bwd"))
    assert e[:1] + e[6:7] == ("DW64", 129)
    assert any("b" in c.want and c.t_dev for k, cs in by.items() if k[0] == "DW64" and k[3] and k[4] for c in cs)
    e = expect_dx(dc.facts(dc.case(BF16, 40, 64, 4100), "bwd"))
    assert e[:1] + e[12:13] + e[15:16] + e[17:18] == ("DXTILED", 64, 26, 1)
    e = expect_dx(dc.facts(dc.case(BF16, 40, 256, 4100), "bwd"))
    assert e[:1] + e[12:14] == ("DXTILED", 128, 2)
    assert {(c.prec, c.K, c.beta) for c in dc.CASES if c.N == 4100} == set(itertools.product((F32, BF16), (64, 256), (0, 1)))
    assert {c.N for k, cs in by.items() if k[0] == "FROWS" for c in cs} >= {36, 100, 260, 448}
    assert any(k[0] == "DXROWS" and len(k[1]) == 3 for k in by)
    assert any(c.K % 128 for c in by[("DWROWS", True, False)]) and any(c.N % 256 for c in by[("DWROWS", True, True)])
    for prec in (F32, BF16):
        for bn in (64, 128):
            assert any(c.K % 32 and c.T % 128 for c in by[("FTILED", prec, bn)])
    # fallbacks: every layout tag once, each on a shape whose aligned twin takes a faster arm
    tags = {}
    for c in dc.CASES:
        if c.layout != "aligned":
            assert c.layout not in tags, c.layout
            tags[c.layout] = c
            twin = c._replace(layout="aligned")
            slow, fast = dict(thirds(c)), dict(thirds(twin))
            which = "dx" if c.layout.startswith("dX") else "fwd"
            assert slow[which][0] in ("FTILED", "DXTILED") and fast[which][0] not in ("FTILED", "DXTILED"), (c, slow, fast)
    assert set(tags) == set(dc.LAYOUTS) - {"aligned"}
    assert dict(thirds(tags["U+ld"]))["dx"][0] == "DXTILED" and tags["U+ld"].act != dc.ACT_NONE      # the scalar arm of GradSrc::at
    assert any(c.N % 4 and c.prec == BF16 and c.want for c in dc.CASES) and any(c.N % 4 and c.prec == F32 for c in dc.CASES)
    # no workspace: 256 x 256 -> tiled, 256 x 1024 -> k_dense_dw_rows, 64 x 64 -> atomics
    nows = {(c.N, c.K): dict(thirds(c))["dw"][0] for c in dc.CASES if c.ws == "none" and "w" in c.want}
    assert nows[(256, 256)] == "DWTILED" and nows[(256, 1024)] == "DWROWS" and nows[(64, 64)] == "DW64"
    for c in dc.CASES:
        if c.ws == "none" and "w" in c.want:
            assert dict(thirds(c._replace(ws="registered")))["dw"] != dict(thirds(c))["dw"], c      # the shape would have used the workspace


def test_gaps_sees_a_missing_key_feature_or_saved_u(reach):
    """The reduction on doctored inputs: a key no case produces, and for every key the table hits, the table without the cases that hit it."""
    fake = ("F256", 8, 1, False)
    assert (fake, "no case") in gaps({**reach, fake: {"drop": {True}}}, dc.CASES)
    seen = hits(dc.CASES)
    for k in sorted(set(seen) & set(reach), key=repr):
        rest = [c for c in dc.CASES if k not in [kk for _, kk in thirds(c)]]
        assert (k, "no case") in gaps(reach, rest), k
    # one case removed: whatever only it delivers is reported
    lone = [c for c in dc.CASES if gaps(reach, [x for x in dc.CASES if x != c])]
    assert len(lone) > len(dc.CASES) // 3
    # a feature value removed from an instantiation
    i = ("F256", 5)
    assert (i, "t_dev", True) in gaps(reach, [c for c in dc.CASES if not (c.t_dev and inst(dict(thirds(c))["fwd"]) == i)])
    i = ("DX256", 2)
    assert (i, "beta", True) in gaps(reach, [c for c in dc.CASES if not (c.beta and "x" in c.want and inst(dict(thirds(c)).get("dx", ("",))) == i)])
    assert ("FTILED", "act", "save_u") in gaps(reach, [c for c in dc.CASES if not (dc.key(c, "fwd")[0] == "FTILED" and c.save_u and c.act == dc.ACT_NONE)])


SMALL = [dc.case(F32, 37, 64, 36, act=dc.ACT_GELU, p=dc.P_DROP, R=1, R2=1, mask=1), dc.case(F32, 50, 100, 64, act=dc.ACT_ELU1, p=0.0, R=1),
         dc.case(F32, 33, 64, 64, act=dc.ACT_RELU, p=dc.P_DROP, mask=1), dc.case(F32, 41, 128, 102, bias=0, p=dc.P_DROP)]


@pytest.mark.parametrize("c", SMALL, ids=dc.case_id)
def test_float64_reference_against_the_tape_oracle(c):
    """ref64 is the oracle of test_wide_kernels.test_dense_forward_backward in float64 with the second residual and the row mask: the two agree to
    float32 rounding (3e-5 of the tensor maximum, what that test allows the exact-fp32 kernels)."""
    inp = dc.make_inputs(c)
    y, dx, dw, db = dc.tape_oracle(c, inp)
    ref = dc.ref64(c)
    for name, got in (("Y", y), ("dX", dx), ("dW", dw), ("db", db)):
        assert np.abs(got - ref[name]).max() <= 3e-5 * np.abs(ref[name]).max(), name
    assert ref["exact"].any() == bool(c.p or c.mask)
    assert np.all(np.abs(ref["Y"][ref["exact"]] - ref["exact_value"][ref["exact"]]) <= 2.0 ** -23 * np.abs(ref["exact_value"][ref["exact"]]))


def test_reference_bounds_are_positive_and_t_dev_cuts_the_weight_gradient():
    c = dc.case(BF16, 100, 64, 64, act=dc.ACT_GELU, p=dc.P_DROP, mask=1, t_dev=1, beta=1, R=1)
    ref, full = dc.ref64(c), dc.ref64(c._replace(t_dev=0))
    live = dc.rows_live(c)
    assert live == 100 - 33
    for name in ("e_y", "e_v", "e_dx", "e_dw", "e_db", "e_plain", "e_dx_plain", "e_dw_plain"):
        assert np.all(ref[name] > 0), name
    assert np.all(ref["e_plain"] >= ref["e_y"]) and np.abs(ref["dW"] - full["dW"]).max() > 0.1
    inp = dc.make_inputs(c)
    G = dc.grad_source(c, inp, ref["U"].astype(np.float32), True)
    assert not G[live:].any() and not G[:live][inp["ids"][:live] == 0].any() and np.array_equal(dc.bf16_round(G.astype(np.float32)), G.astype(np.float32))
    assert np.allclose(ref["dW"], G[:live].T @ dc.bf16_round(inp["X"][:live]).astype(np.float64))


def test_bf16_round_is_the_conversion_torch_makes():
    torch = pytest.importorskip("torch")
    r = np.random.RandomState(0)
    x = np.concatenate([r.standard_normal(4000).astype(np.float32) * np.float32(10.0) ** r.randint(-6, 6, 4000).astype(np.float32),
                        r.randint(0, 2 ** 31 - 2 ** 24, 2000).astype(np.uint32).view(np.float32),
                        # ties (the 16 dropped bits are 0x8000) above an even and an odd kept bit, their neighbours, the last step before a power of two
                        np.array([0x3F808000, 0x3F818000, 0x3F807FFF, 0x3F808001, 0x3F818001, 0x3F817FFF, 0x3FFFFFFF, 0x3FFF8000, 0x00000000, 0x80000000, 0xBF808000,
                                  0xBF818000, 0x7F7F7FFF, 0x00800000, 0x00008000, 0x00018000], np.uint32).view(np.float32)])
    want = torch.from_numpy(x).bfloat16().float().numpy()
    got = dc.bf16_round(x)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(dc.bf16_round(got), got) and not (got.view(np.uint32) & 0xFFFF).any()
