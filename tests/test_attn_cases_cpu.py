"""CPU: the case table of tests/attn_cases.py reaches every resident and chunked masked-attention instantiation that adt_attn_masked_plan can
choose over the supported domain, under every mask mode that can reach it and with dropout off and on.  The plan is read through its Python
restatement expect_attn (test_wide_plan_cpu.py, which checks the restatement against the header); the streamed instantiations belong to
test_attn_hd256_hip.py.  Also: the float64 reference of the GPU tests against the float32 tape oracle the other attention tests use."""
import math
import os
import subprocess

import numpy as np
import pytest

import attn_cases as ac
from test_wide_plan_cpu import expect_attn

MAX_CASES = 120


def modes_of(hd):
    return ac.MODES_128 if hd == 128 else ac.MODES


def reachable():
    """{instantiation key: the (mask, fill) modes that reach it} over prec x (hd 16/32/64, L 1..224 | hd 128, L 1..256) x direction x mode."""
    reach = {}
    for prec in (ac.F32, ac.BF16):
        for hd in (16, 32, 64, 128):
            for L in range(1, (256 if hd == 128 else 224) + 1):
                for bwd in (0, 1):
                    for mode in modes_of(hd):
                        reach.setdefault(ac.inst_key(expect_attn, prec, hd, L, bwd, *mode), set()).add(mode)
    return {k: v for k, v in reach.items() if k[3] != "STREAMED"}


def hits(cases):
    """{instantiation key: (modes seen, dropout settings seen)} of a case list (each case runs its forward and its backward)."""
    seen = {}
    for prec, H, hd, L, mask, fill, p, scale in cases:
        for bwd in (0, 1):
            modes, drops = seen.setdefault(ac.inst_key(expect_attn, prec, hd, L, bwd, mask, fill), (set(), set()))
            modes.add((mask, fill))
            drops.add(p > 0.0)
    return seen


def gaps(reach, cases):
    """What the case list leaves uncovered: (key, what is missing)."""
    seen, out = hits(cases), []
    for key, modes in sorted(reach.items()):
        if key not in seen:
            out.append((key, "no case"))
            continue
        out += [(key, "dropout %s" % ("on" if on else "off")) for on in (False, True) if on not in seen[key][1]]
        out += [(key, mode) for mode in sorted(modes - seen[key][0])]
    return out


@pytest.fixture(scope="module")
def reach():
    return reachable()


DOMAIN_MAIN = r"""
#include <math.h>
#include <stdio.h>
#include "adt_wide_plan.h"
using namespace adt;
int main() {
  static const char* const AF[] = {"RESIDENT", "CHUNKED", "STREAMED"};
  static const int HD[] = {16, 32, 64, 128};
  static const struct { int causal, kid; float fill; } MODE[] = {{1, 0, -INFINITY}, {0, 1, -1e9f}, {1, 1, -1e9f}, {1, 0, -1e9f}, {1, 0, -1e4f}};
  for (int prec = 0; prec < 2; ++prec)
    for (int hd : HD)
      for (int L = 1; L <= (hd == 128 ? 256 : 224); ++L)
        for (int bwd = 0; bwd < 2; ++bwd)
          for (int m = 0; m < (hd == 128 ? 5 : 3); ++m) {
            const AttnPlan p = adt_attn_masked_plan(prec, hd, L, bwd != 0, MODE[m].causal != 0, MODE[m].kid != 0, MODE[m].fill);
            if (p.error[0]) printf("error %s\n", p.error);
            else printf("%d %d %d %d %d %s %d %d %d\n", prec, hd, L, bwd, m, AF[p.family], p.maxkt, p.nch, (int)p.csk);
          }
  return 0;
}
"""


def test_the_restatement_is_the_header_over_the_whole_domain(tmp_path):
    """test_wide_plan_cpu.py holds expect_attn against adt_wide_plan.h at chosen points; the enumeration above relies on it at every L."""
    src, exe = tmp_path / "attn_domain.cpp", tmp_path / "attn_domain"
    src.write_text(DOMAIN_MAIN)
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(repo, "adt_amd", "csrc"), "-o", str(exe), str(src)])
    got = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60, check=True).stdout.splitlines()
    want = []
    for prec in (ac.F32, ac.BF16):
        for hd in (16, 32, 64, 128):
            for L in range(1, (256 if hd == 128 else 224) + 1):
                for bwd in (0, 1):
                    for m, mode in enumerate(modes_of(hd)):
                        key = ac.inst_key(expect_attn, prec, hd, L, bwd, *mode)
                        want.append("%d %d %d %d %d %s %d %d %d" % ((prec, hd, L, bwd, m) + key[3:]))
    assert got == want, [(a, b) for a, b in zip(got, want) if a != b][:5]


def test_reachable_keys_are_the_instantiations_named_in_adt_wide(reach):
    """launch_attn_gen_l: <hd, 4 | 8 | 14> resident, fp32 hd 64 backward at L > 128 chunked <16, 2>; launch_attn_gen_128: <4, 1> and <16, 2>, the
    forward with and without CSK, the backward chunked; fp32 at hd 128 and L > 64 streams and is dropped."""
    want = set()
    for prec in (ac.F32, ac.BF16):
        for hd in (16, 32, 64):
            for maxkt in (4, 8, 14):
                want.add(("fwd", prec, hd, "RESIDENT", maxkt, 1, 0))
                want.add(("bwd", prec, hd, "CHUNKED", 16, 2, 0) if (prec, hd, maxkt) == (ac.F32, 64, 14) else ("bwd", prec, hd, "RESIDENT", maxkt, 1, 0))
        for maxkt, nch in ((4, 1), (16, 2)) if prec == ac.BF16 else ((4, 1),):
            want |= {("fwd", prec, 128, "RESIDENT", maxkt, nch, 0), ("fwd", prec, 128, "RESIDENT", maxkt, nch, 1), ("bwd", prec, 128, "CHUNKED", maxkt, nch, 0)}
    assert set(reach) == want
    for key, modes in reach.items():
        if key[0] == "fwd" and key[2] == 128:      # CSK: causal, no key ids, fill <= -1e9
            assert modes == ({("causal", ac.NINF), ("causal", -1e9)} if key[6] else {("keypad", -1e9), ("both", -1e9), ("causal", -1e4)}), key
        else:
            assert modes == set(modes_of(key[2])), key


def test_table_reaches_every_instantiation_under_every_mode(reach):
    assert set(hits(ac.CASES)) <= set(reach), "a case outside the resident / chunked families: %s" % sorted(set(hits(ac.CASES)) - set(reach))
    assert gaps(reach, ac.CASES) == []
    assert len(ac.CASES) <= MAX_CASES and len(set(ac.CASES)) == len(ac.CASES)


def test_table_holds_the_required_shapes_and_modes():
    plain = {(c[0], c[2], c[3]) for c in ac.CASES if c[7] is None}
    for prec in (ac.F32, ac.BF16):
        assert {(prec, hd, L) for hd in (16, 32, 64) for L in (1, 16, 37, 64, 65, 128, 129, 200, 224)} <= plain
        assert {(prec, 128, L) for L in (1, 50, 64)} <= plain
    assert {(ac.BF16, 128, L) for L in (65, 130, 200, 256)} <= plain
    assert not any(c[0] == ac.F32 and c[2] == 128 and c[3] > 64 for c in ac.CASES)      # streamed: test_attn_hd256_hip.py
    scaled = {(c[0], c[2], c[3], ac.true_hd(c[2], c[7])) for c in ac.CASES if c[7] is not None}
    assert {(p, hd, t) for p, hd, L, t in scaled} >= {(ac.F32, 32, 25), (ac.BF16, 32, 25), (ac.F32, 64, 50), (ac.BF16, 64, 50)} and (ac.BF16, 128, 200, 100) in scaled
    for prec, H, hd, L, mask, fill, p, scale in ac.CASES:
        assert (mask, fill) in modes_of(hd) and p in (0.0, 0.2) and H * hd % 8 == 0
        assert fill != ac.NINF or mask == "causal"      # a fully padded sequence under -inf: the reference is NaN, the kernel deliberately is not
    qkv, dO, ids, valid = ac.make_inputs((ac.BF16, 2, 128, 200, "keypad", -1e9, 0.0, 1 / math.sqrt(100)))
    assert not valid[2].any() and not valid[0, :66].any() and valid[0, 66:].all() and valid[1].all() and ac.B <= 3
    assert not qkv.reshape(-1, 6, 128)[:, :, 100:].any() and not dO.reshape(-1, 2, 128)[:, :, 100:].any() and qkv.reshape(-1, 6, 128)[:, :, 99].all()


def test_leak_and_sharp_cases_cover_their_instantiations(reach):
    """(c): one case per backward instantiation; its causal run (fill -inf) and its key-padding runs reach the matching forwards, CSK on and off.
    (d): the hd 128 instantiations only bf16 reaches."""
    bwd = {ac.inst_key(expect_attn, prec, hd, L, 1, "both", -1e9) for prec, H, hd, L in ac.LEAK_CASES}
    assert bwd == {k for k in reach if k[0] == "bwd"} and len(ac.LEAK_CASES) == len(bwd)
    fwd = {ac.inst_key(expect_attn, prec, hd, L, 0, *mode) for prec, H, hd, L in ac.LEAK_CASES for mode in ac.MODES}
    assert fwd == {k for k in reach if k[0] == "fwd"}
    for prec, H, hd, L in ac.LEAK_CASES:      # an odd number of tiles, at least four rows in the last one, L % 4 != 0
        assert ((L + 15) // 16) % 2 == 1 and L % 16 >= 4 and L % 4 and L > 32
    f32_keys = {k[2:] for k in reach if k[1] == ac.F32}
    only_bf16 = {k for k in reach if k[1] == ac.BF16 and k[2:] not in f32_keys and k[2] == 128}
    assert only_bf16 == {("fwd", ac.BF16, 128, "RESIDENT", 16, 2, 0), ("fwd", ac.BF16, 128, "RESIDENT", 16, 2, 1), ("bwd", ac.BF16, 128, "CHUNKED", 16, 2, 0)}
    sharp = {ac.inst_key(expect_attn, ac.BF16, 128, L, b, mask, fill) for L, mask, fill, p in ac.SHARP_CASES for b in (0, 1)}
    assert sharp == only_bf16 and {p > 0 for L, mask, fill, p in ac.SHARP_CASES} == {False, True}


def test_gaps_sees_a_missing_instantiation_mode_or_dropout(reach):
    """The reduction above on doctored inputs: it must report a key no case produces, a mode no case of a key has, and a dropout setting."""
    fake = ("fwd", ac.BF16, 128, "RESIDENT", 12, 1, 0)
    assert gaps({**reach, fake: {("causal", ac.NINF)}}, ac.CASES) == [(fake, "no case")]
    for key, modes in reach.items():
        hit = [c for c in ac.CASES if key in (ac.inst_key(expect_attn, c[0], c[2], c[3], b, c[4], c[5]) for b in (0, 1))]
        assert (key, "no case") in gaps(reach, [c for c in ac.CASES if c not in hit]), key
        for mode in modes:
            assert (key, mode) in gaps(reach, [c for c in ac.CASES if c not in hit or (c[4], c[5]) != mode]), (key, mode)
        for on in (False, True):
            assert (key, "dropout %s" % ("on" if on else "off")) in gaps(reach, [c for c in ac.CASES if c not in hit or (c[6] > 0) != on]), (key, on)


@pytest.mark.parametrize("case", [(ac.F32, 2, 16, 37, "both", -1e9, 0.2, None), (ac.F32, 2, 32, 20, "causal", ac.NINF, 0.2, 1 / math.sqrt(25)),
                                  (ac.F32, 2, 16, 33, "keypad", -1e9, 0.0, None)], ids=ac.case_id)
def test_float64_reference_against_the_tape_oracle(case):
    """ref64 is attn_oracle of test_wide_kernels.py / test_attn_hd256_hip.py restated in float64: the two agree to float32 rounding (1e-5 of the
    tensor maximum; the tape holds float32 values), the zero lanes of a scaled case included."""
    prec, H, hd, L, mask, fill, p, scale = case
    qkv, dO, ids, valid = ac.make_inputs(case)
    d, t = H * hd, ac.true_hd(hd, scale)
    want = ac.reference(case)
    q, k, v = (ac.true_lanes(qkv[:, i * d:(i + 1) * d], H, hd, t) for i in range(3))
    got = ac.tape_oracle(q, k, v, ac.true_lanes(dO, H, hd, t), ac.B, H, L, valid, ac.flags(mask)[0], fill, p, ac.SEED, ac.SITE, ac.B_OFF,
                         None if scale is None else scale)
    for name, g in zip(("o", "dq", "dk", "dv"), got):
        assert np.abs(g - want[name]).max() <= 1e-5 * np.abs(want[name]).max(), name
    dead = ac.attn_mask(ac.B, H, L, valid, ac.flags(mask)[0]).all(-1)
    assert np.all(want["lse"][dead] == math.log(L)) and dead.any() == (mask != "causal")
    if p == 0.0:
        assert np.abs(want["w"].sum(-1) - 1.0).max() < 1e-12
