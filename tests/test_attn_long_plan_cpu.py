"""CPU: adt_attn_long_plan and adt_attn_masked_max_len of adt_amd/csrc/adt_wide_plan.h (what adt_attn_long_fwd / _bwd launch with, and the
bound the model layer chooses by).  A stand-alone host program (plain g++, no HIP) prints one line per case; the expected lines are restated
here from the rules of the header's comment.  Built and run a second time with -fsanitize=address,undefined, as test_wide_plan_cpu.py does."""
import math
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, BF16 = 0, 1
LDS_MAX = 160 * 1024
HEADS = (16, 32, 64, 128, 256, 48)
LENGTHS = (0, 1, 224, 225, 256, 257, 1009, 1024, 1025)
# (causal, key ids, fill): the three that decide the causal skip, and the two it stays off for whatever the fill
MASKS = ((1, 0, -1e9), (1, 0, -math.inf), (1, 1, -1e9), (0, 0, -1e9), (1, 0, -1e4))
CASES = [(prec, hd, L, bwd) + m for prec in (F32, BF16) for hd in HEADS for L in LENGTHS for bwd in (0, 1) for m in MASKS]

MAIN = r"""
#include <math.h>
#include <stdio.h>
#include "adt_wide_plan.h"
using namespace adt;
static const double CASES[][7] = {%(cases)s};
static const int HEADS[] = {%(heads)s};
int main() {
  static const char* const AF[] = {"RESIDENT", "CHUNKED", "STREAMED"};
  for (int i = 0; i < %(ncases)d; ++i) {
    const double* c = CASES[i];
    const AttnPlan p = adt_attn_long_plan((int)c[0], (int)c[1], (int)c[2], c[3] != 0, c[4] != 0, c[5] != 0, (float)c[6]);
    if (p.error[0]) printf("A %%d error %%s\n", i, p.error);
    else printf("A %%d %%s %%d %%d %%d %%d %%d %%zu\n", i, AF[p.family], p.nch, p.kc, p.waves, (int)p.csk, p.grid_y, p.lds_bytes);
  }
  for (int i = 0; i < %(nheads)d; ++i) printf("M %%d %%d\n", HEADS[i], adt::adt_attn_masked_max_len(HEADS[i]));      // qualified: the C ABI declares the same name
  return 0;
}
"""


def c_double(v):
    return "-INFINITY" if v == -math.inf else repr(float(v))


def expect(prec, hd, L, bwd, causal, kid, fill):
    """The header's rules: head size, then length, then the footprint; always streamed, four waves of one 16-row tile, chunks of 64 keys in
    the bf16 forward and 32 rows elsewhere; images typed by the precision, LSE and delta of 1024 rows in the backward, 1024 validity bytes + 32."""
    if hd not in (16, 32, 64, 128, 256):
        return "error long attention: head_dim=%d unsupported (16/32/64/128/256)" % hd
    if L < 1 or L > 1024:
        return "error long attention: L=%d outside 1..1024" % L
    kc = 64 if prec == BF16 and not bwd else 32
    esz = 4 if prec == F32 else 2
    img = kc * (hd + 8) + hd * (kc + 8)
    lds = 2 * img * esz + 2 * 1024 * 4 + 1024 + 32 if bwd else img * esz + 1024 + 32
    assert lds <= LDS_MAX
    csk = int(bool(causal) and not kid and fill <= -1e9)
    return "STREAMED 1 %d 4 %d %d %d" % (kc, csk, -(-(-(-L // 16)) // 4), lds)


@pytest.fixture(scope="module", params=[[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g", "-O1"]], ids=["plain", "asan-ubsan"])
def table(request, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("attn_long_plan")
    src, exe = tmp / "attn_long_plan_main.cpp", tmp / "attn_long_plan_main"
    src.write_text(MAIN % dict(cases=", ".join("{" + ", ".join(c_double(v) for v in c) + "}" for c in CASES), ncases=len(CASES),
                               heads=", ".join(str(h) for h in HEADS), nheads=len(HEADS)))
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
        assert line == "A %d %s" % (i, expect(*case)), case


def test_errors_exactly_at_head_size_48_and_lengths_0_and_1025(table):
    for case, line in zip(CASES, table["A"]):
        assert (" error " in line) == (case[1] == 48 or case[2] in (0, 1025)), (case, line)


def test_every_footprint_fits_the_lds_and_the_tightest_is_fp32_hd256_backward(table):
    sizes = {case[:4]: int(line.split()[-1]) for case, line in zip(CASES, table["A"]) if " error " not in line}
    assert sizes and max(sizes.values()) <= LDS_MAX
    assert max(sizes.values()) == sizes[(F32, 256, 1024, 1)] == (2 * 32 * 264 + 2 * 256 * 40) * 4 + 8192 + 1024 + 32


def test_grid_covers_the_tiles_four_per_workgroup(table):
    got = {case[2]: int(line.split()[-2]) for case, line in zip(CASES, table["A"]) if " error " not in line}
    assert got == {1: 1, 224: 4, 225: 4, 256: 4, 257: 5, 1009: 16, 1024: 16}


def test_causal_skip_needs_a_causal_mask_no_key_ids_and_a_fill_of_at_most_minus_1e9(table):
    got = {case[4:]: int(line.split()[-3]) for case, line in zip(CASES, table["A"]) if " error " not in line}
    assert got == {(1, 0, -1e9): 1, (1, 0, -math.inf): 1, (1, 1, -1e9): 0, (0, 0, -1e9): 0, (1, 0, -1e4): 0}


def test_masked_max_len(table):
    assert table["M"] == ["M %d %d" % (hd, n) for hd, n in zip(HEADS, (224, 224, 224, 256, 256, 0))]
