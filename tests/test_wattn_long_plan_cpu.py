"""CPU: adt_wattn_long_plan and adt_wattn_max_len of adt_amd/csrc/adt_wide_plan.h (what adt_wattn_long_* / adt_klattn_long_* launch with, and the
bound DisenDistSAModel chooses by).  A stand-alone host program (plain g++, no HIP) prints one line per case; the expected lines are restated
here from the rules of the header's comment.  Built and run a second time with -fsanitize=address,undefined, as test_attn_long_plan_cpu.py does."""
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, BF16 = 0, 1
LDS_MAX = 160 * 1024
HEADS = (16, 32, 64, 48, 128)
LENGTHS = (0, 1, 141, 142, 256, 257, 1009, 1024, 1025)
CASES = [(prec, hd, L, bwd) for prec in (F32, BF16) for hd in HEADS for L in LENGTHS for bwd in (0, 1)]

MAIN = r"""
#include <stdio.h>
#include "adt_wide_plan.h"
using namespace adt;
static const int CASES[][4] = {%(cases)s};
static const int HEADS[] = {%(heads)s};
int main() {
  for (int i = 0; i < %(ncases)d; ++i) {
    const int* c = CASES[i];
    const AttnPlan p = adt_wattn_long_plan(c[0], c[1], c[2], c[3] != 0);
    if (p.error[0]) printf("A %%d error %%s\n", i, p.error);
    else printf("A %%d %%d %%d %%d %%d %%d %%zu\n", i, (int)p.family, p.kc, p.waves, (int)p.csk, p.grid_y, p.lds_bytes);
  }
  for (int i = 0; i < %(nheads)d; ++i) printf("M %%d %%d\n", HEADS[i], adt::adt_wattn_max_len(HEADS[i]));      // qualified: the C ABI declares the same name
  for (int i = 0; i < %(nheads)d; ++i)
    for (int L = 1; L <= 256; L += 5)
      printf("V %%d %%d %%zu %%zu\n", HEADS[i], L, wattn_valu_lds(L, HEADS[i], false), wattn_valu_lds(L, HEADS[i], true));
  return 0;
}
"""


def expect(prec, hd, L, bwd):
    """The header's rules: head size, then length, then the footprint; always streamed (family 2), four waves of one 16-row tile, chunks of
    64 keys in the forward and 32 rows in the backward; fp32 images whatever the precision; the causal skip always on."""
    if hd not in (16, 32, 64):
        return "error long distance attention: head_dim=%d unsupported (16/32/64)" % hd
    if L < 1 or L > 1024:
        return "error long distance attention: L=%d outside 1..1024" % L
    kc = 32 if bwd else 64
    cat, t, nat = kc * (2 * hd + 4) + kc, hd * (kc + 4), kc * (hd + 4)
    floats = cat + 2 * t + 2 * nat + 2 * t + 2 * 1024 if bwd else cat + 2 * t
    lds = 4 * floats + 1024 + 32
    assert lds <= LDS_MAX
    return "2 %d 4 1 %d %d" % (kc, -(-(-(-L // 16)) // 4), lds)


def wattn_lds_bytes(L, hd, bwd):
    """adt_stosa.cuh: 4 resident tensors [L][hd + 1], 2 row vectors [L'] (+ 2 in the backward), per-wave scratch 4 x (3 L' + 4 hd); L' = L up to 64."""
    lp = -(-L // 64) * 64
    return 4 * (4 * L * (hd + 1) + (4 if bwd else 2) * lp + 4 * (3 * lp + 4 * hd))


def wattn_max_len(hd):
    if hd not in (16, 32, 64):
        return 0
    return max(L for L in range(1, 257) if wattn_lds_bytes(L, hd, False) <= LDS_MAX and wattn_lds_bytes(L, hd, True) <= LDS_MAX)


@pytest.fixture(scope="module", params=[[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g", "-O1"]], ids=["plain", "asan-ubsan"])
def table(request, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("wattn_long_plan")
    src, exe = tmp / "wattn_long_plan_main.cpp", tmp / "wattn_long_plan_main"
    src.write_text(MAIN % dict(cases=", ".join("{%d, %d, %d, %d}" % c for c in CASES), ncases=len(CASES),
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


def test_errors_exactly_at_head_sizes_48_and_128_and_lengths_0_and_1025(table):
    for case, line in zip(CASES, table["A"]):
        assert (" error " in line) == (case[1] in (48, 128) or case[2] in (0, 1025)), (case, line)


def test_every_footprint_fits_the_lds_and_does_not_depend_on_the_precision(table):
    sizes = {case: int(line.split()[-1]) for case, line in zip(CASES, table["A"]) if " error " not in line}
    assert sizes and max(sizes.values()) <= LDS_MAX
    for (prec, hd, L, bwd), n in sizes.items():
        assert n == sizes[(1 - prec, hd, L, bwd)]
    # the tightest: head size 64 backward, cross width 128 plus the value / output-gradient images
    assert max(sizes.values()) == sizes[(F32, 64, 1024, 1)] == 4 * (32 * 132 + 32 + 128 * 36 + 2 * 32 * 68 + 2 * 64 * 36 + 2048) + 1056


def test_grid_covers_the_tiles_four_per_workgroup(table):
    got = {case[2]: int(line.split()[-2]) for case, line in zip(CASES, table["A"]) if " error " not in line}
    assert got == {1: 1, 141: 3, 142: 3, 256: 4, 257: 5, 1009: 16, 1024: 16}


def test_restated_footprint_of_the_vector_alu_kernels(table):
    for line in table["V"]:
        _, hd, L, fwd, bwd = line.split()
        assert (int(fwd), int(bwd)) == (wattn_lds_bytes(int(L), int(hd), False), wattn_lds_bytes(int(L), int(hd), True)), line


def test_wattn_max_len(table):
    assert table["M"] == ["M %d %d" % (hd, wattn_max_len(hd)) for hd in HEADS]
    # head size 64: the backward's four [L][65] tensors; 141 fits, 142 (L' = 192) does not
    assert wattn_max_len(64) == 141 and wattn_lds_bytes(141, 64, True) <= LDS_MAX < wattn_lds_bytes(142, 64, True)
    assert wattn_max_len(16) == wattn_max_len(32) == 256
