"""CPU: where a flagship step hands the pad prefix of every sequence to its per-sequence chain kernels (StepPlan::pad_elide of
adt_amd/csrc/adt_step_plan.h; ADT_PAD_ELIDE): only where the embedding layer that writes the prefixes and every kernel that reads them is a
per-sequence kernel on the lean path with partials, and not with 16-wide heads, whose instantiations are left as they are.  A stand-alone host
program (plain g++, no HIP) prints the field per case; built and run a second time with -fsanitize=address,undefined."""
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (name, prec, assignments) -> pad_elide ; the flagship facts: L 200, d 64, H 2, two layers, B 256, 3417 item rows
CASES = [
    ("default", "ADT_PREC_BF16", "", 1),
    ("ADT_PAD_ELIDE=0", "ADT_PREC_BF16", "s.pad_elide = false;", 0),
    # the paths that are not the lean per-sequence one with partials
    ("f32", "ADT_PREC_F32", "", 0),
    ("ADT_SEQ=0", "ADT_PREC_BF16", "s.seq = false;", 0),
    ("ADT_SEQ_LEAN=0", "ADT_PREC_BF16", "s.seq_lean = false;", 0),
    ("ADT_SEQ_TT=0", "ADT_PREC_BF16", "s.seq_tt = false;", 0),
    ("ADT_SEQ_BWD=0", "ADT_PREC_BF16", "s.seq_bwd = false;", 0),
    ("ADT_SEQ_ATTN_BWD=0", "ADT_PREC_BF16", "s.seq_attn_bwd = false;", 0),
    ("ADT_SEQ_POST_BWD=0", "ADT_PREC_BF16", "s.seq_post_bwd = false;", 0),
    ("ADT_SEQ_PARTIALS=0", "ADT_PREC_BF16", "s.seq_partials = false;", 0),
    ("ADT_SEQ_ABLATE=0", "ADT_PREC_BF16", "s.seq_ablate_set = true;", 0),
    ("L=202", "ADT_PREC_BF16", "f.L = 202;", 0),
    # 16-wide heads
    ("H=4", "ADT_PREC_BF16", "f.H = 4; f.L = 128; f.sab_lds = sab_lds(128, 4);", 0),
    # switches and shapes that leave the path alone
    ("ADT_DO_BF16=0", "ADT_PREC_BF16", "s.do_bf16 = false;", 1),
    ("ADT_XATTN_FUSED=0", "ADT_PREC_BF16", "s.xattn_fused = false;", 1),
    ("ADT_SEQ_SPLIT=2", "ADT_PREC_BF16", "s.seq_split = 2;", 1),
    ("ADT_ITEM_SORT=1", "ADT_PREC_BF16", "s.item_sort = true;", 1),
    ("B=16", "ADT_PREC_BF16", "f.B = 16;", 1),
    ("H=1", "ADT_PREC_BF16", "f.H = 1; f.sab_lds = sab_lds(200, 1);", 1),
    ("three layers", "ADT_PREC_BF16", "f.num_layers = 3;", 1),
]

MAIN = r"""
#include <stdio.h>
#include "adt_step_plan.h"
static size_t sab_lds(int L, int H) { const size_t R = (size_t)((L + 31) / 32 * 32); return 4 * R * 72 * 2 + (size_t)H * R * 8 * 4 + 2 * (size_t)H * R * 4; }
int main() {
  { const SeqSwitches s; printf("switch-default %%d\n", (int)s.pad_elide); }
%s
  return 0;
}
"""
CASE = r"""  {
    SeqSwitches s;
    StepFacts f{%s, 200, 64, 2, 2, 256, 3417, true, sab_lds(200, 2)};
    %s
    const StepPlan p = adt_step_plan(f, s);
    printf("%d %%d %%d %%d %%s\n", (int)p.pad_elide, (int)p.parts, (int)p.lean, p.cfg_error);
  }
"""


@pytest.fixture(scope="module", params=[[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g", "-O1"]], ids=["plain", "asan-ubsan"])
def lines(request, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("pad_elision_plan")
    src, exe = tmp / "pad_elision_plan_main.cpp", tmp / "pad_elision_plan_main"
    src.write_text(MAIN % "".join(CASE % (prec, assign, i) for i, (_, prec, assign, _) in enumerate(CASES)))
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(REPO, "adt_amd", "csrc")] +
                          request.param + ["-o", str(exe), str(src)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120,
                         env=dict(os.environ, ASAN_OPTIONS="abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1"))
    assert out.returncode == 0 and "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-3000:]
    return out.stdout.splitlines()


def test_switch_is_on_by_default(lines):
    assert lines[0] == "switch-default 1"


def test_plan_field(lines):
    got = [line.split(" ", 4) for line in lines[1:]]
    assert len(got) == len(CASES)
    for (name, _, _, want), (i, on, parts, lean, err) in zip(CASES, got):
        assert err == "", (name, err)
        assert int(on) == want, (name, on)
        assert int(on) <= int(parts) <= int(lean), name      # never off the lean per-sequence path with partials
    by = {name: (int(g[1]), int(g[2])) for (name, _, _, _), g in zip(CASES, got)}
    assert by["default"] == (1, 1)
    assert by["ADT_PAD_ELIDE=0"] == (0, 1)      # the switch alone: the path stays
    assert by["H=4"] == (0, 1)                  # 16-wide heads: the path stays, the prefixes are not handed out
