"""CPU: the `phase` word of adt_sasrec_backward* (include/adt_hip.h: ADT_PHASE_*) as adt_amd/csrc/adt_bwd_plan.h decodes it, over all 128 words
x deferred-BCE forward {no, yes}.  A stand-alone host program (plain g++, no HIP) prints one line per combination; the expected table is restated
here from the header's rules.  Built and run a second time with -fsanitize=address,undefined."""
import os
import subprocess

import pytest

from adt_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MAIN = r"""
#include <stdio.h>
#include "adt_bwd_plan.h"
int main() {
  for (int deferred = 0; deferred < 2; ++deferred)
    for (int word = 0; word < 128; ++word) {
      BwdPlan p = {-1, false, false, false, false, false};
      const char* err = adt_bwd_plan(word, deferred != 0, &p);
      if (err) printf("%d %d reject %s\n", word, deferred, err);
      else printf("%d %d accept %d %d %d %d %d %d\n", word, deferred, p.phase, (int)p.prep_zeroed, (int)p.defer_fold, (int)p.bce_here, (int)p.bce_fwd,
                  (int)p.seeds_virtual);
    }
  return 0;
}
"""


def expected(word, deferred):
    """None (rejected) or (phase, prep_zeroed, defer_fold, bce_here, bce_fwd, seeds_virtual)."""
    phase = word & _lib.PHASE_MASK
    zeroed, fold = bool(word & _lib.PHASE_PREZEROED), bool(word & _lib.PHASE_DEFER_FOLD)
    here, fwd, virt = bool(word & _lib.PHASE_BCE_HERE), bool(word & _lib.PHASE_BCE_FWD), bool(word & _lib.PHASE_SEEDS_VIRTUAL)
    if phase == 3:
        return None
    if (here or fwd) and not deferred:      # bits 4 / 5 need the deferred-BCE forward
        return None
    if fwd and (here or not zeroed or phase == 2):      # bit 5 needs bit 2, excludes bit 4 and phase 2
        return None
    return (phase, int(zeroed), int(fold and phase == 0), int(here), int(fwd), int(here or fwd or virt))


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g", "-O1"]], ids=["plain", "asan-ubsan"])
def test_backward_plan_table(tmp_path, flags):
    assert (_lib.PHASE_MASK, _lib.PHASE_PREZEROED, _lib.PHASE_DEFER_FOLD, _lib.PHASE_BCE_HERE, _lib.PHASE_BCE_FWD, _lib.PHASE_SEEDS_VIRTUAL) == (3, 4, 8, 16, 32, 64)
    src, exe = tmp_path / "plan_main.cpp", tmp_path / "plan_main"
    src.write_text(MAIN)
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(REPO, "adt_amd", "csrc")] + flags +
                          ["-o", str(exe), str(src)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60,
                         env=dict(os.environ, ASAN_OPTIONS="abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1"))
    assert out.returncode == 0 and "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-3000:]
    lines = out.stdout.splitlines()
    assert len(lines) == 256
    seen, accepted = set(), 0
    for line in lines:
        f = line.split(None, 3)
        word, deferred = int(f[0]), int(f[1])
        seen.add((word, deferred))
        want = expected(word, bool(deferred))
        if want is None:
            assert f[2] == "reject" and f[3].startswith("backward: "), line
        else:
            accepted += 1
            assert f[2] == "accept" and tuple(int(v) for v in f[3].split()) == want, (line, want)
    assert len(seen) == 256
    # phases 0-2 x bits 2, 3, 6 free: 24 words without bits 4 / 5 ; with the deferred forward also bit 4 alone (24) and bit 5 (+ bit 2, phase 0 / 1: 8)
    assert accepted == 24 + (24 + 24 + 8)
    # the messages of the two rules that were there before the plan header
    assert "16 0 reject backward: phase bit 4 / 5 without the deferred-BCE forward (adt_sasrec_bce_deferred)" in lines
    assert "32 1 reject backward: phase bit 5 goes with bit 2, without bit 4, in phase 0 or 1" in lines
