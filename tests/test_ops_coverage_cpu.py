"""Every public wrapper of adt_amd/ops.py that launches a C-ABI kernel is called by at least one GPU kernel test.  A text scan of the
project's own Python sources: it keeps a wrapper from being reachable only through whole-model tests, whose bounds are too loose to notice a
wrong kernel."""
import ast
import glob
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name -> why no kernel test calls it directly
EXEMPT = {
    "lce_supported": "a host-side predicate (which (prec, K) adt_lce_fwd_bwd covers): it launches nothing",
}


def kernel_wrappers():
    """Public functions of adt_amd/ops.py whose body calls _lib.load().adt_* (directly, through a local `lib = _lib.load()`, or by symbol name
    through one of the module's private helpers that does)."""
    src = open(os.path.join(REPO, "adt_amd", "ops.py")).read()
    funcs = {n.name: ast.get_source_segment(src, n) for n in ast.parse(src).body if isinstance(n, ast.FunctionDef)}
    direct = re.compile(r"_lib\.load\(\)\s*\.\s*adt_\w+\s*\(|\blib\.adt_\w+\s*\(|getattr\(lib, \"adt_\"")
    launching = {name for name, body in funcs.items() if direct.search(body)}
    grew = True
    while grew:                                  # wrappers that go through a private helper (_stosa_attn_fwd -> _stosa_attn_call)
        grew = False
        for name, body in funcs.items():
            if name not in launching and any(re.search(r"\b%s\(" % re.escape(h), body) for h in launching if h.startswith("_")):
                launching.add(name)
                grew = True
    return sorted(n for n in launching if not n.startswith("_"))


def test_every_kernel_wrapper_has_a_direct_gpu_test():
    names = kernel_wrappers()
    assert len(names) > 50 and {"axpy", "adam_range", "wattn_fwd", "full_rank", "lce_fwd_bwd"} <= set(names), names
    files = sorted(set(glob.glob(os.path.join(REPO, "tests", "test_*hip*.py")) + glob.glob(os.path.join(REPO, "tests", "test_*kernels*.py"))))
    text = "\n".join(open(f).read() for f in files)
    missing = [n for n in names if n not in EXEMPT and not re.search(r"\b(?:ops|o)\.%s\(" % re.escape(n), text)]
    assert not missing, "adt_amd/ops.py wrappers that no tests/test_*hip*.py or tests/test_*kernels*.py calls: %s" % missing
    stale = [n for n in EXEMPT if n not in names or re.search(r"\b(?:ops|o)\.%s\(" % re.escape(n), text)]
    assert not stale, "exemptions that are no longer needed: %s" % stale
