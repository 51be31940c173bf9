#!/usr/bin/env python
"""Driver of tools/launch_log.cpp: the launch log of the flagship executor over the whole case list, on the CPU.

    python tools/launch_log.py /path/to/parent/adt_amd/csrc/libadt_hip.so --against adt_amd/csrc/libadt_hip.so      # exit status 0: every record equal
    python tools/launch_log.py adt_amd/csrc/libadt_hip.so /tmp/digests.txt                                           # the digests of one build

One child process per switch arm (the ADT_* switches are read once per process); per arm 600 configurations (prec x heads x
maxlen x layers x batch), each running the trainer's three step forms with and without the ring prefetch, both step_begin forms, predict,
loss_seed, the plain calls, the four single-layer calls, rejected phase words and rejected configurations.  The output holds one line per arm and
configuration: launches, a digest of the configuration's log without the argument bytes and one with them.  Argument bytes the host code never
writes (struct padding, unused array tails) hold stack residue and differ from build to build, so two builds are compared with
`--against OTHER_LIB`: both in one process; a record is unequal if anything differs but bytes in the known padding of its argument struct or
behind the used part of a counted array (tables in launch_log.cpp).  The offsets that did differ are listed per kernel.  `--show "1 2 200 2 256" [--env ADT_X=0 ...]` prints one configuration's log itself.
Not part of the test suite: the comparison needs a build of the parent commit."""
import argparse
import concurrent.futures
import hashlib
import itertools
import os
import re
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/llvm/bin")
GATING = ["ADT_SEQ", "ADT_SEQ_LEAN", "ADT_SEQ_TT", "ADT_SEQ_BWD", "ADT_SEQ_ATTN_BWD", "ADT_SEQ_POST_BWD", "ADT_SEQ_PARTIALS", "ADT_XATTN_FUSED"]
ON_OFF = GATING + ["ADT_ATTN_SPLIT", "ADT_LNL_FUSED", "ADT_FOLD_PARTS", "ADT_FWD_FUSED", "ADT_EMBED3", "ADT_BCE_MERGED"]


def arms(which):
    """The switch arms of tests/test_step_plan_cpu.py as environments."""
    out = [{}] + [{k: "0"} for k in ON_OFF] + [{"ADT_ITEM_SORT": "1"}, {"ADT_SIDE_STREAM_DP": "1"}, {"ADT_SEQ_SPLIT": "1"}, {"ADT_SEQ_SPLIT": "2"}]
    out += [{"ADT_SIDE_STREAM": str(v)} for v in range(8)] + [{"ADT_SEQ_ABLATE": "0"}, {"ADT_SEQ_ABLATE": "1"}]
    if which == "all":
        out += [dict(zip(GATING, map(str, bits))) for bits in itertools.product((0, 1), repeat=8)]
    return out


def arg_sizes(lib, tmp):
    """{kernel symbol: [size of each explicit argument]} from the metadata notes of the gfx950 code objects in the library."""
    link = os.path.join(tmp, "lib.so")
    os.symlink(os.path.abspath(lib), link)
    subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", "lib.so"], cwd=tmp, check=True, stdout=subprocess.DEVNULL)
    sizes = {}
    for name in sorted(os.listdir(tmp)):
        if "amdgcn" not in name:
            continue
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", name], cwd=tmp, check=True, capture_output=True, text=True).stdout
        args, size = [], None
        for line in notes.splitlines():
            if line.startswith("  - ."):      # the next kernel
                args = []
            m = re.match(r"^\s+(?:- )?\.size:\s+(\d+)", line)
            if m:
                size = int(m.group(1))
            m = re.match(r"^\s+(?:- )?\.value_kind:\s+(\S+)", line)
            if m and not m.group(1).startswith("hidden_"):
                args.append(size)
            m = re.match(r"^    \.name:\s+(\S+)", line)
            if m:
                sizes[m.group(1)] = args
                args = []
    return sizes


def build(tmp):
    exe = os.path.join(tmp, "launch_log")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O2", "-Wall", "-Wextra", "-rdynamic", "-o", exe, os.path.join(HERE, "launch_log.cpp"), "-ldl"])
    return exe


def run_arm(exe, lib, table, env, extra):
    e = {k: v for k, v in os.environ.items() if not k.startswith("ADT_")}
    e.update(env)
    p = subprocess.run([exe, lib, table, "0"] + extra, env=e, capture_output=True, text=True)
    if p.returncode != 0:
        raise RuntimeError("arm %r: exit %d\n%s" % (env, p.returncode, p.stderr[-2000:]))
    return p.stdout.splitlines()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("lib")
    ap.add_argument("out", nargs="?")
    ap.add_argument("--arms", choices=["named", "all"], default="all")
    ap.add_argument("--jobs", type=int, default=min(16, os.cpu_count() or 1))
    ap.add_argument("--against", metavar="LIB", help="a second build: both in one process, every record compared (see launch_log.cpp)")
    ap.add_argument("--show", help='"prec H L layers B": print that configuration\'s log')
    ap.add_argument("--env", action="append", default=[], help="ADT_X=value for --show")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        exe = build(tmp)
        table = os.path.join(tmp, "argsizes.txt")
        with open(table, "w") as f:
            for name, sizes in sorted(arg_sizes(a.lib, tmp).items()):
                f.write("%s %d %s\n" % (name, len(sizes), " ".join(map(str, sizes))))
        lib = os.path.abspath(a.lib)
        if a.show:
            env = {k: v for k, v in os.environ.items() if not k.startswith("ADT_")}
            env.update(kv.split("=", 1) for kv in a.env)
            return subprocess.call([exe, lib, table, "0"] + a.show.split(), env=env)
        todo = arms(a.arms)
        with concurrent.futures.ThreadPoolExecutor(a.jobs) as pool:
            runs = [pool.submit(run_arm, exe, lib, table, env, [os.path.abspath(a.against)] if a.against else []) for env in todo]
            lines = []
            for env, r in zip(todo, runs):
                tag = ",".join("%s=%s" % kv for kv in sorted(env.items())) or "default"
                lines += ["%s : %s" % (tag, line) for line in r.result()]
    text = "\n".join(lines) + "\n"
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    if not a.against:      # per configuration: launches, digest without the argument bytes, digest with them
        shape = "\n".join(" ".join(line.split()[:-1]) for line in lines) + "\n"
        print("%d arms, %d cases, sha256 without argument bytes %s, with %s" % (len(todo), len(lines), hashlib.sha256(shape.encode()).hexdigest(),
                                                                                hashlib.sha256(text.encode()).hexdigest()))
        return 0
    totals, diffs, other = [0, 0, 0], {}, []
    for line in lines:
        f = line.split(" : ", 1)[1].split()
        if f[0] == "configs":
            totals = [t + int(v) for t, v in zip(totals, f[1::2])]
        elif f[0] == "argdiff":
            diffs.setdefault((f[2], f[3]), set()).update(int(v) for v in f[4:])
        else:
            other.append(line)
    print("%d arms, %d cases, %d launches, %d unequal records" % (len(todo), totals[0], totals[1], totals[2]))
    print("\n".join(other[:20]))
    for (kernel, arg), offs in sorted(diffs.items()):
        print("argument bytes that differ: %s %s: %s" % (kernel, arg, " ".join(map(str, sorted(offs)))))
    return 1 if totals[2] else 0


if __name__ == "__main__":
    sys.exit(main())
