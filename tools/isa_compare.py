#!/usr/bin/env python3
"""tools/isa_compare.py OLD.s NEW.s [--kernel k_pb_half] -- are the instantiations of a kernel template that exist in both builds the same machine code?

For a change that adds a compile-time policy to a kernel template and must leave every existing instantiation as it was.  Make the two listings with the build's own
flags (lives_amd/csrc/build.sh) on the parent's and on the changed source file:

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -mllvm -amdgpu-mfma-vgpr-form --cuda-device-only -S pixbuf.hip -o NEW.s

Functions are matched by their leading integer template arguments: a NEW instantiation whose argument list is OLD's followed by zeros (the new parameters at their
defaults) is OLD's twin; an instantiation with a type among its arguments is matched by its whole mangled name.  Compared: every instruction and label of the function body, comments and assembler directives dropped, basic-block labels renumbered
(their numbers carry the function's index in the file).  Exit status 1 when a twin is missing or differs."""
import argparse
import re
import sys


def bodies(path, kernel):
    out, cur = {}, None
    head = re.compile(r"^(_Z\w*%s\w*):" % re.escape(kernel))
    for line in open(path):
        m = head.match(line)
        if m:
            cur = m.group(1)
            out[cur] = []
            continue
        if cur is None:
            continue
        if line.startswith(".Lfunc_end"):
            cur = None
            continue
        s = line.split(";")[0].rstrip()
        if not s.strip():
            continue
        if s.lstrip().startswith("."):
            if re.match(r"^\.LBB\d+_\d+:", s):
                out[cur].append(re.sub(r"\.LBB\d+_", ".LBBN_", s))
            continue
        out[cur].append(re.sub(r"\.LBB\d+_", ".LBBN_", s))
    return out


def targs(name, kernel):
    m = re.search(r"%sI((?:Li\d+E)+)E" % re.escape(kernel), name)
    return tuple(int(v) for v in re.findall(r"Li(\d+)E", m.group(1))) if m else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--kernel", default="k_pb_half", help="unmangled template name; names it is a prefix of (k_pb_half3) are skipped")
    a = ap.parse_args()
    exact = re.compile(r"\d+%sI" % re.escape(a.kernel))
    old = {k: v for k, v in bodies(a.old, a.kernel).items() if exact.search(k)}
    new = {k: v for k, v in bodies(a.new, a.kernel).items() if exact.search(k)}
    by_args = {targs(k, a.kernel): k for k in new if targs(k, a.kernel) is not None}
    same = bad = 0
    for name, body in sorted(old.items()):
        t = targs(name, a.kernel)
        if t is None:                 # a type among the template arguments (k_pb_pairs<.., PbEpi>): the same mangled name or nothing
            twin, t = (name if name in new else None), (name,)
        else:
            twin = next((by_args[u] for u in by_args if u[:len(t)] == t and not any(u[len(t):])), None)
        if twin is None:
            print("MISSING in new: <%s>" % ", ".join(map(str, t)))
            bad += 1
        elif new[twin] != body:
            print("DIFFERS: <%s> (%d / %d lines)" % (", ".join(map(str, t)), len(body), len(new[twin])))
            bad += 1
        else:
            same += 1
    print("%s: %d instantiations in old, %d identical in new, %d missing or different; %d only in new" % (a.kernel, len(old), same, bad, len(new) - same))
    return 1 if bad or not old else 0


if __name__ == "__main__":
    sys.exit(main())
