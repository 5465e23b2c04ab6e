#!/usr/bin/env python3
"""tools/isa_waits.py LISTING [--args 1,1,0,1,1,0] [--kernel k_pb_half] -- what does every `s_waitcnt vmcnt(N)` of a kernel's row loop wait for?

LISTING is a compiler listing (hipcc -S with the build's flags and --cuda-device-only, as for tools/isa_phases.py) or the text of `llvm-objdump -d` on a code object
of the built library.  The instantiation is picked by its leading integer template arguments; those not given are 0.

The loop: the first innermost loop of the function (a backward branch whose span holds no other backward branch) that holds both a buffer load and a buffer store:
k_pb_half's two-row walk.  It is walked in layout order, forward branches not taken -- the path on which every load of the loop is issued (a forward branch in it skips
loads, a band's last row, or edge-strip fix-ups without memory operations) -- twice round, so that the second trip starts from the steady state's queue.

vmcnt counts vector memory operations that have not returned, loads and stores alike, and they return IN ORDER: `vmcnt(N)` waits until at most N are outstanding, so it
forces every operation but the N youngest.  For every wait of the second trip the tool prints the operations it forces that were still outstanding and how many
instructions ago each was issued.  A wait is FLAGGED when it forces a load that was issued since the last buffer store of the walk, that is in the same row step: the
wave then stands through a whole memory latency with nothing of that row's prefetch left in flight.  Exit status 1 if a wait is flagged, 2 if no such loop is found.

Read: s_waitcnt, buffer_load*, buffer_store*, branches and labels.  Nothing else."""
import argparse
import re
import sys


def pattern(kernel, args):
    return r"_Z\w*?\d+%sI%s(?:Li0E)*E\w*" % (re.escape(kernel), "".join("Li%sE" % a for a in args.split(",")))


def parse_listing(text, kernel, args):
    """hipcc -S: [(op, operands, target index or None)] of the function, labels resolved"""
    m = re.search(r"^(%s):.*?\n(.*?)\n\.Lfunc_end" % pattern(kernel, args), text, re.S | re.M)
    if not m:
        return None, None
    ins, labels = [], {}
    for line in m.group(2).split("\n"):
        s = line.split(";")[0].strip()
        lm = re.match(r"^(\.LBB\d+_\d+):", s)
        if lm:
            labels[lm.group(1)] = len(ins)
            continue
        if not s or s.startswith(".") or s.endswith(":"):
            continue
        op, _, rest = s.partition(" ")
        ins.append([op, rest.strip(), None])
    for i in ins:
        if re.match(r"s_c?branch", i[0]):
            i[2] = labels.get(i[1].split(",")[-1].strip())
    return m.group(1), ins


def parse_objdump(text, kernel, args):
    """llvm-objdump -d: the same, branch targets from the `<symbol+0xOFFSET>` the disassembler prints behind the encoding"""
    m = re.search(r"^([0-9a-fA-F]+) <(%s)>:\n(.*?)(?=^[0-9a-fA-F]+ <|\Z)" % pattern(kernel, args), text, re.S | re.M)
    if not m:
        return None, None
    base, ins, at = int(m.group(1), 16), [], {}
    for line in m.group(3).split("\n"):
        im = re.match(r"^\s+(\w+)\s*(.*?)\s*//\s*([0-9A-Fa-f]+):(.*)$", line)
        if not im:
            continue
        at[int(im.group(3), 16)] = len(ins)
        tgt = None
        if re.match(r"s_c?branch", im.group(1)):
            tm = re.search(r"<[^>]*?\+0x([0-9a-fA-F]+)>", im.group(4))
            tgt = base + int(tm.group(1), 16) if tm else base if "<" in im.group(4) else None
        ins.append([im.group(1), im.group(2), tgt])
    for i in ins:
        if i[2] is not None:
            i[2] = at.get(i[2])
    return m.group(2), ins


def instructions(text, kernel, args):
    name, ins = parse_listing(text, kernel, args)
    if name is None:
        name, ins = parse_objdump(text, kernel, args)
    return name, ins


def row_loop(ins):
    """(first, last) instruction index of the first innermost loop with a buffer load and a buffer store"""
    spans = sorted((t, j) for j, (op, _, t) in enumerate(ins) if t is not None and t <= j)
    for a, b in spans:
        if any(a <= a2 and b2 <= b and (a2, b2) != (a, b) for a2, b2 in spans):
            continue
        ops = [ins[j][0] for j in range(a, b + 1)]
        if any(o.startswith("buffer_load") for o in ops) and any(o.startswith("buffer_store") for o in ops):
            return a, b
    return None


def walk(ins, span, trips=2):
    """-> [(position in the loop, N, [(op text, instructions ago, flagged)], flagged)] for the waits of the last trip"""
    a, b = span
    queue, out, now, last_store = [], [], 0, -1           # queue: [is_load, text, issued at]
    for trip in range(trips):
        for j in range(a, b + 1):
            op, rest, _ = ins[j]
            now += 1
            if op.startswith("buffer_load") or op.startswith("buffer_store"):
                queue.append((op.startswith("buffer_load"), "%s %s" % (op, rest.split(",")[0]), now))
                if op.startswith("buffer_store"):
                    last_store = now
            elif op == "s_waitcnt":
                m = re.search(r"vmcnt\((\d+)\)", rest)
                if not m:
                    continue
                n = int(m.group(1))
                forced, queue = queue[:max(len(queue) - n, 0)], queue[max(len(queue) - n, 0):]
                if trip == trips - 1:
                    rows = [(t, now - at, ld and at > last_store) for ld, t, at in forced]
                    out.append((j - a, n, rows, any(r[2] for r in rows)))
    return out


def report(name, ins, span, waits, out=sys.stdout):
    print("%s\nrow loop: instructions %d .. %d of the function (%d per trip)" % (name, span[0], span[1], span[1] - span[0] + 1), file=out)
    for pos, n, rows, bad in waits:
        print("  +%-4d s_waitcnt vmcnt(%d)%s" % (pos, n, "      <-- FLAGGED: forces a load of its own row step" if bad else ""), file=out)
        if not rows:
            print("          forces nothing that is still outstanding", file=out)
        for t, ago, f in rows:
            print("          %-34s issued %4d instructions ago%s" % (t, ago, "  *" if f else ""), file=out)
    print("%d waits on vmcnt in the loop, %d flagged" % (len(waits), sum(1 for w in waits if w[3])), file=out)


def check(text, args, kernel="k_pb_half"):
    """-> (mangled name, instructions, loop span, waits); span None when there is no such loop"""
    name, ins = instructions(text, kernel, args)
    if name is None:
        raise SystemExit("no %s<%s ..> in the listing" % (kernel, args))
    span = row_loop(ins)
    return name, ins, span, walk(ins, span) if span else []


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("listing")
    ap.add_argument("--args", default="1,1,0,1,1,0", help="leading integer template arguments of the instantiation")
    ap.add_argument("--kernel", default="k_pb_half")
    a = ap.parse_args()
    name, ins, span, waits = check(open(a.listing).read(), a.args, a.kernel)
    if span is None:
        print("%s: no loop with buffer loads and a buffer store" % name)
        return 2
    report(name, ins, span, waits)
    return 1 if any(w[3] for w in waits) else 0


if __name__ == "__main__":
    sys.exit(main())
