#!/usr/bin/env python3
"""count ISA instructions of one kernel

    isa_phases.py file.s mangled-name-substring
        per segment between s_barrier's: instructions by unit and by opcode

    isa_phases.py --row-budget OLD.s NEW.s [--args 1,1,0,1,1,0]
        the two-row loop of one k_pb_half instantiation (HYPER chain forms), parent against new: vector instructions per OUTPUT row by phase of the row's arithmetic,
        as a markdown table (profiles/r10/pbh_isa_budget.md), then registers, LDS and scratch of both.  Make the listings with the build's own flags:
        hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -mllvm -amdgpu-mfma-vgpr-form --cuda-device-only -S pixbuf.hip -o NEW.s

How --row-budget tells the phases apart (k_pb_half's loop has no barriers; the scheduler interleaves the phases, so position says nothing):
    premultiply            SDWA multiplies that write one 16-bit half (pb_premul_pair), v_perm_b32 with the alpha-pair selector 0x0c070c03
    exchange               v_mov_b32_dpp; every other SDWA multiply out of inline assembly (the strip-edge pixel's products in the parent, the two raw neighbours' in the
                           new form); the compiler's own alpha x {65536, 1, 0} multiply of the parent (src1_sel:DWORD); v_cmp / v_cndmask (edge lanes)
    H                      v_add_u32_sdwa, v_dot2_u32_u16
    V                      multiplies and multiply-adds by the literal 7, v_add3_u32
    reciprocal and colours every f64 instruction and conversion, v_max_u32, the alpha's shift by a scalar register
    blend                  the compiler's SDWA multiplies and shifts, 24-bit multiplies without the 7, v_perm_b32 with another selector, v_dot4_u32_u8, shifts right by 8
    LUT and pack           v_lshlrev_b32_e32, v_lshl_or_b32, v_or3_b32
    moves                  v_mov_b32_e32, v_mov_b64_e32
    SALU                   every s_ instruction (s_nop and s_waitcnt among them, also listed apart)"""
import re, sys, collections

PHASES = ["premultiply", "exchange", "H", "V", "reciprocal and colours", "blend", "LUT and pack", "moves", "other VALU", "SALU", "(of SALU: s_nop)", "(of SALU: s_waitcnt)",
          "LDS", "VMEM"]


def function(text, pat):
    m = re.search(r"^(_Z\w*" + re.escape(pat) + r"\w*):.*?\n(.*?)\n\.Lfunc_end", text, re.S | re.M)
    if not m:
        raise SystemExit("no function matches " + pat)
    k = text.find(".amdhsa_kernel " + m.group(1))
    return m.group(1), m.group(2).split("\n"), text[k:text.find(".end_amdhsa_kernel", k)]


def loop_of(lines):
    """the first innermost loop: from its header label to the last branch back to it"""
    for i, l in enumerate(lines):
        mm = re.match(r"^(\.LBB\d+_\d+):.*Inner Loop Header", l)
        if mm:
            back = [j for j, x in enumerate(lines) if re.search(r"s_c?branch\w*\s+" + re.escape(mm.group(1)) + r"\b", x)]
            return lines[i:max(back) + 1]
    raise SystemExit("no inner loop")


def classify(op, rest, in_asm, consts):
    if op.startswith("s_"):
        return "SALU"
    if op.startswith("ds_"):
        return "LDS"
    if op.startswith(("buffer_", "global_")):
        return "VMEM"
    if not op.startswith("v_"):
        return "other VALU"
    if op == "v_mul_u32_u24_sdwa":
        if "dst_sel:WORD_" in rest:
            return "premultiply"
        return "exchange" if in_asm or "src1_sel:DWORD" in rest else "blend"
    if op == "v_perm_b32":
        sel = rest.split(",")[-1].strip()
        return "premultiply" if consts.get(sel) == 0x0C070C03 else "blend"
    if op in ("v_mov_b32_dpp", "v_cndmask_b32_e64", "v_cndmask_b32_e32") or op.startswith("v_cmp"):
        return "exchange"
    if op in ("v_add_u32_sdwa", "v_dot2_u32_u16"):
        return "H"
    if op in ("v_mul_u32_u24_e32", "v_mad_u32_u24"):
        return "V" if re.search(r"(^|,)\s*7\s*(,|$)", rest) else "blend"
    if op == "v_add3_u32":
        return "V"
    if "f64" in op or op == "v_max_u32_e32":
        return "reciprocal and colours"
    if op == "v_lshrrev_b32_e32":
        return "reciprocal and colours" if re.match(r"\s*v\d+,\s*s\d+,", rest) else "blend"
    if op in ("v_lshlrev_b32_sdwa", "v_dot4_u32_u8"):
        return "blend"
    if op in ("v_lshlrev_b32_e32", "v_lshl_or_b32", "v_or3_b32"):
        return "LUT and pack"
    if op in ("v_mov_b32_e32", "v_mov_b64_e32"):
        return "moves"
    return "other VALU"


def budget(path, pat):
    name, lines, tail = function(open(path).read(), pat)
    consts = {}
    for l in lines:
        mm = re.match(r"\s*s_mov_b32\s+(s\d+),\s*(0x[0-9a-fA-F]+)", l)
        if mm:
            consts[mm.group(1)] = int(mm.group(2), 16)
    cnt, in_asm = collections.Counter(), False
    for l in loop_of(lines):
        s = l.strip()
        if s.startswith(";;#ASMSTART"):
            in_asm = True
        elif s.startswith(";;#ASMEND"):
            in_asm = False
        s = s.split(";")[0].strip()
        if not s or s.startswith(".") or s.endswith(":"):
            continue
        op, _, rest = s.partition(" ")
        ph = classify(op, rest, in_asm, consts)
        cnt[ph] += 1
        if op in ("s_nop", "s_waitcnt"):
            cnt["(of SALU: %s)" % op] += 1
        if op.startswith("v_"):
            cnt["VALU"] += 1
    meta = {k: int(re.search(r"\.amdhsa_" + k + r"\s+(\d+)", tail).group(1)) for k in ("next_free_vgpr", "group_segment_fixed_size", "private_segment_fixed_size")}
    return name, cnt, meta


def row_budget(old, new, args):
    pat = "k_pb_halfI" + "".join("Li%sE" % a for a in args.split(","))
    (name, co, mo), (_, cn, mn) = budget(old, pat), budget(new, pat)
    print("`%s`\n" % name)
    print("| phase | parent, per output row | new, per output row |\n|---|---|---|")
    for ph in PHASES:
        if co[ph] or cn[ph]:
            print("| %s | %g | %g |" % (ph, co[ph] / 2, cn[ph] / 2))
    print("| **VALU, per output row** | **%g** | **%g** |" % (co["VALU"] / 2, cn["VALU"] / 2))
    print("| **VALU, per trip of the two-row loop** | **%d** | **%d** |" % (co["VALU"], cn["VALU"]))
    print("\n| | parent | new |\n|---|---|---|")
    for k, what in (("next_free_vgpr", "VGPRs"), ("group_segment_fixed_size", "static LDS bytes"), ("private_segment_fixed_size", "scratch bytes")):
        print("| %s | %d | %d |" % (what, mo[k], mn[k]))


def segments(path, pat):
    s = open(path).read()
    m = re.search(r"^(_Z\w*" + re.escape(pat) + r"\w*):.*?\n(.*?)\n\s*s_endpgm", s, re.S | re.M)
    body = m.group(2).split("\n")
    print(m.group(1), len(body), "lines")
    seg = 0
    cnt = collections.defaultdict(collections.Counter)
    for l in body:
        l = l.strip()
        if not l or l[0] in ";." or l.endswith(":"):
            continue
        op = l.split()[0]
        if op == "s_barrier":
            seg += 1
            continue
        k = ("mfma" if op.startswith("v_mfma") else "valu" if op.startswith("v_") else "ds" if op.startswith("ds_") else
             "vmem" if op.startswith(("global_", "buffer_")) else "salu" if op.startswith("s_") else "other")
        cnt[seg][k] += 1
        cnt[seg]["op:" + op] += 1
    for sg in sorted(cnt):
        c = cnt[sg]
        print("segment", sg, {k: v for k, v in c.items() if not k.startswith("op:")})
        print("    ", " ".join("%s:%d" % (k[3:], v) for k, v in sorted(c.items(), key=lambda kv: -kv[1]) if k.startswith("op:"))[:900])
    mm = re.search(r"\.amdhsa_next_free_vgpr (\d+)", s[m.end():m.end() + 6000])
    if mm:
        print("next_free_vgpr", mm.group(1))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--row-budget":
        a = sys.argv[2:]
        args = "1,1,0,1,1,0,0,0"
        if "--args" in a:
            i = a.index("--args")
            args = a[i + 1]
            del a[i:i + 2]
        row_budget(a[0], a[1], args)
    else:
        segments(sys.argv[1], sys.argv[2])
