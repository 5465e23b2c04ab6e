#!/usr/bin/env python3
"""tests/golden/weed_abi.json: the values the reference's public headers give every WEED_* name that include/lives_gpu_weed_abi.h restates
(libweed/weed.h, weed-palettes.h, weed-effects.h and src/colourspace.h; aliases such as WEED_PALETTE_END resolved).  Only names and their values
are stored: the fixture is data.  TEST INFRASTRUCTURE ONLY; tests/test_host_cpu.py checks the header against it."""
import json
import os
import re
import sys

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("LIVES_REFERENCE", "")      # the reference tree, as for build_ref.sh
OUT = os.path.join(ROOT, "tests", "golden")
OURS_ONLY = ("WEED_API_VERSION_MIN", "WEED_TRUE", "WEED_FALSE")     # ours; (weed_boolean_t) casts of 1 / 0 in weed.h:90-105

DEF = re.compile(r"^\s*#define\s+(WEED_[A-Z0-9_]+)\s+(\(?-?[0-9]+\)?|\"[^\"]*\"|\(1\s*<<\s*[0-9]+\))\s*(?:/[/*].*)?$", re.M)
ALIAS = re.compile(r"^\s*#define\s+(WEED_[A-Z0-9_]+)\s+(WEED_[A-Z0-9_]+)\s*$", re.M)


def defs(text):
    return {m.group(1): m.group(2).replace(" ", "").strip("()") for m in DEF.finditer(text)}


def main():
    assert os.path.isdir(os.path.join(REF, "libweed")), "usage: gen_golden_weed_abi.py REFERENCE_TREE (or LIVES_REFERENCE=...)"
    theirs = "".join(open(os.path.join(REF, "libweed", f)).read() for f in ("weed.h", "weed-palettes.h", "weed-effects.h"))
    theirs += open(os.path.join(REF, "src", "colourspace.h")).read()
    real = defs(theirs)
    for m in ALIAS.finditer(theirs):
        if m.group(2) in real and m.group(1) not in real:
            real[m.group(1)] = real[m.group(2)]
    mine = defs(open(os.path.join(ROOT, "include", "lives_gpu_weed_abi.h")).read())
    want = {k: real[k] for k in sorted(mine) if k not in OURS_ONLY and k in real}
    missing = sorted(k for k in mine if k not in OURS_ONLY and k not in real)
    assert not missing, "not weed ABI names: %s" % missing
    with open(os.path.join(OUT, "weed_abi.json"), "w") as f:
        json.dump(want, f, indent=1, sort_keys=True)
        f.write("\n")
    mpath = os.path.join(OUT, "manifest.json")
    man = json.load(open(mpath))
    man["groups"]["weed_abi.json"] = ("libweed/weed.h, weed-palettes.h, weed-effects.h, src/colourspace.h: the value of every WEED_* name "
                                      "include/lives_gpu_weed_abi.h restates (aliases resolved)")
    with open(mpath, "w") as f:
        json.dump(man, f, indent=1)
        f.write("\n")
    print("weed_abi.json: %d names" % len(want))


if __name__ == "__main__":
    main()
