"""CPU: the oracle against the LIVE reference builds under oracle/_ref at the shapes the GPU suite draws (tools/fuzz_oracle.py: one randomized
family per oracle entry that has a reference build; sizes, strides, in-place choices and parameters as tools/fuzz_ops.py draws them).  Skipped where
the reference was never built.  Two seeds, 1,000 cases per family (stateful families: 100 sequences of 5-12 frames; the three table / planner families: whole sweeps); wall time in docs/ORACLE.md."""
import os
import re
import sys

import pytest

from oracle import pyoracle as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import fuzz_oracle as fo  # noqa: E402

needs_ref = pytest.mark.skipif(not po.have_ref(), reason="oracle/_ref not built (oracle/ref/build_ref.sh needs the reference tree)")
SEEDS = (20261018, 7)
CASES, SEQUENCES = 1000, 100
_runs = {}


def live(seed):
    if seed not in _runs:
        _runs[seed] = fo.run(CASES, seed, subject="oracle", sequences=SEQUENCES, verbose=False)
    return _runs[seed]


@needs_ref
@pytest.mark.parametrize("seed", SEEDS)
def test_every_family_ran(seed):
    out = live(seed)
    assert list(out) == list(fo.FAMILIES), "a family of the driver's list did not run"
    line = fo.summary(out, "oracle", seed)
    got = fo.parse_summary(line)
    assert got and got["families"] == len(fo.FAMILIES) and got["mismatching"] == sum(s["mismatching"] for s in out.values()), line


@needs_ref
@pytest.mark.parametrize("family", list(fo.FAMILIES))
@pytest.mark.parametrize("seed", SEEDS)
def test_oracle_equals_the_live_reference(seed, family):
    st = live(seed)[family]
    want = SEQUENCES if family in fo.STATEFUL else CASES
    if family in fo.EXHAUSTIVE:                 # whole sweeps: every table entry / row / question, the planner queries included
        want = -(-CASES // fo.EXHAUSTIVE[family]) * fo.EXHAUSTIVE[family]
        assert st["compared"] == want and want >= fo.EXHAUSTIVE[family], "the walk did not complete"
    print("%s seed %d: drawn %d redrawn %d compared %d skipped %d mismatching %d masked bytes %d" % (family, seed, st["drawn"], st["redrawn"], st["compared"], st["skipped"], st["mismatching"], st["masked_bytes"]))
    assert st["mismatching"] == 0, st["first"]
    assert st["drawn"] == want
    assert st["compared"] >= 0.95 * st["drawn"], "fewer than 95 %% of the draws were compared: %r" % (st,)
    assert st["compared"] >= want * 0.95 and (st["compared"] >= 1000 or family in fo.STATEFUL)
    assert st["overmasked"] == 0, "a mask covered more bytes than the manifest describes"
    if not any(kind == "never" for (kind, _p, _r, _w) in fo.EXCEPTIONS.get(family, ())):
        assert st["redrawn"] == 0
    assert 3 * st["redrawn"] <= st["drawn"] + st["redrawn"], "more than a third of all draws fell to a `never` entry: the draw itself should avoid them"
    if not any(kind == "mask" for (kind, _p, _r, _w) in fo.EXCEPTIONS.get(family, ())):
        assert st["masked_bytes"] == 0, "a family without a mask entry in EXCEPTIONS masked bytes"


def test_ranges_are_those_of_fuzz_ops():
    """every range the driver copied from tools/fuzz_ops.py still stands there, in the block of its kind, with the same numbers"""
    text = open(os.path.join(ROOT, "tools", "fuzz_ops.py")).read()
    for kind, (line, nums) in fo.FUZZ_OPS_RANGES.items():
        m = re.search(r'kind == "%s":(.*?)\n            (?:elif kind|else:)' % kind, text, re.S)
        assert m, kind
        assert line in m.group(1), "tools/fuzz_ops.py no longer draws `%s` for kind %s" % (line, kind)
        assert tuple(int(v) for pair in re.findall(r"integers\((\d+), (\d+)\)", line) for v in pair) == nums, kind
    assert "rng.choice([1, 4, 8, 16, 32])" in text and fo.PAD_ALIGNS == [1, 4, 8, 16, 32]
    assert "extra_rows" not in text          # fr() of fuzz_ops.py pads rows only; the driver's spare rows are its own (mirrors)


def test_exception_table_is_well_formed():
    for family, rows in fo.EXCEPTIONS.items():
        assert family in fo.FAMILIES, family
        for (kind, pred, reason, where) in rows:
            assert kind in ("never", "mask") and callable(pred) and reason and where
    quirks = open(os.path.join(ROOT, "docs", "QUIRKS.md")).read()
    for rows in fo.EXCEPTIONS.values():
        for (_k, _p, _r, where) in rows:
            for qid in re.findall(r"\bK\d[a-z]?-[a-z]\b", where):
                assert "| %s |" % qid in quirks, "%s is not a row of docs/QUIRKS.md" % qid
