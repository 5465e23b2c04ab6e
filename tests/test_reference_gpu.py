"""GPU: the kernels against the reference's OWN code at random shapes (tools/fuzz_oracle.py --subject gpu: lives_amd.ops in the place of the oracle),
not against the project's restatement of it.  One seed, 150 cases per family, 20 sequences for the stateful families, one whole sweep for the three table / planner families.  Reads oracle/_ref/*.so only;
skipped where they were never built."""
import os
import sys

import pytest

from oracle import pyoracle as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import fuzz_oracle as fo  # noqa: E402

needs_ref = pytest.mark.skipif(not po.have_ref(), reason="oracle/_ref not built (oracle/ref/build_ref.sh needs the reference tree)")
SEED, CASES, SEQUENCES = 20261018, 150, 20


@pytest.fixture(scope="module")
def subject(gpu, orc):
    return fo.GpuSubject()


@needs_ref
@pytest.mark.gpu
@pytest.mark.parametrize("family", list(fo.FAMILIES))
def test_gpu_equals_the_live_reference(subject, family):
    st = fo.run(CASES, SEED, [family], subject=subject, sequences=SEQUENCES, verbose=False)[family]
    want = SEQUENCES if family in fo.STATEFUL else CASES
    if family in fo.EXHAUSTIVE:                 # one whole sweep: every entry of the clamping and premultiply tables, every get_resizable and planner question
        want = fo.EXHAUSTIVE[family]
        assert st["compared"] == want, "the walk did not complete"
    print("%s: drawn %d redrawn %d compared %d skipped %d mismatching %d masked bytes %d" % (family, st["drawn"], st["redrawn"], st["compared"], st["skipped"], st["mismatching"], st["masked_bytes"]))
    assert st["mismatching"] == 0, st["first"]
    assert st["drawn"] == want and st["compared"] >= 0.95 * want
    assert st["overmasked"] == 0
