"""A property of the BUILT code objects, checked without a GPU (as tests/test_isa_hazards.py): in the steady state of k_pb_half's two-row loop no `s_waitcnt vmcnt(N)`
forces a load that was requested in the same row step.  vmcnt retires in order, so such a wait drains everything the wave has in flight and the wave stands through a
whole loaded memory latency: that is what the second half of every trip did while the next rows' requests sat under a run-time `if (r + 1 < rows)` -- the wait-count
pass chose the count of the path without them (profiles/r13/pbh_row_pipeline.md).  tools/isa_waits.py does the walk: the loop in layout order, the in-order queue of
buffer loads and stores, every vmcnt wait against it.  Checked on the headline instantiation (16-track chain, HYPER, strips of 64 quads, swap_rb), its SWAP = 0 twin
and the standalone HYPER scaler on the same strips.  Reads s_waitcnt, buffer_load*, buffer_store* and branches only."""
import importlib.util
import io
import os
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"
FORMS = {"chain, swap_rb (the headline)": "1,1,0,1,1,0", "chain": "1,1,0,1,0,0", "standalone scaler": "0,1,0,1,0,0"}


def _tool():
    spec = importlib.util.spec_from_file_location("isa_waits", os.path.join(ROOT, "tools", "isa_waits.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def disassembly():
    """the text of the gfx950 code object that holds k_pb_half"""
    if not os.path.exists(OBJDUMP):
        pytest.skip("no llvm-objdump in this image")
    so = os.path.join(ROOT, "lives_amd", "liblivesgpu.so")
    if not os.path.exists(so):
        import __graft_entry__ as g
        g.build()
    with tempfile.TemporaryDirectory() as tmp:
        local = os.path.join(tmp, "lib.so")
        shutil.copy(so, local)
        subprocess.run([OBJDUMP, "--offloading", local], cwd=tmp, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        for f in sorted(os.listdir(tmp)):
            if "gfx950" not in f:
                continue
            syms = subprocess.run([OBJDUMP, "-t", os.path.join(tmp, f)], check=True, capture_output=True, text=True).stdout
            if "9k_pb_halfI" in syms:
                return subprocess.run([OBJDUMP, "-d", os.path.join(tmp, f)], check=True, capture_output=True, text=True).stdout
    pytest.fail("no gfx950 code object with k_pb_half in the library")


@pytest.mark.parametrize("form", list(FORMS))
def test_no_wait_forces_a_load_of_its_own_row_step(disassembly, form):
    w = _tool()
    name, ins, span, waits = w.check(disassembly, FORMS[form])
    assert span is not None, "no loop with buffer loads and a buffer store in " + name
    ops = [ins[j][0] for j in range(span[0], span[1] + 1)]
    # the two-row loop: two stores, and both halves request their rows (two 16-byte loads each)
    assert sum(o.startswith("buffer_store") for o in ops) == 2 and sum(o == "buffer_load_dwordx4" for o in ops) == 4, "not the two-row loop: " + name
    assert waits, "no wait on vmcnt in the loop: the walk did not see the listing it expects"
    text = io.StringIO()
    w.report(name, ins, span, waits, out=text)
    assert not any(x[3] for x in waits), "a wait forces a load requested in the same row step:\n" + text.getvalue()
