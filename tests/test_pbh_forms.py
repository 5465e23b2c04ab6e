"""k_pb_half's instantiations: the set the library holds, and every one of them once through its public entry point.

FORMS is the record of the set -- the template arguments <CHAIN, HYPER, BLUR, ALIGNED, SWAP, OPAQUE, YUV, SINK> of the 68 instantiations, grouped by the caller
that launches them (pixbuf.hip: pb_half_form_exists says the same in five clauses, pb_half_launch instantiates exactly those).

Without a GPU: the k_pb_half symbols of the built gfx950 code object are exactly FORMS.  Only symbol names are read.

On the GPU: each form byte for byte against the oracle on 520 x 44 -> 260 x 22, two tracks with different blend amounts.  260 output columns are three strips at
every strip width (120, 124, 128) with the last strip ending inside the frame, so a kernel launched with another form's strip width mis-addresses columns; 22 rows
are more than one band and an even height for the 4:2:0 sink.  Sources of the forms without OPAQUE carry random alpha (zeros included), so an OPAQUE instantiation
in their place differs; swap_rb, interp and blend / noblend all change the bytes of random frames.  What the comparison cannot tell: an OPAQUE = 0 kernel where
OPAQUE = 1 was meant -- the results are equal by design."""
import itertools
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

from tests.chain_ref import Tracks, oracle_chain_rgba
from tests.test_chain_sink import run as run_sink
from tests.test_chain_transcode import run as run_transcode
from tests.test_chain_yuv import run as run_yuv
from tests.test_pixbuf_scale import gpu_scale, orc_scale
from tests.util import align

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"
PIXBUF, OPAQUE, NOBLEND = 0x100, 0x200, 0x400
UYVY, YUV420P = 2, 4
SW, SH = 520, 44

B = (0, 1)
#            CHAIN HYPER BLUR ALIGNED SWAP OPAQUE YUV SINK
SCALER = {(0, hy, 0, al, 0, 0, 0, 0) for hy, al in itertools.product(B, B)}                                       # lgpu_pixbuf_scale (pb_scale_n)
CHAIN = {(ch, hy, 0, al, sw, 0, 0, 0) for ch, hy, al, sw in itertools.product((1, 2), B, B, B)}                  # lgpu_chain / lgpu_chain_amounts (pb_chain_half)
GAUSS = {(1, hy, 1, 0, sw, op, 0, 0) for hy, sw, op in itertools.product(B, B, B)}                               # ... with the gaussian, LGPU_INTERP_OPAQUE or not
YUV = {(ch, hy, 0, 0, sw, 1, 1, 0) for ch, hy, sw in itertools.product((1, 2), B, B)}                            # lgpu_chain_yuv420p
SINK = {(ch, hy, 0, 1, sw, 0, 0, sk) for ch, hy, sw, sk in itertools.product((1, 2), B, B, (1, 2))}              # lgpu_chain_to_yuv
BOTH = {(ch, hy, 0, 0, sw, 1, 1, sk) for ch, hy, sw, sk in itertools.product((1, 2), B, B, (1, 2))}              # lgpu_chain_yuv420p_to_yuv
FORMS = SCALER | CHAIN | GAUSS | YUV | SINK | BOTH


def test_the_record_has_68_forms():
    assert [len(s) for s in (SCALER, CHAIN, GAUSS, YUV, SINK, BOTH)] == [4, 16, 8, 8, 16, 16] and len(FORMS) == 68


def built_forms(so):
    """the template arguments of every k_pb_half instantiation in the library's gfx950 code object (k_pb_half3 is another kernel), padded to eight with zeros"""
    with tempfile.TemporaryDirectory() as tmp:
        local = os.path.join(tmp, "lib.so")
        shutil.copy(so, local)
        subprocess.run([OBJDUMP, "--offloading", local], cwd=tmp, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        syms = "".join(subprocess.run([OBJDUMP, "-t", os.path.join(tmp, f)], check=True, capture_output=True, text=True).stdout
                       for f in sorted(os.listdir(tmp)) if "gfx950" in f)
    forms = set()
    for m in re.finditer(r"\d+k_pb_halfI((?:Li\d+E)+)E", syms):
        args = [int(v) for v in re.findall(r"Li(\d+)E", m.group(1))]
        forms.add(tuple(args + [0] * (8 - len(args))))
    return forms


def test_the_library_holds_exactly_these_instantiations():
    if not os.path.exists(OBJDUMP):
        pytest.skip("no llvm-objdump in this image")
    so = os.path.join(ROOT, "lives_amd", "liblivesgpu.so")
    if not os.path.exists(so):
        import __graft_entry__ as g
        g.build()
    built = built_forms(so)
    assert built, "no k_pb_half symbol in the library's gfx950 code object"
    missing, extra = sorted(FORMS - built), sorted(built - FORMS)
    assert not missing and not extra, "k_pb_half<CHAIN, HYPER, BLUR, ALIGNED, SWAP, OPAQUE, YUV, SINK> -- recorded but not built: %s; built but not recorded: %s" % (missing, extra)


def rgba_sources(rng, n, opaque):
    """source frames with row padding; random alpha with zeros among it, or all-opaque where the caller says so (LGPU_INTERP_OPAQUE)"""
    srcs = [rng.integers(0, 256, (SH, align(SW * 4, 16) + 32), dtype=np.uint8) for _ in range(n)]
    for s in srcs:
        if opaque:
            s[:, 3::4] = 255
        else:
            assert (s[:, 3:SW * 4:4] == 0).any() and (s[:, 3:SW * 4:4] != 255).any()
    return srcs


@pytest.mark.gpu
@pytest.mark.parametrize("form", sorted(FORMS), ids=lambda f: "k_pb_half<%s>" % ",".join(map(str, f)))
def test_every_form_through_its_entry_point(gpu, orc, tune, form):
    chain, hyper, blur, aligned, swap, opaque, yuv, sink = form
    dw, dh = SW // 2, SH // 2
    rng = np.random.default_rng(0x68F0 + sum(v << (2 * i) for i, v in enumerate(form)))
    interp, blend = (3 if hyper else 2), chain != 2
    lut = rng.permutation(256).astype(np.uint8)
    if not blur and not yuv and not sink:
        tune("PBH_ALIGNED", aligned)                 # the other forms have their strips fixed
    if yuv or sink:
        fmt = UYVY if sink == 1 else YUV420P
        if yuv and sink:
            run_transcode(gpu, orc, rng, SW, SH, fmt, ntracks=2, interp=interp, blend=blend, lut=lut, swap=swap)
        elif yuv:
            run_yuv(gpu, orc, rng, SW, SH, ntracks=2, interp=interp, blend=blend, lut=lut, swap=swap)
        else:
            run_sink(gpu, orc, rng, SW, SH, fmt, ntracks=2, interp=interp, blend=blend, lut=lut, swap=swap)
    elif chain:
        srcs = rgba_sources(rng, 2, opaque)
        T = Tracks(rng, srcs, dw, dh, blend=blend)
        assert T.amounts[0] != T.amounts[1]
        prm = gpu.chain_params(SW, SH, srcs[0].strides[0], dw, dh, T.irow2, T.orow, swap_rb=swap, do_blur=blur, bf=0, lut=lut,
                               interp=interp | PIXBUF | (OPAQUE if opaque else 0) | (0 if blend else NOBLEND))
        gpu.chain_amounts(prm, gpu.chain_tracks(T.slots(T.d_src), T.slots(T.d_l2) if blend else None, T.slots(T.d_dst)), T.slots(T.amounts) if blend else None)
        for i in range(2):
            T.check(i, oracle_chain_rgba(orc, srcs[i], SW, SH, dw, dh, interp, swap, T.l2s[i] if blend else None, T.amounts[i], lut, blur=bool(blur)), str(form))
    else:
        plan = gpu.pixbuf_plan(SW, SH, dw, dh, 4, interp)
        assert plan["path"] == "HALF" and plan["aligned"] == aligned and plan["hyper"] == hyper, plan
        src = rgba_sources(rng, 1, False)[0][:, :SW * 4]
        got = gpu_scale(gpu, np.ascontiguousarray(src), SW, SH, dw, dh, 4, interp)
        assert (got == orc_scale(orc, np.ascontiguousarray(src), SW, SH, dw, dh, 4, interp)).all()
