"""Every entry point on buffers at every address and pitch alignment, bit for bit against the CPU oracle.

The other suites upload through tests/util.py:dev(), whose buffers start at multiples of 256 bytes, and mostly use pitches that are multiples of 32.  The library
picks its kernels by exactly those bits: about sixty host-side decisions of the form "aligned, so the vector / cell form; otherwise the fallback", and about
twenty-five branches inside kernels that test a pointer's low bits.  Here every buffer an entry point takes is placed, through tests/offset_buffers.py:dev_at(),

  aligned            all bases 0 mod 64, all pitches 0 mod 16 (the control)
  NAME+o             one buffer at each power of two o with r <= o < m, everything else aligned; r is the alignment the entry point's LGPU_REQUIRE demands of
                     that buffer (1 if none), m the largest alignment any dispatcher or in-kernel test looks at
  all                every buffer at once at its own r (byte data: 1, 2, 3, ... so that the buffers differ)
  pitch+8 .. pitch+1 aligned bases, pitches 8 mod 16, 4 mod 8, 2 mod 4 and odd, as far as each buffer's r admits
  base12-pitch4      base 12 mod 16 with pitch 4 mod 16: the rows cycle through all four residues
  NAME-refused       one step below r: the call returns LGPU_E_BADARG and no byte of any buffer changes (host-side checks: nothing is launched).  The entry points
                     that serve one launch or nothing (lgpu_gauss5_colorkey, lgpu_chain_yuv420p, the YUV sinks) answer LGPU_E_UNSUPPORTED between r and the
                     alignment of their kernel; those classes are held to the same "nothing changed"

at a width and height that satisfy every non-address condition of the fastest form, so that the address alone decides.  Frames are a few KB.

Each op has a plain-Python restatement of its dispatcher's address rule (rule_*).  It is evaluated on the planned address class and, on the GPU, again on the
data_ptr() and pitches of the buffers that were really handed over; both must name the same form, and the cases whose form matters carry the expected name in the
table (EXPECT), so a case cannot silently stop exercising what it names.  FORMS lists, per op, the set of forms its cases must reach between them.
test_address_tests_match_the_sources (no GPU) counts the lines of lives_amd/csrc/*.hip that test address bits and fails when one is added, until the tables here
follow.  Every case also runs with gpu=None (test_oracle_accepts_every_case): inputs, oracle, the oracle's own guard bytes and the restated rule, without a GPU.

gfx950 serves unaligned vector loads and stores to global memory, so a dispatcher that wrongly picks a vector form can still produce the right bytes: these tests
check bytes, not which kernel ran.  What they catch is arithmetic that depends on the address class: shifted tap matrices and window origins (k_half8s' xoff),
head and tail handling (k_clamp_switch), pointers rounded down to a chunk, and the fallback kernels themselves at shapes they otherwise never see.

A comparison is the whole allocation: the bytes in front of the frame, image, row padding, two guard rows and the bytes behind (offset_buffers.same_whole_at).
No tolerances and no masks: the oracle writes its "intent" values where the reference is undefined, as in tests/test_gpu_parity.py.
"""
import collections
import ctypes
import glob
import os
import re
import zlib

import numpy as np
import pytest

from oracle import pyoracle as po
from tests.offset_buffers import dev_at, same_whole_at, whole
from tests.util import align, frame

G = pytest.mark.gpu
P = po.P
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 2
BADARG, UNSUPPORTED = "LGPU_E_BADARG", "LGPU_E_UNSUPPORTED"
CODES = {BADARG: -2, UNSUPPORTED: -3}


def seeded(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def pitch16(nbytes):
    """the control pitch: 0 mod 16 with at least 16 bytes of row padding"""
    return align(nbytes + 16, 16)


# ---------------------------------------------------------------------------------------------- the source scan
# the lines that test address bits.  Directly: a uintptr_t and a mask of 1, 3, 7 or 15 (or a selection between two of them) on one line.  Through gathered bits: one of
# the variables the dispatchers OR addresses and pitches into, under such a mask
MASK = r"\(?(?:1|3|7|15|2 \* s_nc - 1|s_nc == 1 \? 7 : 15|(?:psize|ips|ops) == 4 \? 15 : 3|(?:a\.)?(?:out_alpha|in_alpha) \? 15 : 3)\b"
ADDRESS_TEST = re.compile(r"&\s*" + MASK + r"(?!\s*[0-9])")
BITS_TEST = re.compile(r"\b(?:sb|db|bits|sbits|dbits|d0bits|d12bits|pbits|pb|all|src_bits|dst_bits|py|pd|lb)\s*(?:\|[^&]{0,60}\))?\s*&\s*" + MASK)
# per file: the count this module's tables were written against
ADDRESS_TESTS = {'effects.hip': 13, 'fused.hip': 2, 'palette.hip': 37, 'pixbuf.hip': 14, 'resize.hip': 9, 'stencil.hip': 10, 'swizzle.hip': 8, 'yuv.hip': 4}


def address_tests_in(text):
    return sum(1 for line in text.splitlines() if ("uintptr_t" in line and ADDRESS_TEST.search(line)) or BITS_TEST.search(line))


def test_the_scan_reads_the_idioms():
    assert address_tests_in("  for (int i = 0; i < ntracks; i++) if ((uintptr_t)t.src[i] & 15) xoff = 0;") == 1
    assert address_tests_in("  const size_t head = (16 - (reinterpret_cast<uintptr_t>(buf) & 15)) & 15;") == 1
    assert address_tests_in("      (((uintptr_t)dst_d[0] | (uintptr_t)orow[0]) & (a.out_alpha ? 15 : 3)) == 0 && (unsigned long long)(width >> 2) * height < (1ull << 31)) {") == 1
    assert address_tests_in("  uintptr_t sb = (uintptr_t)irow, db = (uintptr_t)orow;") == 0
    assert address_tests_in("  const uint32_t addr = (uint32_t)(uintptr_t)(h8s_lptr)win + (uint32_t)lane * 8u;") == 0
    assert address_tests_in("  if ((bits & 15) == 0) {") == 1 and address_tests_in("    form_s = (py & (2 * s_nc - 1)) == 0 && (pd & (s_nc == 1 ? 7 : 15)) == 0;") == 1
    assert address_tests_in("  if (!epi && channels == 4 && dw == 2 * sw && (sw & 1) == 0 && ((sbits | (unsigned)irow) & 7) == 0 && ((dbits | (unsigned)orow) & 15) == 0 &&") == 1
    assert address_tests_in("  if ((psize != 3 && psize != 4) || (width & 3) || (bits & (psize == 4 ? 15 : 3))) return LGPU_E_UNSUPPORTED;") == 1
    assert address_tests_in("  if ((irow & 3) || (orow & 3)) return LGPU_E_UNSUPPORTED;") == 0 and address_tests_in("      if (off + 512 <= B1) asm volatile(\"x\" :: \"v\"(addr) : \"memory\");") == 0


def test_address_tests_match_the_sources():
    """per file, the lines that test a pointer's low bits.  A new one is a new dispatch decision or in-kernel branch: add its forms to the rule_* function and the
    cases of the entry point that reaches it, then update ADDRESS_TESTS"""
    found = {}
    for path in sorted(glob.glob(os.path.join(ROOT, "lives_amd", "csrc", "*.hip"))):
        with open(path) as f:
            found[os.path.basename(path)] = address_tests_in(f.read())
    found = {k: v for k, v in found.items() if v or k in ADDRESS_TESTS}
    assert found == ADDRESS_TESTS, ("the address tests in lives_amd/csrc changed (file: lines now, lines this module was written against): %s -- add the new decision to "
                                    "the rule_* function and the case table of its entry point in tests/test_address_alignment.py, then update ADDRESS_TESTS" %
                                    {k: (found.get(k), ADDRESS_TESTS.get(k)) for k in set(found) | set(ADDRESS_TESTS) if found.get(k) != ADDRESS_TESTS.get(k)})


def test_dev_at_builds_the_view_it_promises():
    """the helper itself, in host memory: the base residue, the pitch, the contents, and that same_whole_at() sees a byte written in front of, inside the padding of,
    and behind the frame"""
    a = seeded("dev_at").integers(0, 256, (5, 23), dtype=np.uint8)
    for off in (0, 1, 5, 12, 63):
        v = dev_at(a, off, device="cpu")
        assert v.data_ptr() % 64 == off and v.stride(0) == 23 and (v.numpy() == a).all()
        same_whole_at(v, a, a, 3, "untouched")
        for pos in (v.lgpu_start - 1, v.lgpu_start + 22, v.lgpu_start + a.size):
            v.lgpu_flat[pos] ^= 0xFF
            with pytest.raises(AssertionError):
                same_whole_at(v, a, a, 3, "touched")
            v.lgpu_flat[pos] ^= 0xFF
        want = a.copy()
        want[4, 0] ^= 1
        with pytest.raises(AssertionError, match="the oracle wrote past the frame"):
            same_whole_at(v, want, a, 3, "oracle")
        assert whole(v).size == 64 + 64 + a.size + 64


# ---------------------------------------------------------------------------------------------- placing the buffers of one case
def pl(dp=None, **off):
    """a placement: base offsets by buffer name, pitch deltas by buffer family (the buffers of a batch share one pitch)"""
    return {"off": off, "dp": dp or {}}


class Stage:
    """the buffers of one case.  gpu=None: nothing is uploaded, addresses are the planned offsets (the oracle-only pass and the planned form)"""

    def __init__(self, gpu, place, tune=None, refusal=None):
        self.gpu, self.place, self.tune, self.refusal = gpu, {"off": dict(place["off"]), "dp": dict(place["dp"])}, tune, refusal
        self.host, self.devs, self.fams = {}, {}, set()

    def pitch(self, family, nbytes):
        self.fams.add(family)
        return pitch16(nbytes) + self.place["dp"].get(family, 0)

    def put(self, name, arr):
        """register a buffer as it is uploaded (a copy is kept: the oracle may then work on `arr` in place)"""
        self.host[name] = arr.copy()
        return arr

    def dev(self, name):
        if name not in self.devs:
            self.devs[name] = dev_at(self.host[name], self.place["off"].get(name, 0))
        return self.devs[name]

    def reupload(self, name):
        """the upload again, at the same address: between a batch and the single-frame calls that follow it on the same buffers, so that those calls meet sources
        (in place) and destinations (noise) as the batch met them and have to write every byte themselves"""
        import torch
        v = self.dev(name)
        v.lgpu_flat.copy_(torch.from_numpy(v.lgpu_image))

    def addr(self, name):
        return self.dev(name).data_ptr() if self.gpu is not None else self.place["off"].get(name, 0)

    def bits(self, *names):
        """what the dispatchers OR together: the addresses and pitches of these buffers"""
        b = 0
        for n in names:
            b |= self.addr(n) | self.host[n].shape[1]
        return b

    def launch(self, fn):
        """run the entry point; a refusal case expects its code (LGPU_E_BADARG, or LGPU_E_UNSUPPORTED where the code says so) and every buffer as it was uploaded.
        Returns whether there is a result to compare"""
        from lives_amd.lib import LgpuError
        if not self.refusal:
            fn()
            return True
        with pytest.raises(LgpuError, match=r"\(%d\)" % self.refusal):
            fn()
        for name in self.devs:
            same_whole_at(self.devs[name], self.host[name], self.host[name], self.host[name].shape[0], "%s after a refused call" % name)
        return False

    def check(self, name, want, rows, what):
        before = self.host[name]
        assert (want[rows:] == before[rows:]).all(), "%s: the oracle wrote past the frame of %s" % (what, name)
        if self.gpu is not None:
            same_whole_at(self.dev(name), want, before, rows, "%s, buffer %s" % (what, name))

    def finish(self):
        known = set(self.host)
        assert set(self.place["off"]) <= known and set(self.place["dp"]) <= self.fams, "the placement %r names a buffer this case does not have (%s)" % (self.place, sorted(known))


def classes(bufs):
    """the address classes of one op.  bufs: (family, [names], r, m) -- r the alignment LGPU_REQUIRE demands, m the largest alignment anything looks at"""
    out = [("aligned", pl())]
    for fam, names, r, m in bufs:
        for n in names:
            o = r
            while o < m:
                out.append(("%s+%d" % (n, o), pl(**{n: o})))
                o *= 2
    off, i = {}, 0
    for fam, names, r, m in bufs:
        for n in names:
            i += 1
            off[n] = (r * i) % 16 or r
    out.append(("all", pl(**off)))
    for dp in (8, 4, 2, 1):
        d = {fam: dp for fam, names, r, m in bufs if dp % r == 0}
        if d:
            out.append(("pitch+%d" % dp, pl(dp=d)))
    if all(r <= 4 for fam, names, r, m in bufs):
        out.append(("base12-pitch4", pl(dp={fam: 4 for fam, names, r, m in bufs}, **{n: 12 for fam, names, r, m in bufs for n in names})))
    for fam, names, r, m in bufs:
        if r > 1:
            out.append(("%s-refused" % names[0], pl(**{names[0]: r // 2})))
    return out


def batch_classes(bufs, slot=1):
    """three frames, slot 1 at the class under test, slots 0 and 2 aligned.  bufs: (family, r, m); the buffers are called family + slot number"""
    out = [("aligned", pl())]
    for fam, r, m in bufs:
        o = r
        while o < m:
            out.append(("%s%d+%d" % (fam, slot, o), pl(**{"%s%d" % (fam, slot): o})))
            o *= 2
    out.append(("all", pl(**{"%s%d" % (fam, slot): (r * (i + 1)) % 16 or r for i, (fam, r, m) in enumerate(bufs)})))
    for fam, r, m in bufs:
        if r > 1:
            out.append(("%s%d-refused" % (fam, slot), pl(**{"%s%d" % (fam, slot): r // 2})))
    return out


def src_frame(rng, w, h, ps, stride, alpha_mix=False):
    return frame(rng, w, h, ps, stride=stride, extra_rows=GUARD, alpha_mix=alpha_mix)


def noise(rng, rows, stride):
    """a destination as it is before the call: random bytes, so that a byte the kernel should have left alone shows"""
    return rng.integers(0, 256, (rows + GUARD, stride), dtype=np.uint8)


def ptrs(ts):
    return (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


# ============================================================================================== swizzle.hip
def rule_swizzle(ib, ob, sb, db):
    iv = (sb & 15) == 0 if ib == 4 else (sb & 3) == 0
    ov = (db & 15) == 0 if ob == 4 else (db & 3) == 0
    return "k_swizzle<%d,%d>" % (ib, ob) if iv and ov else "k_swizzle_bytes"


def run_swizzle(orc, st, opname, use_lut, n):
    op = po.OPS.index(opname)
    ib, ob, w, h = po.OP_IBPP[op], po.OP_OBPP[op], 40, 6
    rng = seeded("swizzle", opname, use_lut, n)
    lut = rng.permutation(256).astype(np.uint8) if use_lut else None
    S, D = ["src%d" % i for i in range(n)], ["dst%d" % i for i in range(n)]
    srcs = [st.put(S[i], src_frame(rng, w, h, ib, st.pitch("src", w * ib))) for i in range(n)]
    wants = [st.put(D[i], noise(rng, h, st.pitch("dst", w * ob))) for i in range(n)]
    for i in range(n):
        orc.orc_swizzle(op, 0, P(srcs[i]), srcs[i].strides[0], P(wants[i]), wants[i].strides[0], w, h, P(lut))
    form = rule_swizzle(ib, ob, st.bits(*S), st.bits(*D))
    what = "swizzle %s lut=%d" % (opname, use_lut)
    if st.gpu is not None:
        gpu = st.gpu
        if n > 1:
            gpu.lib.call("lgpu_swizzle_batch", op, 0, ptrs([st.dev(x) for x in S]), srcs[0].strides[0], ptrs([st.dev(x) for x in D]), wants[0].strides[0], w, h,
                         lut.ctypes.data if use_lut else None, n, None)
            for i in range(n):
                st.check(D[i], wants[i], h, what + " batch frame %d" % i)
                st.reupload(D[i])       # back to noise: the single-frame call has to write every byte itself
        for i in range(n):              # the single-frame call on the same buffers
            gpu.swizzle(op, st.dev(S[i]), st.dev(D[i]), w, h, lut=lut)
    for i in range(n):
        st.check(D[i], wants[i], h, what + " frame %d" % i)
        st.check(S[i], srcs[i], h, what + " source %d" % i)
    if ib == ob and n == 1:             # in place
        wip = st.put("inplace", srcs[0].copy())
        orc.orc_swizzle(op, 0, P(wip), wip.strides[0], P(wip), wip.strides[0], w, h, P(lut))
        st.place["off"].setdefault("inplace", st.place["off"].get("src0", 0))
        if st.gpu is not None:
            st.gpu.swizzle(op, st.dev("inplace"), st.dev("inplace"), w, h, lut=lut)
        st.check("inplace", wip, h, what + " in place")
    return form


def rule_bits16(bits, fast, slow):
    return fast if (bits & 15) == 0 else slow


def run_gamma(orc, st, ps, af, rect, n):
    w, h = 40, 6
    x, y, rw, rh = (3, 2, 33, 3) if rect else (0, 0, w, h)
    rng = seeded("gamma", ps, af, rect, n)
    lut = rng.permutation(256).astype(np.uint8)
    N = ["pix%d" % i for i in range(n)]
    pix = [st.put(N[i], src_frame(rng, w, h, ps, st.pitch("pix", w * ps))) for i in range(n)]
    for a in pix:
        sub = a[y:, x * ps:]
        orc.orc_gamma_apply(sub.ctypes.data, a.strides[0], rw, rh, ps, af, P(lut))
    rs = pix[0].strides[0]
    bits = rs                          # the dispatcher looks at the first row of the rectangle: base + y * pitch
    for k in N:
        bits |= st.addr(k) + y * rs
    form = rule_bits16(bits, "k_gamma_apply", "k_gamma_apply_bytes")
    what = "gamma ps=%d af=%d rect=%d" % (ps, af, rect)
    if st.gpu is not None:
        gpu = st.gpu
        if n > 1:
            gpu.lib.call("lgpu_gamma_apply_batch", ptrs([st.dev(k) for k in N]), rs, x, y, rw, rh, ps, af, lut.ctypes.data, n, None)
            for i in range(n):
                st.check(N[i], pix[i], h, what + " batch frame %d" % i)
                st.reupload(N[i])
        for i in range(n):
            gpu.gamma_apply(st.dev(N[i]), rw, rh, ps, lut, alpha_first=af, x=x, y=y)
    for i in range(n):
        st.check(N[i], pix[i], h, what + " frame %d" % i)
    return form


def run_premult(orc, st, af, un, n):
    w, h = 40, 6
    rng = seeded("premult", af, un, n)
    N = ["pix%d" % i for i in range(n)]
    pix = [st.put(N[i], src_frame(rng, w, h, 4, st.pitch("pix", w * 4), alpha_mix=True)) for i in range(n)]
    for a in pix:
        orc.orc_alpha_premult(P(a), a.strides[0], w, h, af, un)
    bits = st.bits(*N)
    form = BADARG if bits & 3 else rule_bits16(bits, "k_premult<true>", "k_premult<false>")
    what = "premult af=%d un=%d" % (af, un)
    if st.gpu is not None:
        gpu, rs = st.gpu, pix[0].strides[0]
        if n > 1:
            if not st.launch(lambda: gpu.lib.call("lgpu_alpha_premult_batch", ptrs([st.dev(k) for k in N]), rs, w, h, af, un, n, None)):
                return form
            for i in range(n):
                st.check(N[i], pix[i], h, what + " batch frame %d" % i)
                st.reupload(N[i])
        for i in range(n):
            if not st.launch(lambda: gpu.alpha_premult(st.dev(N[i]), w, h, alpha_first=af, un=un)):
                return form
    for i in range(n):
        st.check(N[i], pix[i], h, what + " frame %d" % i)
    return form


def run_byte_luts(orc, st, ps):
    w, h = 40, 6
    rng = seeded("byte_luts", ps)
    luts = rng.integers(0, 256, (ps, 256), dtype=np.uint8)
    src = st.put("src", src_frame(rng, w, h, ps, st.pitch("src", w * ps)))
    want = st.put("dst", noise(rng, h, st.pitch("dst", w * ps)))
    orc.orc_byte_luts(P(src), src.strides[0], P(want), want.strides[0], w, h, ps, luts.ctypes.data)
    if st.gpu is not None:
        st.gpu.byte_luts(st.dev("src"), st.dev("dst"), w, h, ps, luts)
    st.check("dst", want, h, "byte_luts ps=%d" % ps)
    st.check("src", src, h, "byte_luts ps=%d source" % ps)
    return "k_byte_luts<%d>" % ps            # one kernel: no address decision, the offsets only move its four-pixel groups


# ============================================================================================== effects.hip
def rule_mirror(ps, bits):
    return "k_mirror_v4" if ps == 4 and (bits & 15) == 0 else "k_mirror<%d>" % ps


def run_mirror(orc, st, mode, ps, n, inplace):
    w, h = 40, 6
    rng = seeded("mirror", mode, ps, n, inplace)
    S, D = ["src%d" % i for i in range(n)], ["dst%d" % i for i in range(n)]
    srcs = [st.put(S[i], src_frame(rng, w, h, ps, st.pitch("src", w * ps))) for i in range(n)]
    if inplace:
        D, wants = S, srcs
        for a in wants:
            orc.orc_mirror(mode, P(a), a.strides[0], P(a), a.strides[0], w, h, ps)
    else:
        wants = [st.put(D[i], noise(rng, h, st.pitch("dst", w * ps))) for i in range(n)]
        for i in range(n):
            orc.orc_mirror(mode, P(srcs[i]), srcs[i].strides[0], P(wants[i]), wants[i].strides[0], w, h, ps)
    form = rule_mirror(ps, st.bits(*(S + D)))
    what = "mirror mode=%d ps=%d inplace=%d" % (mode, ps, inplace)
    if st.gpu is not None:
        gpu, irow, orow = st.gpu, srcs[0].strides[0], wants[0].strides[0]
        if n > 1:
            gpu.lib.call("lgpu_mirror_batch", mode, ptrs([st.dev(k) for k in S]), irow, ptrs([st.dev(k) for k in D]), orow, w, h, ps, n, None)
            for i in range(n):
                st.check(D[i], wants[i], h, what + " batch frame %d" % i)
                st.reupload(D[i])
        for i in range(n):
            gpu.mirror(mode, st.dev(S[i]), st.dev(D[i]), w, h, ps)
    for i in range(n):
        st.check(D[i], wants[i], h, what + " frame %d" % i)
    return form


BLACK = {1: [16, 0, 0, 0], 3: [1, 2, 3, 0], 4: [0, 0, 0, 255]}


def rule_letterbox(ps, sb, db):
    if ps != 4:
        return "k_letterbox<%d>" % ps
    return BADARG if (sb | db) & 3 else "k_letterbox<4> vec" if (db & 15) == 0 else "k_letterbox<4>"


def run_letterbox(orc, st, ps, n):
    nw, nh, w, h = 40, 8, 33, 5
    rng = seeded("letterbox", ps, n)
    bp = np.array(BLACK[ps], np.uint8)
    S, D = ["src%d" % i for i in range(n)], ["dst%d" % i for i in range(n)]
    srcs = [st.put(S[i], src_frame(rng, w, h, ps, st.pitch("src", w * ps))) for i in range(n)]
    wants = [st.put(D[i], noise(rng, nh, st.pitch("dst", nw * ps))) for i in range(n)]
    for i in range(n):
        orc.orc_letterbox(P(srcs[i]), srcs[i].strides[0], w, h, P(wants[i]), wants[i].strides[0], nw, nh, ps, P(bp))
    form = rule_letterbox(ps, st.bits(*S), st.bits(*D))
    what = "letterbox ps=%d" % ps
    if st.gpu is not None:
        gpu, irow, orow = st.gpu, srcs[0].strides[0], wants[0].strides[0]
        if n > 1:
            if not st.launch(lambda: gpu.lib.call("lgpu_letterbox_batch", ptrs([st.dev(k) for k in S]), irow, w, h, ptrs([st.dev(k) for k in D]), orow, nw, nh, ps,
                                                  (ctypes.c_uint8 * 4)(*BLACK[ps]), n, None)):
                return form
            for i in range(n):
                st.check(D[i], wants[i], nh, what + " batch frame %d" % i)
                st.reupload(D[i])
        for i in range(n):
            if not st.launch(lambda: gpu.letterbox(st.dev(S[i]), st.dev(D[i]), w, h, nw, nh, ps, BLACK[ps])):
                return form
    for i in range(n):
        st.check(D[i], wants[i], nh, what + " frame %d" % i)
    return form


def run_letterbox_bars(orc, st, ps):
    nw, nh, ox, oy, w, h = 40, 8, 3, 1, 33, 5
    rng = seeded("bars", ps)
    before = st.put("dst", noise(rng, nh, st.pitch("dst", nw * ps)))
    want = before.copy()
    inner = want[oy:oy + h, ox * ps:(ox + w) * ps].copy()
    want[:nh, :nw * ps] = np.tile(np.array(BLACK[ps][:ps], np.uint8), nw)
    want[oy:oy + h, ox * ps:(ox + w) * ps] = inner
    form = BADARG if ps == 4 and st.bits("dst") & 3 else "k_letterbox_bars<%d>" % ps
    if st.gpu is not None:
        d = st.dev("dst")
        if not st.launch(lambda: st.gpu.lib.call("lgpu_letterbox_bars", d.data_ptr(), d.stride(0), nw, nh, ps, (ctypes.c_uint8 * 4)(*BLACK[ps]), ox, oy, w, h, None)):
            return form
    st.check("dst", want, nh, "letterbox bars ps=%d" % ps)
    return form


def rule_pixel2(ps, bits, argb=False):
    if ps == 4 and bits & 3:
        return BADARG
    if argb:
        return "k_chroma_argb"
    return "k_pixel2<%d> vec" % ps if (bits & (15 if ps == 4 else 3)) == 0 else "k_pixel2<%d> bytes" % ps


def run_pixel2(orc, st, kind, ps, extra, n):
    """lgpu_blend_chroma (extra: alpha first) / _luma (extra: type) / _multi (extra: type) / lgpu_colorkey, and lgpu_colorkey_batch for n > 1"""
    w, h, bf = 40, 6, 100
    rng = seeded("pixel2", kind, ps, extra, n)
    A, B, D = ["a%d" % i for i in range(n)], ["b%d" % i for i in range(n)], ["dst%d" % i for i in range(n)]
    s1 = [st.put(A[i], src_frame(rng, w, h, ps, st.pitch("a", w * ps), alpha_mix=True)) for i in range(n)]
    s2 = [st.put(B[i], src_frame(rng, w, h, ps, st.pitch("b", w * ps), alpha_mix=True)) for i in range(n)]
    wants = [st.put(D[i], noise(rng, h, st.pitch("dst", w * ps))) for i in range(n)]
    r1, r2, ro = s1[0].strides[0], s2[0].strides[0], wants[0].strides[0]
    for i in range(n):
        a, b, out = P(s1[i]), P(s2[i]), P(wants[i])
        if kind == "chroma":
            orc.orc_blend_chroma(a, r1, b, r2, out, ro, w, h, ps, extra, bf)
        elif kind == "luma":
            orc.orc_blend_luma(extra, a, r1, b, r2, out, ro, w, h, ps, 0, bf, 0)
        elif kind == "multi":
            orc.orc_blend_multi(extra, a, r1, b, r2, out, ro, w, h, 0, bf)
        else:
            orc.orc_colorkey(a, r1, b, r2, out, ro, w, h, 0, 0.35, 0.7, 40, 200, 90, 0)
    form = rule_pixel2(ps, st.bits(*(A + B + D)), argb=(kind == "chroma" and ps == 4 and extra))
    what = "%s ps=%d %s" % (kind, ps, extra)

    def single(i):
        gpu, d1, d2, dd = st.gpu, st.dev(A[i]), st.dev(B[i]), st.dev(D[i])
        if kind == "chroma":
            gpu.blend_chroma(d1, d2, dd, w, h, ps, bf, alpha_first=extra)
        elif kind == "luma":
            gpu.blend_luma(extra, d1, d2, dd, w, h, ps, 0, bf)
        elif kind == "multi":
            gpu.blend_multi(extra, d1, d2, dd, w, h, 0, bf)
        else:
            gpu.colorkey(d1, d2, dd, w, h, 0, 0.35, 0.7, (40, 200, 90))

    if st.gpu is not None:
        if n > 1:
            assert kind == "colorkey"
            st.gpu.lib.call("lgpu_colorkey_batch", ptrs([st.dev(k) for k in A]), r1, ptrs([st.dev(k) for k in B]), r2, ptrs([st.dev(k) for k in D]), ro, w, h, 0, 0.35, 0.7,
                            40, 200, 90, n, None)
            for i in range(n):
                st.check(D[i], wants[i], h, what + " batch frame %d" % i)
                st.reupload(D[i])
        for i in range(n):
            if not st.launch(lambda: single(i)):
                return form
    for i in range(n):
        st.check(D[i], wants[i], h, what + " frame %d" % i)
    return form


# ============================================================================================== resize.hip
def rule_resize(ps, two_to_one, sb, db):
    """lgpu_resize: half8_applies (exact 2:1 on 4-aligned frames), then plan_sep with vec on or off, then the generic two passes"""
    if ps == 4 and ((sb | db) & 3) == 0:
        if two_to_one:
            return "k_half8s xoff 1" if (sb & 15) == 0 else "k_half8s xoff 0"
        return "plan_sep vec 1" if (sb & 15) == 0 else "plan_sep vec 0"
    return "k_hpass_generic + k_vpass_generic"


def run_resize(orc, st, ps, sw, sh, dw, dh):
    rng = seeded("resize", ps, sw, sh, dw, dh)
    src = st.put("src", src_frame(rng, sw, sh, ps, st.pitch("src", sw * ps)))
    want = st.put("dst", noise(rng, dh, st.pitch("dst", dw * ps)))
    assert orc.orc_resize(P(src), src.strides[0], sw, sh, P(want), want.strides[0], dw, dh, ps, 3) == 0
    form = rule_resize(ps, sw == 2 * dw and sh == 2 * dh, st.bits("src"), st.bits("dst"))
    if st.gpu is not None:
        st.gpu.resize(st.dev("src"), st.dev("dst"), sw, sh, dw, dh, psize=ps, interp=3)
    st.check("dst", want, dh, "resize ps=%d %dx%d -> %dx%d" % (ps, sw, sh, dw, dh))
    st.check("src", src, sh, "resize source")
    return form


def rule_gauss5(ps, width, sb, db):
    """lgpu_gauss5: gauss5_rows (fused.hip), then for 4-byte pixels try_gauss5x and plan_sep, then the generic two passes"""
    if ps in (3, 4) and (width & 3) == 0 and ((sb | db) & (15 if ps == 4 else 3)) == 0:
        return "gauss5_rows"
    if ps == 4 and ((sb | db) & 3) == 0:
        if (sb & 7) == 0:
            return "k_gauss5x"
        return "plan_sep(5,5) vec 0"          # vec needs the source 16-aligned, and a 16-aligned source with a 4-aligned destination takes k_gauss5x above
    return "k_hpass_generic + k_vpass_generic"


def run_gauss5(orc, st, ps, w, h):
    rng = seeded("gauss5", ps, w, h)
    src = st.put("src", src_frame(rng, w, h, ps, st.pitch("src", w * ps)))
    want = st.put("dst", noise(rng, h, st.pitch("dst", w * ps)))
    orc.orc_gauss5(P(src), src.strides[0], P(want), want.strides[0], w, h, ps)
    form = rule_gauss5(ps, w, st.bits("src"), st.bits("dst"))
    if st.gpu is not None:
        st.gpu.gauss5(st.dev("src"), st.dev("dst"), w, h, psize=ps)
    st.check("dst", want, h, "gauss5 ps=%d %dx%d" % (ps, w, h))
    st.check("src", src, h, "gauss5 source")
    return form


def l2s_lut(orc):
    lut = np.zeros(256, np.uint8)
    assert orc.orc_gamma_lut8(1.0, po.GAMMA_LINEAR, po.GAMMA_SRGB, 1.4, P(lut)) == 1
    return lut


def rule_chain(two_to_one, blur, sb, l2b, db):
    """lgpu_chain on the polyphase arithmetic: lgpu_chain_check, then half8_applies / plan_sep (route_resize) for the resize stage (into scratch when the blur follows)"""
    if (sb | l2b | db) & 3:
        return BADARG
    stage = ("k_half8s xoff 1" if (sb & 15) == 0 else "k_half8s xoff 0") if two_to_one else ("plan_sep vec 1" if (sb & 15) == 0 else "plan_sep vec 0")
    return stage + (", blur from scratch" if blur else "")


def run_chain(orc, st, sw, sh, dw, dh, blur):
    ntr = 3
    rng = seeded("chain", sw, sh, dw, dh, blur)
    lut = l2s_lut(orc)
    S, L, D = ["src%d" % i for i in range(ntr)], ["l2%d" % i for i in range(ntr)], ["dst%d" % i for i in range(ntr)]
    srcs = [st.put(S[i], src_frame(rng, sw, sh, 4, st.pitch("src", sw * 4), alpha_mix=True)) for i in range(ntr)]
    l2s = [st.put(L[i], src_frame(rng, dw, dh, 4, st.pitch("l2", dw * 4), alpha_mix=True)) for i in range(ntr)]
    wants = [st.put(D[i], noise(rng, dh, st.pitch("dst", dw * 4))) for i in range(ntr)]
    irow, irow2, orow = srcs[0].strides[0], l2s[0].strides[0], wants[0].strides[0]
    for i in range(ntr):
        assert orc.orc_chain(P(srcs[i]), irow, sw, sh, P(l2s[i]), irow2, P(wants[i]), orow, dw, dh, 1, 3, blur, 77, P(lut)) == 0
    form = rule_chain(sw == 2 * dw and sh == 2 * dh, blur, st.bits(*S), st.bits(*L), st.bits(*D))
    if st.gpu is not None:
        gpu = st.gpu
        prm = gpu.chain_params(sw, sh, irow, dw, dh, irow2, orow, swap_rb=1, interp=3, do_blur=blur, bf=77, lut=lut)
        if not st.launch(lambda: gpu.chain(prm, gpu.chain_tracks([st.dev(k) for k in S], [st.dev(k) for k in L], [st.dev(k) for k in D]))):
            return form
    for i in range(ntr):
        st.check(D[i], wants[i], dh, "chain %dx%d -> %dx%d blur=%d track %d" % (sw, sh, dw, dh, blur, i))
    return form


# ============================================================================================== pixbuf.hip
def rule_pixbuf(ch, sw, sh, dw, dh, sb, db, aligned=1):
    """pb_scale_n: k_pb_double (exact 1:2), k_pb_half3 (3 channels, exact 2:1), k_pb_half (4 channels, exact 2:1; strips of 64 quads unless PBH_ALIGNED is 0),
    then the general kernels"""
    if ch == 4 and (sb | db) & 3:
        return BADARG
    if ch == 4 and dw == 2 * sw and dh == 2 * sh and (sw & 1) == 0:
        return "k_pb_double" if (sb & 7) == 0 and (db & 15) == 0 else "k_pb_up"
    if sw == 2 * dw and sh == 2 * dh:
        if ch == 3:
            return "k_pb_half3" if (sw & 7) == 0 and ((sb | db) & 3) == 0 else "k_pb_pairs<3>"
        if (sw & 3) == 0 and (sb & 15) == 0 and (db & 7) == 0:
            return "k_pb_half ALIGNED" if aligned else "k_pb_half plain"
        return "k_pb_gather"
    return "general"


def run_pixbuf(orc, st, ch, sw, sh, dw, dh, interp, n, aligned=1):
    rng = seeded("pixbuf", ch, sw, sh, dw, dh, interp, n, aligned)
    S, D = ["src%d" % i for i in range(n)], ["dst%d" % i for i in range(n)]
    srcs = [st.put(S[i], src_frame(rng, sw, sh, ch, st.pitch("src", sw * ch), alpha_mix=True)) for i in range(n)]
    wants = [st.put(D[i], noise(rng, dh, st.pitch("dst", dw * ch))) for i in range(n)]
    for i in range(n):
        assert orc.orc_pixbuf_scale(P(srcs[i]), srcs[i].strides[0], sw, sh, P(wants[i]), wants[i].strides[0], dw, dh, ch, interp) == 0
    form = rule_pixbuf(ch, sw, sh, dw, dh, st.bits(*S), st.bits(*D), aligned)
    what = "pixbuf_scale ch=%d %dx%d -> %dx%d interp=%d" % (ch, sw, sh, dw, dh, interp)
    if st.gpu is not None:
        gpu = st.gpu
        st.tune("PBH_ALIGNED", aligned)
        if n > 1:
            if not st.launch(lambda: gpu.pixbuf_scale_batch([st.dev(k) for k in S], [st.dev(k) for k in D], sw, sh, dw, dh, channels=ch, interp=interp)):
                return form
            for i in range(n):
                st.check(D[i], wants[i], dh, what + " batch frame %d" % i)
                st.reupload(D[i])
        for i in range(n):
            if not st.launch(lambda: gpu.pixbuf_scale(st.dev(S[i]), st.dev(D[i]), sw, sh, dw, dh, channels=ch, interp=interp)):
                return form
    for i in range(n):
        st.check(D[i], wants[i], dh, what + " frame %d" % i)
        st.check(S[i], srcs[i], sh, what + " source %d" % i)
    return form


# ============================================================================================== palette.hip
CLAMP_PITCH = {588: 127, 589: 172, 564: 86, 565: 86, 544: 44, 545: 44, 522: 44, 512: 44, 513: 44}       # 6 rows of these are no multiple of 16 bytes, nor are the chroma planes


def run_clamp_switch(orc, st, palette, to_unclamped):
    """k_clamp_switch walks a plane as ONE byte range of height * pitch bytes: 16-byte chunks from the first aligned address, the bytes in front of it (head) and behind
    the last whole chunk (tail) one by one.  The form is the (head, tail) of every plane"""
    h, py = 6, CLAMP_PITCH[palette] + st.place["dp"].get("p", 0)
    st.fams.add("p")
    rng = seeded("clamp", palette, to_unclamped)
    if palette in (588, 589, 564, 565):
        dims = [(h, py)]
    else:
        cs, chh = (py, h) if palette in (544, 545) else (py >> 1, h >> 1 if palette in (512, 513) else h)
        dims = [(h, py), (chh, cs), (chh, cs)] + ([(h, py)] if palette == 545 else [])
    names = ["p%d" % i for i in range(len(dims))]
    planes = [st.put(names[i], rng.integers(0, 256, (r + GUARD, c), dtype=np.uint8)) for i, (r, c) in enumerate(dims)]
    wp, ws = po.planes_args(planes)
    assert orc.orc_switch_yuv_clamping(ctypes.addressof(wp), ctypes.addressof(ws), palette, h, to_unclamped) == 0
    forms = []
    for i, (r, c) in enumerate(dims[:3]):                   # the alpha plane of 545 is left alone
        nbytes = h * py if i == 0 else (h * py) // (1 if palette in (544, 545) else 2 if palette == 522 else 4)
        head = (16 - (st.addr(names[i]) & 15)) & 15
        tail = (nbytes - head) % 16 if nbytes > head else 0
        forms.append("head" if head and tail else "head only" if head else "tail only" if tail else "chunks only")
    if st.gpu is not None:
        st.gpu.yuv_switch_clamping([st.dev(k) for k in names], palette, h, to_unclamped)
    for i, (r, c) in enumerate(dims):
        st.check(names[i], planes[i], r, "switch clamping %d to_unclamped=%d plane %d" % (palette, to_unclamped, i))
    return "k_clamp_switch " + " / ".join(forms)


def rule_rgb_to_yuv(fmt, ips, order, oa, width, sb, d0, d12, d3):
    """rgb_to_yuv_impl_n: the cell kernels (k_rgb_to_yuv420_s, _422_s, _444_s) when every address condition holds, else k_rgb_to_yuv"""
    if fmt in (2, 3) and d0 & 3:
        return BADARG
    if order <= 1 and (width & 3) == 0:
        if fmt == 4 and ips == 4 and (sb & 15) == 0 and (d0 & 3) == 0 and (d12 & 1) == 0:
            return "k_rgb_to_yuv420_s"
        if fmt in (2, 3, 5) and ips == 4 and (sb & 15) == 0 and (((d0 & 3) == 0 and (d12 & 1) == 0) if fmt == 5 else (d0 & 7) == 0):
            return "k_rgb_to_yuv422_s"
        pb = d0 | d12 | (d3 if oa else 0)
        if ((fmt == 0 and (d0 & (15 if oa else 3)) == 0) or (fmt == 1 and (pb & 3) == 0)) and (sb & (15 if ips == 4 else 3)) == 0:
            return "k_rgb_to_yuv444_s"
    return "k_rgb_to_yuv"


def run_rgb_to_yuv(orc, st, order, ia, fmt, n):
    w, h = 40, 6
    rng = seeded("rgb_to_yuv", order, ia, fmt, n)
    ips = 4 if (order == 2 or ia) else 3
    oa = 1 if (fmt <= 1 and ia) else 0
    which = (1 if order == 1 else 0) | (2 if (fmt >= 4 and ia) else 0)
    _, dims = po.k4_out_planes(0, w, h, fmt, oa)
    S = ["src%d" % i for i in range(n)] if n > 1 else ["src"]
    D = [["dst%d_%d" % (i, k) for k in range(len(dims))] for i in range(n)] if n > 1 else [["dst%d" % k for k in range(len(dims))]]
    srcs = [st.put(S[i], src_frame(rng, w, h, ips, st.pitch("src", w * ips))) for i in range(n)]
    wants = [[st.put(D[i][k], noise(rng, b, st.pitch("dst%d" % k, a))) for k, (a, b) in enumerate(dims)] for i in range(n)]
    for i in range(n):
        wp, ws = po.planes_args(wants[i])
        assert orc.orc_rgb_to_yuv(P(srcs[i]), srcs[i].strides[0], w, h, order, ia, ctypes.addressof(wp), ctypes.addressof(ws), fmt, oa, which) == 0
    col = lambda k: st.bits(*[D[i][k] for i in range(n)]) if k < len(dims) else 0
    form = rule_rgb_to_yuv(fmt, ips, order, oa, w, st.bits(*S), col(0), col(1) | col(2), col(3))
    what = "rgb_to_yuv order=%d alpha=%d fmt=%d" % (order, ia, fmt)
    if st.gpu is not None:
        gpu = st.gpu
        if n > 1:
            if not st.launch(lambda: gpu.rgb_to_yuv_batch([st.dev(k) for k in S], [[st.dev(k) for k in D[i]] for i in range(n)], w, h, order, ia, fmt, oa, which)):
                return form
            for i in range(n):
                for k, (a, b) in enumerate(dims):
                    st.check(D[i][k], wants[i][k], b, what + " batch frame %d plane %d" % (i, k))
                    st.reupload(D[i][k])
        for i in range(n):
            if not st.launch(lambda: gpu.rgb_to_yuv(st.dev(S[i]), [st.dev(k) for k in D[i]], w, h, order, ia, fmt, oa, which)):
                return form
    for i in range(n):
        for k, (a, b) in enumerate(dims):
            st.check(D[i][k], wants[i][k], b, what + " frame %d plane %d" % (i, k))
    return form


def rule_yuv_to_rgb(fmt, ia, ops, width, s0, sall, db):
    if fmt >= 2 and s0 & 3:
        return BADARG
    if (width & 3) == 0:
        if fmt >= 2 and ops == 4 and (s0 & 7) == 0 and (db & 15) == 0:
            return "k_uyvy_to_rgb_s"
        if ((fmt == 0 and (s0 & (15 if ia else 3)) == 0) or (fmt == 1 and (sall & 3) == 0)) and (db & (15 if ops == 4 else 3)) == 0:
            return "k_yuv444_to_rgb_s"
    return "k_yuv_to_rgb"


def run_yuv_to_rgb(orc, st, fmt, ia, order, oa, n):
    w, h = 40, 6
    rng = seeded("yuv_to_rgb", fmt, ia, order, oa, n)
    which = (1 if oa else 0) | (2 if (fmt == 0 and ia) else 0)
    dims = [(w * (4 if ia else 3), h)] if fmt == 0 else [(w, h)] * (4 if ia else 3) if fmt == 1 else [(w * 2, h)]
    ops = 4 if (order == 2 or oa) else 3
    S = [["src%d_%d" % (i, k) for k in range(len(dims))] for i in range(n)] if n > 1 else [["src%d" % k for k in range(len(dims))]]
    D = ["dst%d" % i for i in range(n)] if n > 1 else ["dst"]
    planes = [[st.put(S[i][k], rng.integers(0, 256, (b + GUARD, st.pitch("src%d" % k, a)), dtype=np.uint8)) for k, (a, b) in enumerate(dims)] for i in range(n)]
    wants = [st.put(D[i], noise(rng, h, st.pitch("dst", w * ops))) for i in range(n)]
    for i in range(n):
        sp, ss = po.planes_args(planes[i])
        assert orc.orc_yuv_to_rgb(ctypes.addressof(sp), ctypes.addressof(ss), w, h, fmt, ia, P(wants[i]), wants[i].strides[0], order, oa, which) == 0
    form = rule_yuv_to_rgb(fmt, ia, ops, w, st.bits(*[S[i][0] for i in range(n)]), st.bits(*[k for fr in S for k in fr]), st.bits(*D))
    what = "yuv_to_rgb fmt=%d ia=%d order=%d oa=%d" % (fmt, ia, order, oa)
    if st.gpu is not None:
        gpu = st.gpu
        if n > 1:
            tab = (ctypes.c_void_p * (4 * n))()
            for i in range(n):
                for k in range(len(dims)):
                    tab[4 * i + k] = st.dev(S[i][k]).data_ptr()
            irow = (ctypes.c_int * 4)(*([p_.strides[0] for p_ in planes[0]] + [0] * (4 - len(dims))))
            if not st.launch(lambda: gpu.lib.call("lgpu_yuv_to_rgb_batch", tab, irow, w, h, fmt, ia, ptrs([st.dev(k) for k in D]), wants[0].strides[0], order, oa, which, n, None)):
                return form
            for i in range(n):
                st.check(D[i], wants[i], h, what + " batch frame %d" % i)
                st.reupload(D[i])
        for i in range(n):
            if not st.launch(lambda: gpu.yuv_to_rgb([st.dev(k) for k in S[i]], st.dev(D[i]), w, h, fmt, ia, order, oa, which)):
                return form
    for i in range(n):
        st.check(D[i], wants[i], h, what + " frame %d" % i)
    return form



# ============================================================================================== yuv.hip
def rule_yuv420p(opsize, lut16, low_quality, yb, db, nc=2):
    """yuv420p_to_rgb_impl: the paired-table cell form k_yuv420p_to_rgb_s (NC = 2 chroma columns per lane by default) looks at Y and the destination only; U and V
    are never tested"""
    if opsize == 4 and db & 3:
        return BADARG
    if opsize == 4 and not lut16 and not low_quality and (yb & (2 * nc - 1)) == 0 and (db & (7 if nc == 1 else 15)) == 0:
        return "k_yuv420p_to_rgb_s"
    return "k_yuv420p_to_rgb"


def run_yuv420p(orc, st, opsize, is422, use_lut, n, lut16=0):
    w, h = 40, 6
    rng = seeded("yuv420p", opsize, is422, use_lut, n, lut16)
    lut = l2s_lut(orc) if use_lut else None
    l16 = None
    if lut16:
        l16 = np.zeros(65536, np.uint16)
        assert orc.orc_gamma_lut16(1.0, po.GAMMA_LINEAR, po.GAMMA_SRGB, 1.4, P(l16)) == 1
    ch = h if is422 else h // 2
    fr = lambda i, k: "%s%d" % (k, i) if n > 1 else k
    Y = [st.put(fr(i, "y"), rng.integers(0, 256, (h + GUARD, st.pitch("y", w)), dtype=np.uint8)) for i in range(n)]
    # (no guard rows behind the chroma planes: their size is an argument -- the conversion clamps its reads to it -- and the batch form takes it from the tensors)
    U = [st.put(fr(i, "u"), rng.integers(0, 256, (ch, st.pitch("u", w >> 1)), dtype=np.uint8)) for i in range(n)]
    V = [st.put(fr(i, "v"), rng.integers(0, 256, (ch, st.pitch("v", w >> 1)), dtype=np.uint8)) for i in range(n)]
    wants = [st.put(fr(i, "dst"), noise(rng, h, st.pitch("dst", w * opsize))) for i in range(n)]
    strides = (ctypes.c_int * 3)(Y[0].strides[0], U[0].strides[0], V[0].strides[0])
    usz, vsz = ch * U[0].strides[0], ch * V[0].strides[0]
    for i in range(n):
        if lut16:
            assert orc.orc_yuv420p_to_rgb_lut16(P(Y[i]), P(U[i]), P(V[i]), strides, usz, vsz, P(wants[i]), wants[i].strides[0], w, h, opsize, 0, is422, 1, 2, P(l16), 1) == 0
        else:
            orc.orc_yuv420p_to_rgb(P(Y[i]), P(U[i]), P(V[i]), strides, usz, vsz, P(wants[i]), wants[i].strides[0], w, h, opsize, 0, is422, 1, 2, P(lut), 1)
    form = rule_yuv420p(opsize, lut16, 0, st.bits(*[fr(i, "y") for i in range(n)]), st.bits(*[fr(i, "dst") for i in range(n)]))
    what = "yuv42%dp opsize=%d lut=%d lut16=%d" % (2 if is422 else 0, opsize, use_lut, lut16)
    if st.gpu is not None:
        gpu = st.gpu
        dv = lambda i: (st.dev(fr(i, "y")), st.dev(fr(i, "u")), st.dev(fr(i, "v")), st.dev(fr(i, "dst")))
        if n > 1:
            if not st.launch(lambda: gpu.yuv420p_to_rgb_batch([dv(i) for i in range(n)], w, h, opsize=opsize, is_422=is422, which_tables=1, lut=lut, flags=1)):
                return form
            for i in range(n):
                st.check(fr(i, "dst"), wants[i], h, what + " batch frame %d" % i)
                st.reupload(fr(i, "dst"))
        for i in range(n):
            y_, u_, v_, d_ = dv(i)
            if lut16:
                import torch
                ok = st.launch(lambda: gpu.yuv420p_to_rgb_lut16(y_, u_, v_, d_, w, h, torch.from_numpy(l16.view(np.int16)).cuda(), opsize=opsize, is_422=is422, which_tables=1, flags=1))
            else:
                ok = st.launch(lambda: gpu.yuv420p_to_rgb(y_, u_, v_, d_, w, h, opsize=opsize, is_422=is422, which_tables=1, lut=lut, flags=1, u_size=usz, v_size=vsz))
            if not ok:
                return form
    for i in range(n):
        st.check(fr(i, "dst"), wants[i], h, what + " frame %d" % i)
        for k, a, rows in (("y", Y[i], h), ("u", U[i], ch), ("v", V[i], ch)):
            st.check(fr(i, k), a, rows, what + " source")
    return form


# ============================================================================================== lgpu_yuv_repack: the `_s` cell forms
def rule_repack(ip, op, width, sa, ir, da, orw):
    """the guards of the cell forms in lgpu_yuv_repack: sa / da plane addresses, ir / orw plane pitches; everything else is k_yuv_repack"""
    z = lambda v, m: (v & m) == 0
    if 595 in (ip, op):
        return "k_yuv411_repack"             # the 4:1:1 pairs: one byte-wise kernel over compact streams, no address decision
    in444, in420, inpk, outpk = ip in (544, 545), ip in (512, 513), ip in (564, 565), op in (564, 565)
    if (in420 or ip == 522) and outpk:
        if z(width, 7) and z(sa[0] | ir[0], 7) and z(sa[1] | sa[2] | ir[1] | ir[2], 3) and z(da[0] | (orw[0] // 4 * 4), 15):
            return "k_420_to_packed_s"
    elif in444 and op in (588, 589):
        oa = op == 589
        if z(width, 3) and z(ir[0] | ir[1] | ir[2], 3) and ir[0] == ir[1] == ir[2] and z(sa[0] | sa[1] | sa[2], 3) and (not (ip == 545 and oa) or z(sa[3], 3)) and \
                z(da[0] | orw[0], 15 if oa else 3):
            return "k_combine_s"
    elif ip == 588 and op == 544:
        if z(width, 3) and z(sa[0] | ir[0], 3) and z(da[0] | da[1] | da[2] | orw[0] | orw[1] | orw[2], 3):
            return "k_split_s"
    elif inpk and outpk:
        if z(width, 7) and z(sa[0] | ir[0] | da[0] | orw[0], 15):
            return "k_swab_s"
    elif inpk and op in (512, 513, 544, 545, 588, 589):
        if z(width, 7) and z(sa[0] | (ir[0] // 4 * 4), 15):
            if op in (512, 513):
                ok = z(da[0], 7) and z(da[1] | da[2], 3)
            elif op in (544, 545):
                ok = z(da[0] | da[1] | da[2] | orw[0], 7)
            else:
                ok = z(da[0] | orw[0], 15 if op == 589 else 3)
            if ok:
                return "k_pk_to_s"
    elif ip in (588, 589) and (op in (512, 513, 522) or outpk):
        if z(width, 3) and z(sa[0] | ir[0], 15 if ip == 589 else 3):
            if (z(da[0], 3) and z(da[1] | da[2], 1)) if not outpk else z(da[0], 7):
                return "k_888_to_s"
    elif in420 and op == 522:
        if z(width, 7) and z(sa[0] | ir[0] | da[0] | orw[0], 7) and z(sa[1] | sa[2] | ir[1] | ir[2] | da[1] | da[2] | orw[1] | orw[2], 3):
            return "k_420_to_422p_s"
    return "k_yuv_repack"


def run_repack(orc, st, ip, op, w, padok):
    h = 6
    rng = seeded("repack", ip, op, w)
    sd, dd = po.YUV_PLANE_DIMS[ip](w, h), po.YUV_PLANE_DIMS[op](w, h)
    S, D = ["s%d" % k for k in range(len(sd))], ["d%d" % k for k in range(len(dd))]
    for k in S + D:
        st.fams.add(k)
    pitch = (lambda fam, nb: st.pitch(fam, nb)) if padok else (lambda fam, nb: nb)         # the pairs whose reference walks compact buffers keep compact rows
    src = [st.put(S[k], rng.integers(0, 256, (rows + GUARD, pitch(S[k], nb)), dtype=np.uint8)) for k, (nb, rows) in enumerate(sd)]
    want = [st.put(D[k], noise(rng, rows, pitch(D[k], nb))) for k, (nb, rows) in enumerate(dd)]
    sp, ss = po.planes_args(src)
    wp, ws = po.planes_args(want)
    assert orc.orc_yuv_repack(ip, op, ctypes.addressof(sp), ctypes.addressof(ss), ctypes.addressof(wp), ctypes.addressof(ws), w, h, 0, 0) == 0
    form = rule_repack(ip, op, w, [st.addr(k) for k in S], [a.strides[0] for a in src], [st.addr(k) for k in D], [a.strides[0] for a in want])
    if st.gpu is not None:
        st.gpu.yuv_repack(ip, op, [st.dev(k) for k in S], [st.dev(k) for k in D], w, h, 0)
    for k, (nb, rows) in enumerate(dd):
        st.check(D[k], want[k], rows, "repack %d -> %d width %d plane %d" % (ip, op, w, k))
    for k, (nb, rows) in enumerate(sd):
        st.check(S[k], src[k], rows, "repack %d -> %d width %d source plane %d" % (ip, op, w, k))
    return form


# ============================================================================================== two frames in, one out: transitions, fused blur + key, lgpu_fx_batch
FX = {"softlight": 1, "transition": 2, "yuv411_to_rgb": 3, "gauss5_colorkey": 4, "chroma": 5, "luma": 6, "multi": 7}          # LGPU_FX_* of include/lives_gpu.h


def rule_two(name, ps, bits):
    if name == "gauss5_colorkey":           # the fused kernel takes aligned frames only; the caller runs lgpu_gauss5 + lgpu_colorkey otherwise
        return UNSUPPORTED if bits & (15 if ps == 4 else 3) else "k_gauss5_colorkey<%d>" % ps
    if name in ("chroma", "luma", "multi"):
        return rule_pixel2(ps, bits)
    return {"transition": "k_transition<%d>", "slide_over": "k_slide_over<%d>", "dissolve": "k_dissolve<%d>", "triple_split": "k_triple_split"}[name].replace("%d", str(ps))


def run_two(orc, st, name, ps, prm, n, batch):
    """src1, src2 -> dst: lgpu_transition (prm: kind), lgpu_slide_over (direction), lgpu_dissolve, lgpu_triple_split (rows), lgpu_gauss5_colorkey, and -- batch -- the same
    operations and the three blends through lgpu_fx_batch with a frame table; n frames, each against the oracle and the single-frame entry point"""
    w, h = 40, 6
    rng = seeded("two", name, ps, prm, n, batch)
    A, B, D = ["a%d" % i for i in range(n)], ["b%d" % i for i in range(n)], ["dst%d" % i for i in range(n)]
    s1 = [st.put(A[i], src_frame(rng, w, h, ps, st.pitch("a", w * ps), alpha_mix=True)) for i in range(n)]
    s2 = [st.put(B[i], src_frame(rng, w, h, ps, st.pitch("b", w * ps), alpha_mix=True)) for i in range(n)]
    wants = [st.put(D[i], noise(rng, h, st.pitch("dst", w * ps))) for i in range(n)]
    r1, r2, ro = s1[0].strides[0], s2[0].strides[0], wants[0].strides[0]
    amt, bc, col = 0.37, np.array([13, 250, 77], np.int32), (128, 120, 135)
    mask = np.zeros(w * h, np.float32)
    if name == "dissolve":
        orc.orc_dissolve_mask(0xC0FFEE, w, h, mask.ctypes.data)
    form = rule_two(name, ps, st.bits(*(A + B + D)))
    for i in range(n):
        a, b, out = P(s1[i]), P(s2[i]), P(wants[i])
        if form in (UNSUPPORTED, BADARG):
            break
        if name == "transition":
            orc.orc_transition(prm, a, r1, b, r2, out, ro, w, h, ps, amt)
        elif name == "slide_over":
            orc.orc_slide_over(a, r1, b, r2, out, ro, w, h, ps, 77, prm, 1, 0)
        elif name == "dissolve":
            orc.orc_dissolve(a, r1, b, r2, out, ro, w, h, ps, mask.ctypes.data, amt)
        elif name == "triple_split":
            orc.orc_triple_split(a, r1, b, r2, out, ro, w, h, 0, 0.4, 1, 0.0, prm, 0.07, bc.ctypes.data)
        elif name == "gauss5_colorkey":
            bl = np.zeros_like(s1[i])
            orc.orc_gauss5(a, r1, P(bl), r1, w, h, ps)
            (orc.orc_colorkey if ps == 3 else orc.orc_colorkey4)(P(bl), r1, b, r2, out, ro, w, h, 1, 0.4, 0.7, *(col + ((0,) if ps == 3 else ())))
        elif name == "chroma":
            orc.orc_blend_chroma(a, r1, b, r2, out, ro, w, h, ps, 0, 100)
        elif name == "luma":
            orc.orc_blend_luma(prm, a, r1, b, r2, out, ro, w, h, ps, 0, 100, 0)
        else:
            orc.orc_blend_multi(prm, a, r1, b, r2, out, ro, w, h, 0, 100)
    what = "%s ps=%d %s" % (name, ps, prm)

    def single(i):
        gpu, d1, d2, dd = st.gpu, st.dev(A[i]), st.dev(B[i]), st.dev(D[i])
        if name == "transition":
            gpu.transition(prm, d1, d2, dd, w, h, ps, amt)
        elif name == "slide_over":
            gpu.slide_over(d1, d2, dd, w, h, ps, 77, prm, 1, 0)
        elif name == "dissolve":
            import torch
            gpu.dissolve(d1, d2, dd, w, h, ps, torch.from_numpy(mask).cuda(), amt)
        elif name == "triple_split":
            gpu.triple_split(d1, d2, dd, w, h, 0, 0.4, 1, 0.0, prm, 0.07, bc)
        elif name == "gauss5_colorkey":
            gpu.gauss5_colorkey(d1, d2, dd, w, h, ps, 1, 0.4, 0.7, col)
        elif name == "chroma":
            gpu.blend_chroma(d1, d2, dd, w, h, ps, 100)
        elif name == "luma":
            gpu.blend_luma(prm, d1, d2, dd, w, h, ps, 0, 100)
        else:
            gpu.blend_multi(prm, d1, d2, dd, w, h, 0, 100)

    if st.gpu is not None:
        gpu = st.gpu
        if batch:
            ip, dp = {"transition": ((prm, ps), (amt,)), "gauss5_colorkey": ((ps, 1, col[0] | (col[1] << 8) | (col[2] << 16)), (0.4, 0.7)), "chroma": ((ps, 0), (100.,)),
                      "luma": ((prm, ps, 0), (100.,)), "multi": ((prm, 0), (100.,))}[name]
            if not st.launch(lambda: gpu.fx_batch(FX[name], [[st.dev(k)] for k in A], [[st.dev(k)] for k in D], w, h, ins1=[[st.dev(k)] for k in B], ip=ip, dp=dp)):
                return form
            for i in range(n):
                st.check(D[i], wants[i], h, what + " fx_batch frame %d" % i)
                st.reupload(D[i])
        for i in range(n):
            if not st.launch(lambda: single(i)):
                return form
    for i in range(n):
        st.check(D[i], wants[i], h, what + " frame %d" % i)
    return form


def rule_softlight(width, bits):
    return "k_softlight_s" if (width & 3) == 0 and width >= 8 and (bits & 3) == 0 else "k_softlight"


def run_softlight(orc, st, palette, w, n):
    """lgpu_softlight and lgpu_fx_batch(LGPU_FX_SOFTLIGHT): the luma plane against the oracle, the other planes copied (by extra blocks of the same launch, whose row copy
    looks at its own addresses)"""
    h = 6
    rng = seeded("softlight", palette, w, n)
    cw, chh = (w >> 1 if palette in (512, 513, 522) else w), (h >> 1 if palette in (512, 513) else h)
    dims = [(w, h), (cw, chh), (cw, chh)] + ([(w, h)] if palette == 545 else [])
    fr = lambda i, k: "%s%d" % (k, i) if n > 1 else k
    S = [["%s_%d" % (fr(i, "s"), k) for k in range(len(dims))] for i in range(n)]
    D = [["%s_%d" % (fr(i, "d"), k) for k in range(len(dims))] for i in range(n)]
    src = [[st.put(S[i][k], rng.integers(0, 256, (b + GUARD, st.pitch("s_%d" % k, a)), dtype=np.uint8)) for k, (a, b) in enumerate(dims)] for i in range(n)]
    want = [[st.put(D[i][k], noise(rng, b, st.pitch("d_%d" % k, a))) for k, (a, b) in enumerate(dims)] for i in range(n)]
    for i in range(n):
        orc.orc_softlight_y(P(src[i][0]), src[i][0].strides[0], P(want[i][0]), want[i][0].strides[0], w, h, 0)
        for k, (a, b) in enumerate(dims[1:], 1):
            want[i][k][:b, :a] = src[i][k][:b, :a]
    form = rule_softlight(w, st.bits(*([S[i][0] for i in range(n)] + [D[i][0] for i in range(n)])))
    what = "softlight %d width %d" % (palette, w)
    if st.gpu is not None:
        gpu = st.gpu
        if n > 1:
            gpu.fx_batch(FX["softlight"], [[st.dev(k) for k in S[i]] for i in range(n)], [[st.dev(k) for k in D[i]] for i in range(n)], w, h, palette=palette, ip=(0,))
            for i in range(n):
                for k, (a, b) in enumerate(dims):
                    st.check(D[i][k], want[i][k], b, what + " fx_batch frame %d plane %d" % (i, k))
                    st.reupload(D[i][k])
        for i in range(n):
            gpu.softlight([st.dev(k) for k in S[i]], [st.dev(k) for k in D[i]], w, h, palette, 0)
    for i in range(n):
        for k, (a, b) in enumerate(dims):
            st.check(D[i][k], want[i][k], b, what + " frame %d plane %d" % (i, k))
    return form


def run_yuv411_to_rgb(orc, st, order, oa, n):
    wm, h = 10, 6
    ps = 4 if (order == 2 or oa) else 3
    rng = seeded("yuv411_to_rgb", order, oa, n)
    S, D = ["src%d" % i for i in range(n)], ["dst%d" % i for i in range(n)]
    st.fams.add("src")
    srcs = [st.put(S[i], rng.integers(0, 256, (h + GUARD, wm * 6), dtype=np.uint8)) for i in range(n)]         # compact rows: the reference walks the 4:1:1 side as one stream
    wants = [st.put(D[i], noise(rng, h, st.pitch("dst", wm * 4 * ps))) for i in range(n)]
    for i in range(n):
        assert orc.orc_yuv411_to_rgb(P(srcs[i]), wm, h, P(wants[i]), wants[i].strides[0], order, oa, 0) == 0
    what = "yuv411_to_rgb order=%d alpha=%d" % (order, oa)
    if st.gpu is not None:
        gpu = st.gpu
        if n > 1:
            gpu.fx_batch(FX["yuv411_to_rgb"], [[st.dev(k)] for k in S], [[st.dev(k)] for k in D], wm, h, ip=(order, oa, 0))
            for i in range(n):
                st.check(D[i], wants[i], h, what + " fx_batch frame %d" % i)
                st.reupload(D[i])
        for i in range(n):
            gpu.yuv411_to_rgb(st.dev(S[i]), st.dev(D[i]), wm, h, out_order=order, out_alpha=oa, unclamped=0)
    for i in range(n):
        st.check(D[i], wants[i], h, what + " frame %d" % i)
    return "k_yuv411_to_rgb"                 # one kernel; it stores a macropixel as dwords where the address allows (palette.hip, in the kernel)


def run_rgb_to_yuv411(orc, st, order, ia):
    w, h = 40, 6
    ips = 4 if ia else 3
    rng = seeded("rgb_to_yuv411", order, ia)
    src = st.put("src", src_frame(rng, w, h, ips, st.pitch("src", w * ips)))
    st.fams.add("dst")
    want = st.put("dst", noise(rng, h, (w >> 2) * 6))
    assert orc.orc_rgb_to_yuv411(P(src), src.strides[0], w, h, order, ia, P(want), 0) == 0
    if st.gpu is not None:
        st.gpu.rgb_to_yuv411(st.dev("src"), st.dev("dst"), w, h, in_order=order, in_alpha=ia, unclamped=0)
    st.check("dst", want, h, "rgb_to_yuv411 order=%d alpha=%d" % (order, ia))
    return "k_rgb_to_yuv411"


# ============================================================================================== stencil.hip
def rule_deinterlace(palette, width, inplace, bits):
    ps4 = palette in (3, 4, 589, 5)
    return "k_deinterlace dword" if ps4 and width % 3 == 0 and (bits & 3) == 0 else "k_deinterlace bytes"


def run_deinterlace(orc, st, palette, w, inplace):
    h = 8
    ps = 3 if palette in (1, 2, 588) else 4
    rng = seeded("deinterlace", palette, w, inplace)
    s1 = src_frame(rng, w, h, ps, st.pitch("src", w * ps))
    s1[1:h:2] = (s1[1:h:2] >> 2) + 160                     # comb rows, so that both branches of the decision occur
    s1[0:h:2] = (s1[0:h:2] >> 2) + (rng.integers(0, 2, (s1[0:h:2].shape[0], 1), dtype=np.uint8) * 120)
    st.put("src", s1)
    want = s1 if inplace else st.put("dst", noise(rng, h, st.pitch("dst", w * ps)))
    assert orc.orc_deinterlace(P(s1), s1.strides[0], P(want), want.strides[0], w, h, palette) == 0
    # in place the kernel reads a 256-aligned snapshot: only the frame's own address and pitch count
    form = rule_deinterlace(palette, w, inplace, (st.addr("src") | s1.strides[0]) if inplace else st.bits("src", "dst"))
    if st.gpu is not None:
        st.gpu.deinterlace(st.dev("src"), st.dev("src" if inplace else "dst"), w, h, palette)
    st.check("src" if inplace else "dst", want, h, "deinterlace pal=%d width %d inplace=%d" % (palette, w, inplace))
    return form


def rule_edge(ps, width, bits):
    if ps == 4 and (width & 3) == 0 and width >= 8 and (bits & 15) == 0:
        return "k_edge_map4 + k_edge_paint4"
    return "k_edge_map<4> + k_edge_paint<4> dword" if ps == 4 and (bits & 3) == 0 else "k_edge_map<%d> + k_edge_paint<%d>" % (ps, ps)


def run_edge(orc, st, palette, mode, inplace):
    w, h = 40, 12
    ps = 3 if palette <= 2 else 4
    rng = seeded("edge", palette, mode, inplace)
    s = src_frame(rng, w, h, ps, st.pitch("src", w * ps))
    yy, xx = np.mgrid[0:h, 0:w]                              # smooth structure under the noise so that the histogram is not flat
    for c in range(ps):
        s[:h, c:w * ps:ps] = ((s[:h, c:w * ps:ps] >> 3) + (96 * ((xx // 9 + yy // 7 + c) % 2)).astype(np.uint8) + 40).astype(np.uint8)
    st.put("src", s)
    want = s if inplace else st.put("dst", noise(rng, h, st.pitch("dst", w * ps)))
    m16 = np.zeros(w * h, np.int16)
    orc.orc_edge(P(s), s.strides[0], P(want), want.strides[0], w, h, palette, mode, P(m16), inplace)
    form = rule_edge(ps, w, st.bits("src") if inplace else st.bits("src", "dst"))
    if st.gpu is not None:
        st.gpu.edge(st.dev("src"), st.dev("src" if inplace else "dst"), w, h, palette, mode)
    st.check("src" if inplace else "dst", want, h, "edge pal=%d mode=%d inplace=%d" % (palette, mode, inplace))
    return form


def run_composite(orc, st, ps, is_bgr, revz):
    """lgpu_composite: layers painted at odd pixel offsets; the kernel loads a layer pixel and stores a canvas pixel as one dword where address and pitch allow"""
    ow, oh = 40, 12
    rng = seeded("composite", ps, is_bgr, revz)
    geo = [(12, 8, -3, -2, 0.7312), (15, 6, 9, 7, 1.0), (8, 4, 5, 3, 0.5), (25, 14, 21, -1, 0.25)]
    layers = [(st.put("l%d" % z, src_frame(rng, w, h, ps, st.pitch("l%d" % z, w * ps))), w, h, ox, oy, al) for z, (w, h, ox, oy, al) in enumerate(geo)]
    bg = [int(v) for v in rng.integers(0, 256, 3)]
    L = (po.CompLayer * len(layers))()
    for z, (a, w, h, ox, oy, al) in enumerate(layers):
        L[z].src, L[z].irow = a.ctypes.data, a.strides[0]
        L[z].width, L[z].height, L[z].offs_x, L[z].offs_y, L[z].alpha = w, h, ox, oy, al
    want = st.put("dst", noise(rng, oh, st.pitch("dst", ow * ps)))
    orc.orc_composite(P(want), want.strides[0], ow, oh, ps, is_bgr, (ctypes.c_int * 3)(*bg), L, len(layers), revz)
    if st.gpu is not None:
        st.gpu.composite(st.dev("dst"), ow, oh, ps, [(st.dev("l%d" % z), w, h, ox, oy, al) for z, (a, w, h, ox, oy, al) in enumerate(layers)], bgcol=bg, is_bgr=is_bgr, revz=revz)
    st.check("dst", want, oh, "composite ps=%d bgr=%d revz=%d" % (ps, is_bgr, revz))
    return "k_composite<%d>" % ps


PIXBUF, OPAQUE, NOBLEND = 0x100, 0x200, 0x400


def rule_chain_pb(sw, sh, dw, dh, sb, l2b, db):
    """lgpu_chain / lgpu_chain_amounts with LGPU_INTERP_PIXBUF: pb_chain_half (one launch of k_pb_half behind the table check of pb_half_ok) or the stages one by one"""
    if (sb | l2b | db) & 3:
        return BADARG
    if sw == 2 * dw and sh == 2 * dh and (sw & 3) == 0 and (sb & 15) == 0 and ((db | l2b) & 7) == 0:
        return "k_pb_half chain"
    return "staged"


def run_chain_pb(orc, st, sw, sh, dw, dh, blur, flag, amounts):
    """three tracks on the gdk-pixbuf arithmetic, a blend amount per track (lgpu_chain_amounts) or one for all (lgpu_chain)"""
    ntr = 3
    rng = seeded("chain_pb", sw, sh, dw, dh, blur, flag, amounts)
    lut = l2s_lut(orc)
    am = [0, 255, 117] if amounts else [99] * ntr
    S, L, D = ["src%d" % i for i in range(ntr)], ["l2%d" % i for i in range(ntr)], ["dst%d" % i for i in range(ntr)]
    srcs = []
    for i in range(ntr):
        a = src_frame(rng, sw, sh, 4, st.pitch("src", sw * 4), alpha_mix=True)
        if flag & OPAQUE:
            a[:, 3::4] = 255
        srcs.append(st.put(S[i], a))
    noblend = bool(flag & NOBLEND)          # no layer 2 at all: the tracks carry a null pointer, and no address or pitch of a layer 2 enters any check
    l2s = [None] * ntr if noblend else [st.put(L[i], src_frame(rng, dw, dh, 4, st.pitch("l2", dw * 4), alpha_mix=True)) for i in range(ntr)]
    wants = [st.put(D[i], noise(rng, dh, st.pitch("dst", dw * 4))) for i in range(ntr)]
    irow, orow = srcs[0].strides[0], wants[0].strides[0]
    irow2 = orow if noblend else l2s[0].strides[0]
    for i in range(ntr):
        if noblend:
            from tests import chain_ref
            wants[i][:dh, :dw * 4] = chain_ref.oracle_chain_rgba(orc, srcs[i], sw, sh, dw, dh, 3, 1, None, 0, lut, blur=bool(blur))
        else:
            assert orc.orc_chain(P(srcs[i]), irow, sw, sh, P(l2s[i]), irow2, P(wants[i]), orow, dw, dh, 1, 3 | PIXBUF, blur, am[i], P(lut)) == 0
    form = rule_chain_pb(sw, sh, dw, dh, st.bits(*S), 0 if noblend else st.bits(*L), st.bits(*D))
    if st.gpu is not None:
        gpu = st.gpu
        prm = gpu.chain_params(sw, sh, irow, dw, dh, irow2, orow, swap_rb=1, interp=3 | PIXBUF | flag, do_blur=blur, bf=99, lut=lut)
        trk = lambda: gpu.chain_tracks([st.dev(k) for k in S], None if noblend else [st.dev(k) for k in L], [st.dev(k) for k in D])
        if not st.launch((lambda: gpu.chain_amounts(prm, trk(), None if noblend else am)) if amounts else (lambda: gpu.chain(prm, trk()))):
            return form
    for i in range(ntr):
        st.check(D[i], wants[i], dh, "pixbuf chain %dx%d -> %dx%d blur=%d flag=%#x amounts=%d track %d" % (sw, sh, dw, dh, blur, flag, amounts, i))
    return form


def run_premult_yuva(orc, st, palette, clamped, un):
    w, h = 40, 6
    rng = seeded("premult_yuva", palette, clamped, un)
    if palette == 589:
        names, planes = ["p0"], [st.put("p0", src_frame(rng, w, h, 4, st.pitch("p0", w * 4)))]
    else:
        names = ["p%d" % k for k in range(4)]
        planes = [st.put(names[k], src_frame(rng, w, h, 1, st.pitch(names[k], w))) for k in range(4)]
    pp = (ctypes.c_void_p * 4)(*([x.ctypes.data for x in planes] + [None] * (4 - len(planes))))
    ss = (ctypes.c_int * 4)(*([x.strides[0] for x in planes] + [0] * (4 - len(planes))))
    orc.orc_alpha_premult_yuva(pp, ss, w, h, palette, clamped, un)
    b = st.bits("p0")
    form = "k_premult_yuva<1>" if (palette == 589 and clamped and (b & 15) == 0) else "k_premult_yuva<0> dword" if (palette == 589 and (b & 3) == 0) else "k_premult_yuva<0>"
    if st.gpu is not None:
        st.gpu.alpha_premult_yuva([st.dev(k) for k in names], w, h, palette, clamped, un=un)
    for k in range(len(planes)):
        st.check(names[k], planes[k], h, "premult yuva %d clamped=%d un=%d plane %d" % (palette, clamped, un, k))
    return form


def run_rgb_to_yuv_lut16(orc, st, order, ia, fmt):
    w, h = 40, 6
    ips = 4 if ia else 3
    rng = seeded("rgb_to_yuv_lut16", order, ia, fmt)
    l16 = np.zeros(65536, np.uint16)
    assert orc.orc_gamma_lut16(1.0, po.GAMMA_SRGB, po.GAMMA_LINEAR, 1.4, P(l16)) == 1
    src = st.put("src", src_frame(rng, w, h, ips, st.pitch("src", w * ips)))
    want = st.put("dst", noise(rng, h, st.pitch("dst", w * 2)))
    assert orc.orc_rgb_to_yuv_lut16(P(src), src.strides[0], w, h, order, ia, P(want), want.strides[0], fmt, 0, P(l16)) == 0
    form = BADARG if st.bits("dst") & 3 else "k_rgb_to_yuv"            # the cell form takes no gamma LUT
    if st.gpu is not None:
        import torch
        if not st.launch(lambda: st.gpu.rgb_to_yuv_lut16(st.dev("src"), st.dev("dst"), w, h, order, ia, fmt, 0, torch.from_numpy(l16.view(np.int16)).cuda())):
            return form
    st.check("dst", want, h, "rgb_to_yuv_lut16 order=%d alpha=%d fmt=%d" % (order, ia, fmt))
    return form


def run_fill_pattern(orc, st, plen):
    n, rows = 37, 6
    rng = seeded("fill_pattern", plen)
    pat = rng.integers(0, 256, plen, dtype=np.uint8)
    before = st.put("dst", noise(rng, rows, st.pitch("dst", n * plen)))
    want = before.copy()
    want[:rows, :n * plen] = np.tile(pat, n)
    if st.gpu is not None:
        d = st.dev("dst")
        st.gpu.lib.call("lgpu_fill_pattern", d.data_ptr(), d.stride(0), pat.ctypes.data, plen, n, rows, None)
    st.check("dst", want, rows, "fill_pattern plen=%d" % plen)
    return "k_fill_pattern"


def run_chain_canvas(orc, st, blur, noblend):
    """lgpu_chain_amounts onto a letterbox canvas (72 x 12, the 64 x 8 frame at the even column 4, row 2): 8-byte stores into canvas + offs_y * pitch + offs_x * 4, so
    the destination's own base residue decides with the (even) offset"""
    from tests import chain_ref
    sw, sh, dw, dh, canvas, ntr = 128, 16, 64, 8, (72, 12, 4, 2), 3
    cw, ch = canvas[:2]
    rng = seeded("chain_canvas", blur, noblend)
    lut, am = l2s_lut(orc), [0, 255, 117]
    S, L, D = ["src%d" % i for i in range(ntr)], ["l2%d" % i for i in range(ntr)], ["dst%d" % i for i in range(ntr)]
    srcs = [st.put(S[i], src_frame(rng, sw, sh, 4, st.pitch("src", sw * 4), alpha_mix=True)) for i in range(ntr)]
    l2s = [None] * ntr if noblend else [st.put(L[i], src_frame(rng, cw, ch, 4, st.pitch("l2", cw * 4), alpha_mix=True)) for i in range(ntr)]
    wants = [st.put(D[i], noise(rng, ch, st.pitch("dst", cw * 4))) for i in range(ntr)]
    irow, orow = srcs[0].strides[0], wants[0].strides[0]
    irow2 = orow if noblend else l2s[0].strides[0]
    for i in range(ntr):
        wants[i][:ch, :cw * 4] = chain_ref.oracle_chain_rgba(orc, srcs[i], sw, sh, dw, dh, 3, 1, l2s[i], am[i], lut, canvas=canvas, blur=bool(blur))
    form = rule_chain_pb(sw, sh, dw, dh, st.bits(*S), 0 if noblend else st.bits(*L), st.bits(*D))
    if st.gpu is not None:
        gpu = st.gpu
        prm = gpu.chain_params(sw, sh, irow, dw, dh, irow2, orow, swap_rb=1, interp=3 | PIXBUF | (NOBLEND if noblend else 0), do_blur=blur, bf=99, lut=lut)
        trk = lambda: gpu.chain_tracks([st.dev(k) for k in S], None if noblend else [st.dev(k) for k in L], [st.dev(k) for k in D])
        if not st.launch(lambda: gpu.chain_amounts(prm, trk(), None if noblend else am, canvas)):
            return form
    for i in range(ntr):
        st.check(D[i], wants[i], ch, "chain onto a canvas blur=%d noblend=%d track %d" % (blur, noblend, i))
    return form


def rule_chain_yuv(l2b, db):
    """lgpu_chain_yuv420p: destination and layer 2 4-aligned or refused; one launch when their rows are 8-aligned, LGPU_E_UNSUPPORTED otherwise; Y, U, V at any address"""
    return BADARG if (l2b | db) & 3 else UNSUPPORTED if (l2b | db) & 7 else "k_pb_half<YUV>"


def run_chain_yuv(orc, st, tight, canvas):
    from tests import chain_ref
    sw, sh, ntr = 128, 16, 3
    dw, dh = sw // 2, sh // 2
    cw, ch = canvas[:2] if canvas else (dw, dh)
    rng = seeded("chain_yuv", tight, canvas)
    lut, am = l2s_lut(orc), [0, 255, 117]
    Yn, Un, Vn = ["y%d" % i for i in range(ntr)], ["u%d" % i for i in range(ntr)], ["v%d" % i for i in range(ntr)]
    L, D = ["l2%d" % i for i in range(ntr)], ["dst%d" % i for i in range(ntr)]
    pad = (st.place["dp"].get("y", 0) + 16, st.place["dp"].get("u", 0) + 8, st.place["dp"].get("v", 0) + 8)
    st.fams |= {"y", "u", "v"}
    src = [chain_ref.planes(rng, sw, sh, pad, tight) for _ in range(ntr)]
    strides = src[0][3]
    for i in range(ntr):
        st.put(Yn[i], src[i][0])
        st.put(Un[i], src[i][1].reshape(1, -1))          # the chroma planes travel as one row: a tight plane ends with its last sample
        st.put(Vn[i], src[i][2].reshape(1, -1))
    l2s = [st.put(L[i], src_frame(rng, cw, ch, 4, st.pitch("l2", cw * 4), alpha_mix=True)) for i in range(ntr)]
    wants = [st.put(D[i], noise(rng, ch, st.pitch("dst", cw * 4))) for i in range(ntr)]
    irow2, orow = l2s[0].strides[0], wants[0].strides[0]
    form = rule_chain_yuv(st.bits(*L), st.bits(*D))
    for i in range(ntr):
        Y, U, V, _ = src[i]
        wants[i][:ch, :cw * 4] = chain_ref.oracle_chain(orc, Y, U, V, strides, sw, sh, 3, 0, 1, 2, 1, l2s[i][:ch], am[i], lut, canvas)
    if st.gpu is not None:
        gpu = st.gpu
        prm = gpu.chain_params(sw, sh, sw * 4, dw, dh, irow2, orow, swap_rb=0, interp=3 | PIXBUF, do_blur=0, bf=99, lut=lut)
        ysrc = gpu.yuv_source(strides, src[0][1].size, src[0][2].size, out_order=0, which_tables=1, pb_quality=2, flags=1)
        trk = lambda: gpu.chain_yuv_tracks([st.dev(k) for k in Yn], [st.dev(k) for k in Un], [st.dev(k) for k in Vn], [st.dev(k) for k in L], [st.dev(k) for k in D])
        if not st.launch(lambda: gpu.chain_yuv420p(prm, ysrc, trk(), am, canvas)):
            return form
    for i in range(ntr):
        st.check(D[i], wants[i], ch, "chain from 4:2:0 planes tight=%d canvas=%s track %d" % (tight, canvas, i))
    return form


def rule_chain_sink(yuvsrc, sb, l2b, planes, pitches):
    """lgpu_chain_to_yuv / lgpu_chain_yuv420p_to_yuv: one launch or nothing.  planes: OR of the sink planes' addresses; pitches: the sink's rowstrides"""
    if (l2b & 3) or (not yuvsrc and sb & 3):
        return BADARG
    if (not yuvsrc and sb & 15) or (l2b & 7) or (planes & 15) or (pitches[0] & 7) or (len(pitches) > 1 and (pitches[1] | pitches[2]) & 3):
        return UNSUPPORTED
    return "k_pb_half<YUV, SINK>" if yuvsrc else "k_pb_half<SINK>"


def run_chain_sink(orc, st, fmt, yuvsrc):
    """the chain ending at a YUV sink (UYVY 2, YUYV 3, 4:2:0 planar 4), from RGBA frames or from 4:2:0 planes: three tracks, a blend amount each"""
    from tests import chain_ref
    sw, sh, ntr = 128, 16, 3
    dw, dh = sw // 2, sh // 2
    rng = seeded("chain_sink", fmt, yuvsrc)
    lut, am = l2s_lut(orc), [0, 255, 117]
    dims = [(dw * 2, dh)] if fmt in (2, 3) else [(dw, dh), (dw >> 1, dh >> 1), (dw >> 1, dh >> 1)]
    L = ["l2%d" % i for i in range(ntr)]
    D = [["sink%d_%d" % (i, k) for k in range(len(dims))] for i in range(ntr)]
    if yuvsrc:
        st.fams |= {"y", "u", "v"}
        pad = (st.place["dp"].get("y", 0) + 16, st.place["dp"].get("u", 0) + 8, st.place["dp"].get("v", 0) + 8)
        src = [chain_ref.planes(rng, sw, sh, pad, 1) for _ in range(ntr)]
        S = [["y%d" % i, "u%d" % i, "v%d" % i] for i in range(ntr)]
        for i in range(ntr):
            st.put(S[i][0], src[i][0])
            st.put(S[i][1], src[i][1].reshape(1, -1))
            st.put(S[i][2], src[i][2].reshape(1, -1))
        sb = 0
    else:
        S = [["src%d" % i] for i in range(ntr)]
        src = [st.put(S[i][0], src_frame(rng, sw, sh, 4, st.pitch("src", sw * 4), alpha_mix=True)) for i in range(ntr)]
        sb = st.bits(*[s[0] for s in S])
    l2s = [st.put(L[i], src_frame(rng, dw, dh, 4, st.pitch("l2", dw * 4), alpha_mix=True)) for i in range(ntr)]
    wants = [[st.put(D[i][k], noise(rng, r, st.pitch("sink_%d" % k, b))) for k, (b, r) in enumerate(dims)] for i in range(ntr)]
    pitches = [a.strides[0] for a in wants[0]]
    planes = 0
    for i in range(ntr):
        for k in D[i]:
            planes |= st.addr(k)
    form = rule_chain_sink(yuvsrc, sb, st.bits(*L), planes, pitches)
    for i in range(ntr):
        if yuvsrc:
            Y, U, V, strides = src[i]
            rgba = chain_ref.oracle_chain(orc, Y, U, V, strides, sw, sh, 3, 0, 1, 2, 1, l2s[i][:dh], am[i], lut, None)
        else:
            rgba = chain_ref.oracle_chain_rgba(orc, src[i], sw, sh, dw, dh, 3, 0, l2s[i][:dh], am[i], lut)
        compact, _ = po.k4_out_planes(0, dw, dh, fmt, 0)
        wp, ws = po.planes_args(compact)
        assert orc.orc_rgb_to_yuv(P(rgba), rgba.strides[0], dw, dh, 0, 1, ctypes.addressof(wp), ctypes.addressof(ws), fmt, 0, 1) == 0
        for k, (b, r) in enumerate(dims):
            wants[i][k][:r, :b] = compact[k]
    if st.gpu is not None:
        gpu = st.gpu
        prm = gpu.chain_params(sw, sh, sw * 4 if yuvsrc else src[0].strides[0], dw, dh, l2s[0].strides[0], 0, swap_rb=0, interp=3 | PIXBUF, bf=0, lut=lut)
        sink = gpu.chain_sink(fmt, pitches, which_tables=1, in_order=0)
        dpl = lambda: [[st.dev(k) for k in D[i]] for i in range(ntr)]
        if yuvsrc:
            ysrc = gpu.yuv_source(src[0][3], src[0][1].size, src[0][2].size, out_order=0, which_tables=1, pb_quality=2, flags=1)
            call = lambda: gpu.chain_yuv420p_to_yuv(prm, ysrc, sink, gpu.chain_yuv_sink_tracks([st.dev(s[0]) for s in S], [st.dev(s[1]) for s in S], [st.dev(s[2]) for s in S],
                                                                                                [st.dev(k) for k in L], dpl()), am)
        else:
            call = lambda: gpu.chain_to_yuv(prm, sink, gpu.chain_sink_tracks([st.dev(s[0]) for s in S], [st.dev(k) for k in L], dpl()), am)
        if not st.launch(call):
            return form
    for i in range(ntr):
        for k, (b, r) in enumerate(dims):
            st.check(D[i][k], wants[i][k], r, "chain to sink fmt=%d yuvsrc=%d track %d plane %d" % (fmt, yuvsrc, i, k))
    return form


def run_rgbdelay(orc, st, palette, w, inplace):
    """lgpu_rgbdelay_process, two consecutive frames through one ring (the second one accumulates the first from the ring): k_rgbdelay4 moves 12 bytes per lane when
    3 * width, the destination pitch and the destination address are multiples of 4, k_rgbdelay 3 bytes per lane otherwise; both zero the row padding as the reference does"""
    from tests import golden_util as gu
    h = 6
    rng = seeded("rgbdelay", palette, w, inplace)
    on, strength = gu.rgbdelay_params({0: (1, 0, 0, 1.0), 1: (0, 1, 1, 0.8)})
    s = orc.orc_rgbdelay_new()
    steps, forms = [], []
    for f in range(2):
        src = st.put("src%d" % f, src_frame(rng, w, h, 3, st.pitch("src", w * 3)))
        want = src if inplace else st.put("dst%d" % f, noise(rng, h, st.pitch("dst", w * 3)))
        assert orc.orc_rgbdelay_process(s, P(src), src.strides[0], P(want), want.strides[0], w, h, palette, 1, 3, on.ctypes.data, strength.ctypes.data) == 0
        steps.append((src, want))
        d = "src%d" % f if inplace else "dst%d" % f
        forms.append("k_rgbdelay4" if (3 * w) % 4 == 0 and (st.bits(d) & 3) == 0 else "k_rgbdelay")
    orc.orc_rgbdelay_free(s)
    if st.gpu is not None:
        rd = st.gpu.RgbDelay()
        try:
            for f in range(2):
                ds = st.dev("src%d" % f)
                rd.process(ds, ds if inplace else st.dev("dst%d" % f), w, h, palette, 3, on, strength, yuv_clamped=True)
        finally:
            rd.close()
    for f, (src, want) in enumerate(steps):
        st.check("src%d" % f if inplace else "dst%d" % f, want, h, "rgbdelay pal=%d width %d inplace=%d frame %d" % (palette, w, inplace, f))
    assert forms[0] == forms[1] or st.place["off"]
    return forms[1]


def run_blurzoom(orc, st, palette, mode):
    """lgpu_blurzoom_process, two consecutive frames of one instance; 4-byte aligned frames and rowstrides or LGPU_E_BADARG"""
    w, h = 70, 16
    rng = seeded("blurzoom", palette, mode)
    compact = mode in (1, 2)
    z = orc.orc_blurzoom_new(w, h, palette)
    steps = []
    for f in range(2):
        a = src_frame(rng, w, h, 4, w * 4 if compact else st.pitch("src", w * 4))
        a[:h, :w * 4] = (a[:h, :w * 4] >> 4) + 40
        a[2 + 5 * f:8 + 5 * f, (8 + 5 * f) * 4:(24 + 5 * f) * 4] = 250          # a bright block moving over a dim noisy background, so that the background subtraction fires
        st.put("src%d" % f, a)
        want = st.put("dst%d" % f, noise(rng, h, w * 4 if compact else st.pitch("dst", w * 4)))
        assert orc.orc_blurzoom_process(z, P(a), a.strides[0], P(want), want.strides[0], mode, f) == 0
        steps.append(want)
    orc.orc_blurzoom_free(z)
    st.fams |= {"src", "dst"}
    form = BADARG if st.bits("src0", "src1", "dst0", "dst1") & 3 else "k_bz_*"
    if st.gpu is not None:
        g = st.gpu.Blurzoom(w, h, palette)
        try:
            for f in range(2):
                if not st.launch(lambda: g.process(st.dev("src%d" % f), st.dev("dst%d" % f), mode, f)):
                    return form
        finally:
            g.close()
    for f in range(2):
        st.check("dst%d" % f, steps[f], h, "blurzoom pal=%d mode=%d frame %d" % (palette, mode, f))
    return form


# ============================================================================================== the table
# a group: (id, runner, parameters, address classes, expected forms by class label, the forms the group's classes must reach between them)
def single(fams):
    return [(f, [f], r, m) for (f, r, m) in fams]


GROUPS = []


def group(gid, run, params, cls, expect, forms):
    """forms: a list or set is the exact set the classes reach; a frozenset names forms that must be among them"""
    GROUPS.append((gid, run, params, cls, expect, forms if isinstance(forms, frozenset) else set(forms)))


# ---- swizzle.hip: 4-byte sides are vector forms on 16-aligned rows, 3-byte sides on 4-aligned rows
for opname, lut in (("swap3", 1), ("swap3addpost", 0), ("delpost", 1), ("swap3postalpha", 1)):
    ib, ob = po.OP_IBPP[po.OPS.index(opname)], po.OP_OBPP[po.OPS.index(opname)]
    vec = "k_swizzle<%d,%d>" % (ib, ob)
    group("swizzle-%s" % opname, run_swizzle, (opname, lut, 1), classes([("src", ["src0"], 1, 16 if ib == 4 else 4), ("dst", ["dst0"], 1, 16 if ob == 4 else 4)]),
          {"aligned": vec, "src0+1": "k_swizzle_bytes", "dst0+2": "k_swizzle_bytes", "all": "k_swizzle_bytes", "pitch+8": vec if ib == ob == 3 else "k_swizzle_bytes"},
          [vec, "k_swizzle_bytes"])
    group("swizzle_batch-%s" % opname, run_swizzle, (opname, lut, 3), batch_classes([("src", 1, 16 if ib == 4 else 4), ("dst", 1, 16 if ob == 4 else 4)]),
          {"aligned": vec, "src1+1": "k_swizzle_bytes", "all": "k_swizzle_bytes"}, [vec, "k_swizzle_bytes"])
for ps, af in ((3, 0), (4, 0), (4, 1)):
    for rect in (0, 1):
        group("gamma-ps%d-af%d-rect%d" % (ps, af, rect), run_gamma, (ps, af, rect, 1), classes([("pix", ["pix0"], 1, 16)]),
              {"aligned": "k_gamma_apply", "pix0+4": "k_gamma_apply_bytes", "pix0+8": "k_gamma_apply_bytes", "pitch+8": "k_gamma_apply_bytes"}, ["k_gamma_apply", "k_gamma_apply_bytes"])
    group("gamma_batch-ps%d-af%d" % (ps, af), run_gamma, (ps, af, 1, 3), batch_classes([("pix", 1, 16)]), {"aligned": "k_gamma_apply", "pix1+8": "k_gamma_apply_bytes"},
          ["k_gamma_apply", "k_gamma_apply_bytes"])
for af, un in ((0, 0), (1, 1)):
    group("premult-af%d-un%d" % (af, un), run_premult, (af, un, 1), classes([("pix", ["pix0"], 4, 16)]),
          {"aligned": "k_premult<true>", "pix0+4": "k_premult<false>", "pix0+8": "k_premult<false>", "pitch+4": "k_premult<false>", "pix0-refused": BADARG},
          ["k_premult<true>", "k_premult<false>", BADARG])
    group("premult_batch-af%d-un%d" % (af, un), run_premult, (af, un, 3), batch_classes([("pix", 4, 16)]),
          {"aligned": "k_premult<true>", "pix1+4": "k_premult<false>", "pix1-refused": BADARG}, ["k_premult<true>", "k_premult<false>", BADARG])
for ps in (3, 4):
    group("byte_luts-ps%d" % ps, run_byte_luts, (ps,), classes(single([("src", 1, 16), ("dst", 1, 16)])), {}, ["k_byte_luts<%d>" % ps])

# ---- effects.hip
for ps in (3, 4):
    for mode in (0, 1, 2):
        forms = ["k_mirror_v4", "k_mirror<4>"] if ps == 4 else ["k_mirror<3>"]
        group("mirror-mode%d-ps%d" % (mode, ps), run_mirror, (mode, ps, 1, 0), classes([("src", ["src0"], 1, 16 if ps == 4 else 4), ("dst", ["dst0"], 1, 16 if ps == 4 else 4)]),
              {"aligned": forms[0], "src0+4": forms[-1], "dst0+8": forms[-1]} if ps == 4 else {}, forms)
        group("mirror-mode%d-ps%d-inplace" % (mode, ps), run_mirror, (mode, ps, 1, 1), classes([("src", ["src0"], 1, 16 if ps == 4 else 4)]), {"aligned": forms[0]}, forms)
    group("mirror_batch-ps%d" % ps, run_mirror, (2, ps, 3, 0), batch_classes([("src", 1, 16 if ps == 4 else 4), ("dst", 1, 16 if ps == 4 else 4)]),
          {"aligned": forms[0], "src1+4": forms[-1]} if ps == 4 else {}, forms)
    group("mirror_batch-ps%d-inplace" % ps, run_mirror, (0, ps, 3, 1), batch_classes([("src", 1, 16 if ps == 4 else 4)]), {}, forms)
for ps in (1, 3, 4):
    r, m = (4, 16) if ps == 4 else (1, 4)
    forms = ["k_letterbox<4> vec", "k_letterbox<4>", BADARG] if ps == 4 else ["k_letterbox<%d>" % ps]
    group("letterbox-ps%d" % ps, run_letterbox, (ps, 1), classes([("src", ["src0"], r, 4 if ps == 4 else m), ("dst", ["dst0"], r, m)]),
          {"aligned": forms[0], "dst0+4": "k_letterbox<4>", "dst0+8": "k_letterbox<4>", "src0-refused": BADARG, "dst0-refused": BADARG} if ps == 4 else {}, forms)
    group("letterbox_batch-ps%d" % ps, run_letterbox, (ps, 3), batch_classes([("src", r, 4 if ps == 4 else m), ("dst", r, m)]),
          {"aligned": forms[0], "dst1+8": "k_letterbox<4>", "dst1-refused": BADARG} if ps == 4 else {}, forms)
    group("letterbox_bars-ps%d" % ps, run_letterbox_bars, (ps,), classes(single([("dst", r, m)])), {"dst-refused": BADARG} if ps == 4 else {},
          ["k_letterbox_bars<%d>" % ps] + ([BADARG] if ps == 4 else []))
for kind, ps, extra in (("chroma", 3, 0), ("chroma", 4, 0), ("chroma", 4, 1), ("luma", 3, 1), ("luma", 4, 3), ("multi", 3, 0), ("multi", 3, 5), ("colorkey", 3, 0)):
    r, m = (4, 16) if ps == 4 else (1, 4)
    argb = kind == "chroma" and ps == 4 and extra
    forms = ["k_chroma_argb"] if argb else ["k_pixel2<%d> vec" % ps, "k_pixel2<%d> bytes" % ps]
    group("%s-ps%d-%d" % (kind, ps, extra), run_pixel2, (kind, ps, extra, 1), classes([("a", ["a0"], r, m), ("b", ["b0"], r, m), ("dst", ["dst0"], r, m)]),
          {"aligned": forms[0], "b0+%d" % (m // 2): forms[-1], "all": forms[-1], "a0-refused": BADARG} if ps == 4 else {"aligned": forms[0], "a0+1": forms[-1], "dst0+2": forms[-1]},
          forms + ([BADARG] if ps == 4 else []))
group("colorkey_batch", run_pixel2, ("colorkey", 3, 0, 3), batch_classes([("a", 1, 4), ("b", 1, 4), ("dst", 1, 4)]),
      {"aligned": "k_pixel2<3> vec", "b1+1": "k_pixel2<3> bytes", "dst1+2": "k_pixel2<3> bytes"}, ["k_pixel2<3> vec", "k_pixel2<3> bytes"])

# ---- resize.hip.  136 x 20 -> 68 x 10: two kTileW tiles across, every window on the frame's border; 272 x 72 -> 136 x 36: tile (1, 1) has its window inside the frame
GENERIC = "k_hpass_generic + k_vpass_generic"
RESIZE4 = classes(single([("src", 1, 16), ("dst", 1, 16)]))
for shape in ((136, 20, 68, 10), (272, 72, 136, 36)):
    group("resize-ps4-%dx%d-%dx%d" % shape, run_resize, (4,) + shape, RESIZE4,
          {"aligned": "k_half8s xoff 1", "src+4": "k_half8s xoff 0", "src+8": "k_half8s xoff 0", "pitch+4": "k_half8s xoff 0", "pitch+8": "k_half8s xoff 0", "dst+4": "k_half8s xoff 1",
           "dst+8": "k_half8s xoff 1", "src+1": GENERIC, "src+2": GENERIC, "pitch+1": GENERIC, "pitch+2": GENERIC, "base12-pitch4": "k_half8s xoff 0", "all": GENERIC},
          ["k_half8s xoff 1", "k_half8s xoff 0", GENERIC])
group("resize-ps4-200x60-133x40", run_resize, (4, 200, 60, 133, 40), RESIZE4,
      {"aligned": "plan_sep vec 1", "src+4": "plan_sep vec 0", "src+8": "plan_sep vec 0", "pitch+4": "plan_sep vec 0", "dst+4": "plan_sep vec 1", "src+2": GENERIC, "pitch+1": GENERIC},
      ["plan_sep vec 1", "plan_sep vec 0", GENERIC])
for ps in (1, 3):
    for shape in ((136, 20, 68, 10), (50, 14, 67, 20)):
        group("resize-ps%d-%dx%d-%dx%d" % ((ps,) + shape), run_resize, (ps,) + shape, classes(single([("src", 1, 4), ("dst", 1, 4)])), {}, [GENERIC])
# lgpu_gauss5, 4-byte pixels at width 40: the four forms by (base, pitch) of the source
group("gauss5-ps4-40x12", run_gauss5, (4, 40, 12), classes(single([("src", 1, 16), ("dst", 1, 16)])),
      {"aligned": "gauss5_rows", "src+8": "k_gauss5x", "pitch+8": "k_gauss5x", "dst+4": "k_gauss5x", "dst+8": "k_gauss5x", "src+4": "plan_sep(5,5) vec 0", "pitch+4": "plan_sep(5,5) vec 0",
       "base12-pitch4": "plan_sep(5,5) vec 0", "src+1": GENERIC, "pitch+1": GENERIC, "pitch+2": GENERIC},
      ["gauss5_rows", "k_gauss5x", "plan_sep(5,5) vec 0", GENERIC])
group("gauss5-ps4-72x9", run_gauss5, (4, 72, 9), classes(single([("src", 1, 16), ("dst", 1, 16)])), {"aligned": "gauss5_rows", "src+4": "plan_sep(5,5) vec 0"},
      ["gauss5_rows", "k_gauss5x", "plan_sep(5,5) vec 0", GENERIC])
group("gauss5-ps3-40x12", run_gauss5, (3, 40, 12), classes(single([("src", 1, 4), ("dst", 1, 4)])), {"aligned": "gauss5_rows", "src+1": GENERIC, "dst+2": GENERIC, "pitch+2": GENERIC},
      ["gauss5_rows", GENERIC])
group("gauss5-ps1-40x12", run_gauss5, (1, 40, 12), classes(single([("src", 1, 4), ("dst", 1, 4)])), {}, [GENERIC])
# lgpu_chain, polyphase, three tracks: only track 1 leaves the aligned class (track 0 stays aligned); layer 2 and the destination at 4 and 8 in turn
CHAIN_CLASSES = [("aligned", pl()), ("src1+4", pl(src1=4)), ("src1+8", pl(src1=8)), ("src-pitch+4", pl(dp={"src": 4})), ("src1+4-l21+4-dst1+8", pl(src1=4, l21=4, dst1=8)),
                 ("l21+8-dst1+4", pl(l21=8, dst1=4)), ("l2-dst-pitch+4", pl(dp={"l2": 4, "dst": 4})), ("base12-pitch4", pl(dp={"src": 4, "l2": 4, "dst": 4}, src1=12, l21=12, dst1=12)),
                 ("src1-refused", pl(src1=2)), ("l21-refused", pl(l21=1)), ("dst1-refused", pl(dst1=2))]
for blur in (0, 1):
    tail = ", blur from scratch" if blur else ""
    group("chain-136x20-68x10-blur%d" % blur, run_chain, (136, 20, 68, 10, blur), CHAIN_CLASSES,
          {"aligned": "k_half8s xoff 1" + tail, "src1+4": "k_half8s xoff 0" + tail, "src1+8": "k_half8s xoff 0" + tail, "src-pitch+4": "k_half8s xoff 0" + tail,
           "src1+4-l21+4-dst1+8": "k_half8s xoff 0" + tail, "l21+8-dst1+4": "k_half8s xoff 1" + tail, "src1-refused": BADARG, "l21-refused": BADARG, "dst1-refused": BADARG},
          ["k_half8s xoff 1" + tail, "k_half8s xoff 0" + tail, BADARG])
    group("chain-200x60-133x40-blur%d" % blur, run_chain, (200, 60, 133, 40, blur), CHAIN_CLASSES,
          {"aligned": "plan_sep vec 1" + tail, "src1+4": "plan_sep vec 0" + tail, "src-pitch+4": "plan_sep vec 0" + tail, "l21+8-dst1+4": "plan_sep vec 1" + tail},
          ["plan_sep vec 1" + tail, "plan_sep vec 0" + tail, BADARG])

# ---- pixbuf.hip
PB4 = [("src", 4, 16), ("dst", 4, 16)]
for interp in (3, 2):
    for aligned in (1, 0):
        half = "k_pb_half ALIGNED" if aligned else "k_pb_half plain"
        group("pixbuf-ch4-2to1-interp%d-strips64_%d" % (interp, aligned), run_pixbuf, (4, 128, 16, 64, 8, interp, 1, aligned), classes([("src", ["src0"], 4, 16), ("dst", ["dst0"], 4, 16)]),
              {"aligned": half, "src0+4": "k_pb_gather", "src0+8": "k_pb_gather", "dst0+4": "k_pb_gather", "dst0+8": half, "pitch+8": "k_pb_gather", "pitch+4": "k_pb_gather",
               "src0-refused": BADARG, "dst0-refused": BADARG}, [half, "k_pb_gather", BADARG])
    group("pixbuf_batch-ch4-2to1-interp%d" % interp, run_pixbuf, (4, 128, 16, 64, 8, interp, 3, 1), batch_classes(PB4),
          {"aligned": "k_pb_half ALIGNED", "src1+4": "k_pb_gather", "dst1+4": "k_pb_gather", "dst1+8": "k_pb_half ALIGNED", "src1-refused": BADARG}, ["k_pb_half ALIGNED", "k_pb_gather", BADARG])
group("pixbuf-ch4-1to2", run_pixbuf, (4, 32, 8, 64, 16, 3, 1), classes([("src", ["src0"], 4, 16), ("dst", ["dst0"], 4, 16)]),
      {"aligned": "k_pb_double", "src0+8": "k_pb_double", "src0+4": "k_pb_up", "dst0+4": "k_pb_up", "dst0+8": "k_pb_up", "pitch+8": "k_pb_up"}, ["k_pb_double", "k_pb_up", BADARG])
group("pixbuf_batch-ch4-1to2", run_pixbuf, (4, 32, 8, 64, 16, 3, 3), batch_classes(PB4), {"aligned": "k_pb_double", "src1+4": "k_pb_up", "dst1+8": "k_pb_up"}, ["k_pb_double", "k_pb_up", BADARG])
for shape in ((96, 12, 32, 4), (96, 12, 64, 8), (64, 8, 96, 12)):            # 3:1, 3:2, 2:3
    group("pixbuf-ch4-%dx%d-%dx%d" % shape, run_pixbuf, (4,) + shape + (3, 1), classes([("src", ["src0"], 4, 16), ("dst", ["dst0"], 4, 16)]), {"src0-refused": BADARG}, ["general", BADARG])
# 3-byte frames sit at 1, 2 and 3 mod 4: the powers of two of classes(), and offset 3 on its own
PB3 = classes([("src", ["src0"], 1, 4), ("dst", ["dst0"], 1, 4)]) + [("src0+3", pl(src0=3)), ("dst0+3", pl(dst0=3)), ("src0+3-dst0+3", pl(src0=3, dst0=3))]
for interp in (3, 2):
    group("pixbuf-ch3-2to1-interp%d" % interp, run_pixbuf, (3, 64, 16, 32, 8, interp, 1), PB3,
          {"aligned": "k_pb_half3", "src0+1": "k_pb_pairs<3>", "src0+2": "k_pb_pairs<3>", "src0+3": "k_pb_pairs<3>", "dst0+1": "k_pb_pairs<3>", "dst0+3": "k_pb_pairs<3>",
           "src0+3-dst0+3": "k_pb_pairs<3>", "pitch+2": "k_pb_pairs<3>", "pitch+4": "k_pb_half3"}, ["k_pb_half3", "k_pb_pairs<3>"])
group("pixbuf_batch-ch3-2to1", run_pixbuf, (3, 64, 16, 32, 8, 3, 3), batch_classes([("src", 1, 4), ("dst", 1, 4)]) + [("src1+3", pl(src1=3)), ("dst1+3", pl(dst1=3))],
      {"aligned": "k_pb_half3", "src1+1": "k_pb_pairs<3>", "src1+3": "k_pb_pairs<3>", "dst1+3": "k_pb_pairs<3>", "all": "k_pb_pairs<3>"}, ["k_pb_half3", "k_pb_pairs<3>"])
group("pixbuf-ch3-3to2", run_pixbuf, (3, 96, 12, 64, 8, 3, 1), PB3, {}, ["general"])

# ---- palette.hip
for palette in (588, 589, 544, 545, 522, 512, 513, 564, 565):
    np_ = 1 if palette in (588, 589, 564, 565) else 4 if palette == 545 else 3
    cls = [("aligned", pl()), ("p0+5", pl(p0=5))] + [("p%d+%d" % (k, o), pl(**{"p%d" % k: o})) for k in range(min(np_, 3)) for o in (1, 2, 4, 8)] + \
          [("all", pl(**{"p%d" % k: (5, 3, 9, 7)[k] for k in range(np_)})), ("pitch+2", pl(dp={"p": 2}))]
    first = "k_clamp_switch head" + (" / tail only / tail only" if np_ >= 3 else "")
    group("clamp_switch-%d" % palette, run_clamp_switch, (palette, palette & 1), cls, {"p0+5": first, "all": "k_clamp_switch " + " / ".join(["head"] * min(np_, 3))}, frozenset([first]))
for order, ia in ((0, 1), (1, 1), (0, 0), (1, 0)):
    ips = 4 if ia else 3
    for fmt in range(6):
        oa = 1 if (fmt <= 1 and ia) else 0
        nd = 1 if fmt in (0, 2, 3) else (4 if oa else 3)
        dm = [16 if oa else 4] if fmt == 0 else [4] * nd if fmt == 1 else [8] if fmt in (2, 3) else [4, 2, 2]
        dr = 4 if fmt in (2, 3) else 1
        cell = {0: "k_rgb_to_yuv444_s", 1: "k_rgb_to_yuv444_s", 2: "k_rgb_to_yuv422_s", 3: "k_rgb_to_yuv422_s", 4: "k_rgb_to_yuv420_s", 5: "k_rgb_to_yuv422_s"}[fmt]
        fast = cell if (ips == 4 or fmt <= 1) else "k_rgb_to_yuv"
        exp = {"aligned": fast, "src+1": "k_rgb_to_yuv", "all": "k_rgb_to_yuv"}
        if fast != "k_rgb_to_yuv":
            exp["dst%d+%d" % (nd - 1, dm[nd - 1] // 2)] = "k_rgb_to_yuv"          # exactly one plane misaligned at a width that qualifies: the fallback
        if dr > 1:
            exp["dst0-refused"] = BADARG
        group("rgb_to_yuv-order%d-alpha%d-fmt%d" % (order, ia, fmt), run_rgb_to_yuv, (order, ia, fmt, 1),
              classes(single([("src", 1, 16 if ips == 4 else 4)] + [("dst%d" % k, dr, dm[k]) for k in range(nd)])), exp, {fast, "k_rgb_to_yuv"} | ({BADARG} if dr > 1 else set()))
for fmt in (0, 2, 4, 5):
    nd = 1 if fmt in (0, 2) else 3
    cell = {0: "k_rgb_to_yuv444_s", 2: "k_rgb_to_yuv422_s", 4: "k_rgb_to_yuv420_s", 5: "k_rgb_to_yuv422_s"}[fmt]
    group("rgb_to_yuv_batch-fmt%d" % fmt, run_rgb_to_yuv, (1, 1, fmt, 3), batch_classes([("src", 1, 16)]) + [("dst1_%d+1" % (nd - 1), pl(**{"dst1_%d" % (nd - 1): 4 if fmt == 2 else 1}))],
          {"aligned": cell, "src1+4": "k_rgb_to_yuv", "dst1_%d+1" % (nd - 1): "k_rgb_to_yuv"}, [cell, "k_rgb_to_yuv"])
for fmt, ia, order, oa in ((0, 0, 0, 0), (0, 1, 1, 1), (0, 1, 2, 1), (1, 0, 0, 1), (1, 1, 1, 1), (1, 1, 0, 0), (2, 0, 0, 0), (2, 0, 2, 1), (3, 0, 1, 0), (3, 0, 0, 1)):
    ns = (4 if ia else 3) if fmt == 1 else 1
    ops = 4 if (order == 2 or oa) else 3
    sr, sm = (4, 8) if fmt >= 2 else (1, (16 if ia else 4) if fmt == 0 else 4)
    fast = "k_uyvy_to_rgb_s" if (fmt >= 2 and ops == 4) else "k_yuv444_to_rgb_s" if fmt <= 1 else "k_yuv_to_rgb"
    exp = {"aligned": fast, "all": "k_yuv_to_rgb"}
    if fast != "k_yuv_to_rgb":
        exp["dst+%d" % (8 if ops == 4 else 2)] = "k_yuv_to_rgb"
        exp["src%d+%d" % (ns - 1, sm // 2)] = "k_yuv_to_rgb"
    if sr > 1:
        exp["src0-refused"] = BADARG
    group("yuv_to_rgb-fmt%d-ia%d-order%d-oa%d" % (fmt, ia, order, oa), run_yuv_to_rgb, (fmt, ia, order, oa, 1),
          classes(single([("src%d" % k, sr, sm) for k in range(ns)] + [("dst", 1, 16 if ops == 4 else 4)])), exp, {fast, "k_yuv_to_rgb"} | ({BADARG} if sr > 1 else set()))
for fmt, ia, order, oa in ((0, 1, 0, 1), (1, 0, 0, 1), (2, 0, 0, 1)):
    fast = "k_uyvy_to_rgb_s" if fmt == 2 else "k_yuv444_to_rgb_s"
    group("yuv_to_rgb_batch-fmt%d" % fmt, run_yuv_to_rgb, (fmt, ia, order, oa, 3), batch_classes([("dst", 1, 16)]) + [("src1_0+4", pl(src1_0=4))],
          {"aligned": fast, "dst1+8": "k_yuv_to_rgb", "src1_0+4": "k_yuv_to_rgb" if fmt != 1 else fast}, [fast, "k_yuv_to_rgb"])
# lgpu_yuv_repack: one pair per kind that has a cell form, at 40 and 72 pixels
for ip, op, cell in ((512, 564, "k_420_to_packed_s"), (545, 589, "k_combine_s"), (544, 588, "k_combine_s"), (588, 544, "k_split_s"), (564, 565, "k_swab_s"), (564, 512, "k_pk_to_s"),
                     (565, 544, "k_pk_to_s"), (564, 589, "k_pk_to_s"), (589, 512, "k_888_to_s"), (588, 522, "k_888_to_s"), (589, 565, "k_888_to_s"), (512, 522, "k_420_to_422p_s")):
    padok = [p_[2] for p_ in po.YUV_REPACK_PAIRS if p_[:2] == (ip, op)][0]
    ns, nd = len(po.YUV_PLANE_DIMS[ip](8, 8)), len(po.YUV_PLANE_DIMS[op](8, 8))
    cls = classes(single([("s%d" % k, 1, 16) for k in range(ns)] + [("d%d" % k, 1, 16) for k in range(nd)]))
    if not padok:
        cls = [c for c in cls if not c[1]["dp"]]
    for w in (40, 72):
        group("repack-%d-%d-w%d" % (ip, op, w), run_repack, (ip, op, w, padok), cls, {"aligned": cell, "s0+1": "k_yuv_repack", "all": "k_yuv_repack"}, [cell, "k_yuv_repack"])
# the 4:1:1 pairs (k_yuv411_repack): one out of and one into YUV411, compact rows on both sides as the reference walks them, so base offsets only
for ip, op in ((595, 589), (565, 595)):
    assert (ip, op, 0) in po.YUV411_REPACK_PAIRS
    cls = [c for c in classes(single([("s0", 1, 16), ("d0", 1, 16)])) if not c[1]["dp"]]
    for w in (40, 72):
        group("repack-%d-%d-w%d" % (ip, op, w), run_repack, (ip, op, w, 0), cls, {"aligned": "k_yuv411_repack", "all": "k_yuv411_repack"}, ["k_yuv411_repack"])

# ---- yuv.hip
for opsize, is422, use_lut in ((4, 0, 1), (4, 1, 0), (3, 0, 1), (3, 1, 0)):
    fast = "k_yuv420p_to_rgb_s" if opsize == 4 else "k_yuv420p_to_rgb"
    exp = {"aligned": fast, "y+1": "k_yuv420p_to_rgb", "y+2": "k_yuv420p_to_rgb", "u+1": fast, "v+1": fast, "all": "k_yuv420p_to_rgb"}
    if opsize == 4:
        exp.update({"dst+4": "k_yuv420p_to_rgb", "dst+8": "k_yuv420p_to_rgb", "dst-refused": BADARG, "pitch+2": "k_yuv420p_to_rgb"})
    group("yuv420p_to_rgb-ops%d-422_%d" % (opsize, is422), run_yuv420p, (opsize, is422, use_lut, 1),
          classes(single([("y", 1, 4), ("u", 1, 4), ("v", 1, 4), ("dst", 4 if opsize == 4 else 1, 16 if opsize == 4 else 4)])), exp, {fast, "k_yuv420p_to_rgb"} | ({BADARG} if opsize == 4 else set()))
    group("yuv420p_to_rgb_batch-ops%d-422_%d" % (opsize, is422), run_yuv420p, (opsize, is422, use_lut, 3),
          batch_classes([("y", 1, 4), ("u", 1, 4), ("v", 1, 4), ("dst", 4 if opsize == 4 else 1, 16 if opsize == 4 else 4)]),
          {"aligned": fast, "y1+2": "k_yuv420p_to_rgb", "u1+1": fast}, {fast, "k_yuv420p_to_rgb"} | ({BADARG} if opsize == 4 else set()))
group("yuv420p_to_rgb_lut16", run_yuv420p, (4, 0, 0, 1, 1), classes(single([("y", 1, 4), ("u", 1, 4), ("v", 1, 4), ("dst", 4, 16)])), {"aligned": "k_yuv420p_to_rgb", "dst-refused": BADARG},
      ["k_yuv420p_to_rgb", BADARG])

# ---- effects.hip and palette.hip: two frames in and one out, lgpu_fx_batch, softlight, the 4:1:1 conversions; stencil.hip: deinterlace, edge; lgpu_composite
for ps in (3, 4):
    r, m = 1, 4
    three = lambda: classes([("a", ["a0"], r, m), ("b", ["b0"], r, m), ("dst", ["dst0"], r, m)])
    for kind in (0, 1, 2):
        group("transition-kind%d-ps%d" % (kind, ps), run_two, ("transition", ps, kind, 1, 0), three(), {}, ["k_transition<%d>" % ps])
    group("fx_batch-transition-ps%d" % ps, run_two, ("transition", ps, ps - 3, 3, 1), batch_classes([("a", r, m), ("b", r, m), ("dst", r, m)]), {}, ["k_transition<%d>" % ps])
    for dirn in (1, 4):
        group("slide_over-dir%d-ps%d" % (dirn, ps), run_two, ("slide_over", ps, dirn, 1, 0), three(), {}, ["k_slide_over<%d>" % ps])
    group("dissolve-ps%d" % ps, run_two, ("dissolve", ps, 0, 1, 0), three(), {}, ["k_dissolve<%d>" % ps])
    m5 = 16 if ps == 4 else 4
    fused = "k_gauss5_colorkey<%d>" % ps
    group("gauss5_colorkey-ps%d" % ps, run_two, ("gauss5_colorkey", ps, 0, 1, 0), classes([("a", ["a0"], 1, m5), ("b", ["b0"], 1, m5), ("dst", ["dst0"], 1, m5)]),
          {"aligned": fused, "a0+%d" % (m5 // 2): UNSUPPORTED, "b0+1": UNSUPPORTED, "dst0+%d" % (m5 // 2): UNSUPPORTED, "pitch+%d" % (m5 // 2): UNSUPPORTED}, [fused, UNSUPPORTED])
    group("fx_batch-gauss5_colorkey-ps%d" % ps, run_two, ("gauss5_colorkey", ps, 0, 3, 1), batch_classes([("a", 1, m5), ("b", 1, m5), ("dst", 1, m5)]),
          {"aligned": fused, "b1+%d" % (m5 // 2): UNSUPPORTED}, [fused, UNSUPPORTED])
for is_rows in (0, 1):
    group("triple_split-rows%d" % is_rows, run_two, ("triple_split", 3, is_rows, 1, 0), classes([("a", ["a0"], 1, 4), ("b", ["b0"], 1, 4), ("dst", ["dst0"], 1, 4)]), {}, ["k_triple_split"])
for name, ps, prm in (("chroma", 3, 0), ("chroma", 4, 0), ("luma", 3, 2), ("luma", 4, 4), ("multi", 3, 3)):
    r, m = (4, 16) if ps == 4 else (1, 4)
    group("fx_batch-%s-ps%d" % (name, ps), run_two, (name, ps, prm, 3, 1), batch_classes([("a", r, m), ("b", r, m), ("dst", r, m)]),
          {"aligned": "k_pixel2<%d> vec" % ps, "b1+%d" % (m // 2): "k_pixel2<%d> bytes" % ps}, ["k_pixel2<%d> vec" % ps, "k_pixel2<%d> bytes" % ps] + ([BADARG] if ps == 4 else []))
for palette, w in ((544, 40), (545, 40), (522, 40), (512, 40), (544, 8), (522, 8)):
    nplanes = 4 if palette == 545 else 3
    fams = [("s_%d" % k, 1, 16 if k else 4) for k in range(nplanes)] + [("d_%d" % k, 1, 16 if k else 4) for k in range(nplanes)]
    group("softlight-%d-w%d" % (palette, w), run_softlight, (palette, w, 1), classes(single(fams)),
          {"aligned": "k_softlight_s", "s_0+1": "k_softlight", "d_0+2": "k_softlight", "s_1+1": "k_softlight_s", "pitch+2": "k_softlight"}, ["k_softlight_s", "k_softlight"])
for palette in (544, 522):
    group("fx_batch-softlight-%d" % palette, run_softlight, (palette, 40, 3),
          [("aligned", pl()), ("s1_0+1", pl(s1_0=1)), ("d1_0+2", pl(d1_0=2)), ("s1_1+1-d1_2+4", pl(s1_1=1, d1_2=4)), ("all", pl(s1_0=1, s1_1=2, s1_2=3, d1_0=5, d1_1=6, d1_2=7))],
          {"aligned": "k_softlight_s", "s1_0+1": "k_softlight", "d1_0+2": "k_softlight", "s1_1+1-d1_2+4": "k_softlight_s"}, ["k_softlight_s", "k_softlight"])
for order, oa in ((0, 0), (1, 1), (2, 0)):
    group("yuv411_to_rgb-order%d-alpha%d" % (order, oa), run_yuv411_to_rgb, (order, oa, 1), [c for c in classes([("src", ["src0"], 1, 4), ("dst", ["dst0"], 1, 4)]) if "src" not in c[1]["dp"]], {},
          ["k_yuv411_to_rgb"])
    group("fx_batch-yuv411_to_rgb-order%d-alpha%d" % (order, oa), run_yuv411_to_rgb, (order, oa, 3), batch_classes([("src", 1, 4), ("dst", 1, 4)]), {}, ["k_yuv411_to_rgb"])
for order, ia in ((0, 0), (1, 1)):
    group("rgb_to_yuv411-order%d-alpha%d" % (order, ia), run_rgb_to_yuv411, (order, ia), [c for c in classes(single([("src", 1, 16 if ia else 4), ("dst", 1, 4)])) if "dst" not in c[1]["dp"]], {},
          ["k_rgb_to_yuv411"])
for palette, w in ((1, 21), (3, 21), (3, 20), (589, 21), (564, 20)):
    ps = 3 if palette == 1 else 4
    fast = "k_deinterlace dword" if (ps == 4 and w % 3 == 0 and palette != 564) else "k_deinterlace bytes"
    group("deinterlace-pal%d-w%d" % (palette, w), run_deinterlace, (palette, w, 0), classes(single([("src", 1, 4), ("dst", 1, 4)])),
          {"aligned": fast, "src+1": "k_deinterlace bytes", "dst+2": "k_deinterlace bytes"}, {fast, "k_deinterlace bytes"})
    group("deinterlace-pal%d-w%d-inplace" % (palette, w), run_deinterlace, (palette, w, 1), classes(single([("src", 1, 4)])), {"aligned": fast, "src+2": "k_deinterlace bytes"},
          {fast, "k_deinterlace bytes"})
for palette, mode in ((1, 0), (2, 2), (3, 1), (4, 2), (5, 0)):
    ps = 3 if palette <= 2 else 4
    forms = ["k_edge_map4 + k_edge_paint4", "k_edge_map<4> + k_edge_paint<4> dword", "k_edge_map<4> + k_edge_paint<4>"] if ps == 4 else ["k_edge_map<3> + k_edge_paint<3>"]
    m = 16 if ps == 4 else 4
    group("edge-pal%d-mode%d" % (palette, mode), run_edge, (palette, mode, 0), classes(single([("src", 1, m), ("dst", 1, m)])),
          {"aligned": forms[0], "src+4": forms[1], "dst+8": forms[1], "src+1": forms[2], "pitch+4": forms[1], "pitch+2": forms[2]} if ps == 4 else {}, forms)
    group("edge-pal%d-mode%d-inplace" % (palette, mode), run_edge, (palette, mode, 1), classes(single([("src", 1, m)])), {"aligned": forms[0]}, forms)
for ps, is_bgr, revz in ((3, 0, 0), (4, 1, 0), (4, 0, 1)):
    group("composite-ps%d-bgr%d-revz%d" % (ps, is_bgr, revz), run_composite, (ps, is_bgr, revz), classes(single([("l%d" % z, 1, 4) for z in range(4)] + [("dst", 1, 4)])), {},
          ["k_composite<%d>" % ps])

# ---- pixbuf.hip: the chains on the gdk-pixbuf arithmetic; then lgpu_alpha_premult_yuva, lgpu_rgb_to_yuv_lut16, lgpu_fill_pattern
PB_CHAIN = [("aligned", pl()), ("src1+4", pl(src1=4)), ("src1+8", pl(src1=8)), ("dst1+4", pl(dst1=4)), ("dst1+8", pl(dst1=8)), ("dst1+12", pl(dst1=12)), ("l21+4", pl(l21=4)),
            ("l21+8-dst1+8", pl(l21=8, dst1=8)), ("src-pitch+8", pl(dp={"src": 8})), ("dst-l2-pitch+4", pl(dp={"dst": 4, "l2": 4})),
            ("base12-pitch4", pl(dp={"src": 4, "l2": 4, "dst": 4}, src1=12, l21=12, dst1=12)), ("src1-refused", pl(src1=2)), ("l21-refused", pl(l21=2)), ("dst1-refused", pl(dst1=1))]
for blur, flag, amounts in ((0, 0, 1), (1, 0, 1), (0, OPAQUE, 1), (1, OPAQUE, 0), (0, 0, 0)):
    group("chain_pixbuf-128x16-64x8-blur%d-flag%x-amounts%d" % (blur, flag, amounts), run_chain_pb, (128, 16, 64, 8, blur, flag, amounts), PB_CHAIN,
          {"aligned": "k_pb_half chain", "src1+4": "staged", "src1+8": "staged", "dst1+4": "staged", "dst1+8": "k_pb_half chain", "dst1+12": "staged", "l21+4": "staged",
           "l21+8-dst1+8": "k_pb_half chain", "src-pitch+8": "staged", "dst-l2-pitch+4": "staged", "src1-refused": BADARG}, ["k_pb_half chain", "staged", BADARG])
def without_l2(cls):
    """LGPU_INTERP_NOBLEND: the tracks have no layer 2, so the classes that place one go and the others lose its pitch"""
    return [(label, pl(dp={k: v for k, v in place["dp"].items() if k != "l2"}, **{k: v for k, v in place["off"].items() if not k.startswith("l2")}))
            for label, place in cls if not label.startswith("l2")]


for blur, flag in ((0, 0), (1, 0), (0, OPAQUE)):
    group("chain_pixbuf-96x12-64x8-blur%d-flag%x" % (blur, flag), run_chain_pb, (96, 12, 64, 8, blur, flag, 1), PB_CHAIN, {"aligned": "staged"}, ["staged", BADARG])
for blur in (0, 1):          # off 2:1 without a layer 2: the scaler with the chain's last stages in its store (no blur), the stages one by one (blur)
    group("chain_pixbuf-96x12-64x8-blur%d-flag%x" % (blur, NOBLEND), run_chain_pb, (96, 12, 64, 8, blur, NOBLEND, 1), without_l2(PB_CHAIN),
          {"aligned": "staged", "dst1+4": "staged", "dst1+12": "staged", "src1+4": "staged", "base12-pitch4": "staged", "src1-refused": BADARG, "dst1-refused": BADARG},
          ["staged", BADARG])
for palette, clamped, un in ((589, 1, 0), (589, 1, 1), (589, 0, 0), (545, 1, 0), (545, 0, 1)):
    fams = [("p0", 1, 16)] if palette == 589 else [("p%d" % k, 1, 4) for k in range(4)]
    exp = {"aligned": "k_premult_yuva<1>" if clamped else "k_premult_yuva<0> dword", "p0+4": "k_premult_yuva<0> dword", "p0+1": "k_premult_yuva<0>", "pitch+8": "k_premult_yuva<0> dword"} \
        if palette == 589 else {"aligned": "k_premult_yuva<0>"}
    group("premult_yuva-%d-clamped%d-un%d" % (palette, clamped, un), run_premult_yuva, (palette, clamped, un), classes(single(fams)), exp, set(exp.values()))
for order, ia, fmt in ((0, 0, 2), (1, 1, 3)):
    group("rgb_to_yuv_lut16-order%d-alpha%d-fmt%d" % (order, ia, fmt), run_rgb_to_yuv_lut16, (order, ia, fmt), classes(single([("src", 1, 16 if ia else 4), ("dst", 4, 8)])),
          {"dst-refused": BADARG}, ["k_rgb_to_yuv", BADARG])
for plen in (1, 3, 4, 8):
    group("fill_pattern-plen%d" % plen, run_fill_pattern, (plen,), classes(single([("dst", 1, 16)])), {}, ["k_fill_pattern"])

# ---- pixbuf.hip: the 2:1 chain onto a letterbox canvas, and from decoded 4:2:0 planes
for blur, noblend in ((0, 0), (1, 0), (0, 1)):
    cls = without_l2(PB_CHAIN) if noblend else PB_CHAIN
    exp = {"aligned": "k_pb_half chain", "dst1+4": "staged", "dst1+8": "k_pb_half chain", "dst1+12": "staged", "src1+4": "staged"}
    group("chain_canvas-blur%d-noblend%d" % (blur, noblend), run_chain_canvas, (blur, noblend), cls, exp, ["k_pb_half chain", "staged", BADARG])
YUV_CHAIN = [("aligned", pl()), ("y1+1", pl(y1=1)), ("u1+1", pl(u1=1)), ("v1+1", pl(v1=1)), ("y1+1-u1+2-v1+3", pl(y1=1, u1=2, v1=3)), ("yuv-pitch+1", pl(dp={"y": 1, "u": 1, "v": 1})),
             ("dst1+8", pl(dst1=8)), ("l21+8", pl(l21=8)), ("dst1+4", pl(dst1=4)), ("l21+4", pl(l21=4)), ("dst-pitch+4", pl(dp={"dst": 4})), ("dst1-refused", pl(dst1=2)), ("l21-refused", pl(l21=1))]
for tight, canvas in ((1, None), (0, None), (1, (72, 12, 4, 2))):
    group("chain_yuv420p-tight%d-canvas%d" % (tight, 1 if canvas else 0), run_chain_yuv, (tight, canvas), YUV_CHAIN,
          {"aligned": "k_pb_half<YUV>", "y1+1-u1+2-v1+3": "k_pb_half<YUV>", "yuv-pitch+1": "k_pb_half<YUV>", "dst1+8": "k_pb_half<YUV>", "dst1+4": UNSUPPORTED, "l21+4": UNSUPPORTED,
           "dst-pitch+4": UNSUPPORTED, "dst1-refused": BADARG}, ["k_pb_half<YUV>", UNSUPPORTED, BADARG])

# ---- pixbuf.hip: the chains that end at a YUV sink
for fmt in (2, 3, 4):
    for yuvsrc in (0, 1):
        fused = "k_pb_half<YUV, SINK>" if yuvsrc else "k_pb_half<SINK>"
        npl = 3 if fmt == 4 else 1
        cls = [("aligned", pl())] + [("sink1_%d+%d" % (k, o), pl(**{"sink1_%d" % k: o})) for k in range(npl) for o in ((1, 2, 4, 8) if fmt == 4 else (4, 8))] + \
              [("l21+4", pl(l21=4)), ("l21+8", pl(l21=8)), ("sink-pitch+8", pl(dp={"sink_0": 8})), ("l21-refused", pl(l21=2))]
        exp = {"aligned": fused, "sink1_0+4": UNSUPPORTED, "sink1_0+8": UNSUPPORTED, "l21+4": UNSUPPORTED, "l21+8": fused, "sink-pitch+8": fused, "l21-refused": BADARG}
        if fmt == 4:
            cls += [("chroma-pitch+4", pl(dp={"sink_1": 4, "sink_2": 4})), ("chroma-pitch+2", pl(dp={"sink_1": 2, "sink_2": 2}))]
            exp.update({"sink1_2+1": UNSUPPORTED, "chroma-pitch+4": fused, "chroma-pitch+2": UNSUPPORTED})
        if yuvsrc:
            cls += [("y1+1-u1+2-v1+3", pl(y1=1, u1=2, v1=3))]
            exp["y1+1-u1+2-v1+3"] = fused
        else:
            cls += [("src1+4", pl(src1=4)), ("src1+8", pl(src1=8)), ("src-pitch+8", pl(dp={"src": 8})), ("src1-refused", pl(src1=2))]
            exp.update({"src1+4": UNSUPPORTED, "src1+8": UNSUPPORTED, "src-pitch+8": UNSUPPORTED, "src1-refused": BADARG})
        group("chain_sink-fmt%d-yuvsrc%d" % (fmt, yuvsrc), run_chain_sink, (fmt, yuvsrc), cls, exp, [fused, UNSUPPORTED, BADARG])

# ---- the stateful effects, two consecutive frames each: lgpu_rgbdelay_process, lgpu_blurzoom_process
for palette, w in ((1, 24), (2, 22), (588, 24)):
    quad = "k_rgbdelay4" if w == 24 else "k_rgbdelay"
    group("rgbdelay-pal%d-w%d" % (palette, w), run_rgbdelay, (palette, w, 0), classes([("src", ["src0", "src1"], 1, 4), ("dst", ["dst0", "dst1"], 1, 4)]),
          {"aligned": quad, "dst1+1": "k_rgbdelay", "dst1+2": "k_rgbdelay", "src1+1": quad, "pitch+2": "k_rgbdelay", "pitch+4": quad}, {quad, "k_rgbdelay"})
    group("rgbdelay-pal%d-w%d-inplace" % (palette, w), run_rgbdelay, (palette, w, 1), classes([("src", ["src0", "src1"], 1, 4)]), {"aligned": quad, "src1+2": "k_rgbdelay"}, {quad, "k_rgbdelay"})
for palette, mode in ((3, 0), (4, 3), (3, 1)):
    cls = classes([("src", ["src0", "src1"], 4, 16), ("dst", ["dst0", "dst1"], 4, 16)])
    if mode == 1:
        cls = [c for c in cls if not c[1]["dp"]]            # the strobe modes take compact rows only
    group("blurzoom-pal%d-mode%d" % (palette, mode), run_blurzoom, (palette, mode), cls, {"aligned": "k_bz_*", "src0-refused": BADARG, "dst0-refused": BADARG}, ["k_bz_*", BADARG])

assert len({g[0] for g in GROUPS}) == len(GROUPS)


# ============================================================================================== the tests
def drive(orc, gpu, tune, grp):
    gid, run, params, cls, expect, forms = grp
    reached = set()
    assert set(expect) <= {label for label, _ in cls}, "%s: EXPECT names a class this group does not have: %s" % (gid, sorted(set(expect) - {label for label, _ in cls}))
    for label, place in cls:
        plan = Stage(None, place)
        planned = run(orc, plan, *params)                   # inputs, oracle, the oracle's guard bytes, the rule on the planned addresses
        plan.finish()
        if label in expect:
            assert planned == expect[label], "%s, class %s: the restated rule says %r, the table expects %r" % (gid, label, planned, expect[label])
        assert (planned == BADARG) == label.endswith("-refused"), "%s, class %s: %r" % (gid, label, planned)
        reached.add(planned)
        if gpu is None:
            continue
        st = Stage(gpu, place, tune, refusal=CODES.get(planned))
        try:
            actual = run(orc, st, *params)
        except AssertionError as e:
            raise AssertionError("%s, class %s (%s): %s" % (gid, label, planned, e)) from None
        assert actual == planned, "%s, class %s: the buffers handed over give %r by the restated rule, the planned class gives %r" % (gid, label, actual, planned)
    assert forms <= reached if isinstance(forms, frozenset) else reached == forms, "%s: its classes reach %s, the table says %s" % (gid, sorted(reached), sorted(forms))
    return reached


@G
@pytest.mark.parametrize("grp", GROUPS, ids=[g[0] for g in GROUPS])
def test_address_classes(gpu, orc, tune, grp):
    """one entry point at one shape through all of its address classes: every buffer against the oracle over its whole allocation, the refusals, the batch forms
    against the single-frame call on the same buffers, and the form the restated dispatch rule names for the buffers that were really handed over"""
    drive(orc, gpu, tune, grp)


PLANNED = {}


def planned_forms(orc):
    """every case without a GPU, once per session: group id -> the forms the restated rules give for its classes"""
    if len(PLANNED) != len(GROUPS):
        for grp in GROUPS:
            PLANNED[grp[0]] = drive(orc, None, None, grp)
    return PLANNED


def test_oracle_accepts_every_case(orc):
    """every case without a GPU: inputs, the oracle (a status of 0 wherever it reports one, nothing written past a frame), the restated rule on the planned address
    class against the table's expectation, and the set of forms each group reaches"""
    planned_forms(orc)


def test_the_forms_no_other_suite_reaches(orc):
    """the forms this module is the first to run, taken from what the restated rules GIVE for the planned classes (not from what the table declares): a class that is
    edited away, or a rule that stops naming the form, fails here"""
    reached, mixed = collections.defaultdict(set), collections.defaultdict(set)
    for (gid, run, params, cls, expect, forms) in GROUPS:
        got = planned_forms(orc)[gid]
        reached[gid.split("-")[0]] |= got
        # a mixed-alignment batch: a class that moves a buffer of slot 1 alone, and is not a refusal
        for label, place in cls:
            if place["off"] and not label.endswith("-refused") and all(re.search(r"1(_\d)?$", k) for k in place["off"]):
                mixed[gid.split("-")[1] if gid.startswith("fx_batch-") else gid.split("-")[0]].add(label)
    assert "k_half8s xoff 0" in reached["resize"] and "k_half8s xoff 0" in reached["chain"]
    assert "plan_sep(5,5) vec 0" in reached["gauss5"] and "plan_sep vec 0" in reached["resize"]
    assert any(f.startswith("k_clamp_switch head") for f in reached["clamp_switch"])
    assert "k_pb_half plain" in reached["pixbuf"] and "k_yuv411_repack" in reached["repack"]
    for batch in ("swizzle_batch", "gamma_batch", "premult_batch", "mirror_batch", "letterbox_batch", "colorkey_batch", "rgb_to_yuv_batch", "yuv_to_rgb_batch",
                  "yuv420p_to_rgb_batch", "pixbuf_batch"):
        assert mixed[batch], "%s has no class with slot 1 alone off the aligned class" % batch
        assert len(reached[batch] - {BADARG}) >= 2, batch
    assert {k for k in mixed if k in FX} == set(FX), "every LGPU_FX_* op has a batch whose slot 1 leaves the aligned class: %s" % sorted(set(FX) - set(mixed))


# ============================================================================================== the layer seam
needs_ref = pytest.mark.skipif(not po.have_ref(), reason="oracle/_ref (reference libweed) not built")


@needs_ref
@G
def test_layer_seam_on_frames_where_the_host_has_them(gpu, orc):
    """lives_gpu_layer_pin_device takes whatever pointer the host has: a BGRA32 frame whose device base is 4 mod 16, and a YUV420P frame whose planes sit at 1, 2 and
    3 mod 16 -- convert_layer_palette(RGBA32), resize_layer (2:1 on the gdk-pixbuf body), a flush and a sync, deferred and eager, against the oracle's composition;
    the caller's buffers are read and never written"""
    from lives_amd import lib
    from tests import weedhost as wh
    from tests.test_deferred import oracle_step, plan_step, view
    from tests.test_deferred_yuv import oracle_conv, yuv_layer
    L = lib.load()
    wh.bind(L)
    L.lives_gpu_layers_flush.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_int]
    L.lives_gpu_layer_pin_device.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p), ctypes.c_int, ctypes.c_void_p, ctypes.c_int]
    assert L.lives_gpu_get_resize_backend() == 1
    H = po.RefHost()
    rng = seeded("layer seam")
    sw, sh, dw, dh = 128, 16, 64, 8
    src = frame(rng, sw, sh, 4, stride=sw * 4 + 16, alpha_mix=True)
    Y, U, V = (rng.integers(0, 256, s, dtype=np.uint8) for s in ((sh, sw + 16), (sh // 2, sw // 2 + 8), (sh // 2, sw // 2 + 8)))
    want_rgba = oracle_step(orc, src, sw, sh, None, dw, dh, None, 0, None, True)
    want_yuv = oracle_step(orc, oracle_conv(orc, Y, U, V, sw, sh), sw, sh, None, dw, dh, None, 0, None, False)
    prev = L.lives_gpu_set_deferred(1)
    try:
        for deferred in (1, 0):
            L.lives_gpu_set_deferred(deferred)
            d_src = dev_at(src, 4)
            lay = wh.new_layer(4, sw, sh, [np.zeros_like(src)], gamma=1)                   # BGRA32; the host plane holds nothing: the pixels are on the device
            assert d_src.data_ptr() % 16 == 4 and L.lives_gpu_layer_pin_device(lay, (ctypes.c_void_p * 1)(d_src.data_ptr()), 1, None, 1) == 0
            plan_step(L, wh, H, lay, None, dw, dh, None, 0, None)
            assert L.lives_gpu_layers_flush((ctypes.c_void_p * 1)(lay), 1) == 0 and L.lives_gpu_layer_sync(lay) == 0
            assert (view(wh, lay)[:, :dw * 4] == want_rgba).all(), "BGRA32 frame at 4 mod 16, deferred=%d" % deferred
            assert L.lives_gpu_layer_forget(lay) == 0
            same_whole_at(d_src, src, src, sh, "the caller's BGRA32 frame")
            dY, dU, dV = dev_at(Y, 1), dev_at(U, 2), dev_at(V, 3)
            lay = yuv_layer(wh, 512, sw, sh, np.zeros_like(Y), np.zeros_like(U), np.zeros_like(V))
            assert L.lives_gpu_layer_pin_device(lay, (ctypes.c_void_p * 3)(dY.data_ptr(), dU.data_ptr(), dV.data_ptr()), 3, None, 1) == 0
            plan_step(L, wh, H, lay, None, dw, dh, None, 0, None)
            assert L.lives_gpu_layers_flush((ctypes.c_void_p * 1)(lay), 1) == 0 and L.lives_gpu_layer_sync(lay) == 0
            assert (view(wh, lay)[:, :dw * 4] == want_yuv).all(), "YUV420P planes at 1 / 2 / 3, deferred=%d" % deferred
            assert L.lives_gpu_layer_forget(lay) == 0
            for t, a, name in ((dY, Y, "Y"), (dU, U, "U"), (dV, V, "V")):
                same_whole_at(t, a, a, a.shape[0], "the caller's %s plane" % name)
    finally:
        L.lives_gpu_set_deferred(prev)
