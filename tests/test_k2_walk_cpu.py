"""CPU: K2's chroma walk as lives_amd/csrc/k2_walk.h writes it down -- which chroma sample feeds which pixel of convert_yuv420p_to_rgb_frame -- against the oracle.

tests/c/k2_walk_host.cpp includes the header and nothing from HIP, and converts frames with the header's accessor forms and plain integer arithmetic.  It is built with
the address and undefined-behaviour sanitizers and run as a child process; every plane is allocated at exactly its stated size, so the walk's read one past a plane's
end is checked by the sanitizer as well as by value.  Every byte is compared with orc_yuv420p_to_rgb, which writes the "evident intent" values into the pixels the
reference leaves undefined (tests/test_gpu_parity.py), so nothing is masked.

Shapes: column 0 alone (w = 2), columns 0 and 1 (the k < 2 seed), no row pair (h = 2), a pair without a trailing row (odd h), the last-byte clamp (every tight stride)."""
import ctypes
import itertools
import os
import subprocess

import numpy as np
import pytest

from lives_amd import lib
from oracle import pyoracle as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = po.P
WIDTHS, HEIGHTS = (2, 4, 6, 18), (2, 3, 4, 5, 9)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("k2_walk") / "k2_walk_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "lives_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "c", "k2_walk_host.cpp")])
    return exe


def test_header_compiles_without_hip():
    """plain C++17 under g++, no HIP header on the include path"""
    src = '#include "k2_walk.h"\nint main() { return 0; }\n'
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "lives_amd", "csrc"), "-x", "c++", "-"],
                   input=src, text=True, check=True)


def test_k2_walk_matches_oracle(host, orc, tmp_path):
    L = lib.load()
    tables = np.zeros((4, 5, 256), np.int32)
    for which in range(4):
        assert L.lgpu_conversion_tables(which, None, P(tables[which])) == 0
    rng = np.random.default_rng(1800)
    cases, blob = [], [tables.tobytes()]
    for w, h, pad, is422 in itertools.product(WIDTHS, HEIGHTS, (0, 3), (0, 1)):
        ys, cs, crows = w + pad, w // 2 + pad, (h if is422 else (h + 1) // 2)
        Y = rng.integers(0, 256, (h, ys), dtype=np.uint8)
        U = rng.integers(0, 256, (crows, cs), dtype=np.uint8)
        V = rng.integers(0, 256, (crows, cs), dtype=np.uint8)
        for which, quality, fix in itertools.product(range(4), (1, 2), (0, 1)):
            cases.append((w, h, is422, ys, cs, Y, U, V, which, quality, fix))
    blob.append(np.int32(len(cases)).tobytes())
    for (w, h, is422, ys, cs, Y, U, V, which, quality, fix) in cases:
        blob.append(np.array([w, h, is422, ys, cs, cs, Y.size, U.size, V.size, which, int(quality == 1), fix], np.int32).tobytes())
        blob += [Y.tobytes(), U.tobytes(), V.tobytes()]
    assert len(cases) == 1280
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    open(fin, "wb").write(b"".join(blob))
    r = subprocess.run([host, fin, fout], capture_output=True, text=True)
    assert r.returncode == 0, "k2_walk_host (sanitized) failed:\n" + r.stderr[-4000:]
    got_all = np.fromfile(fout, np.uint8)
    assert got_all.size == sum(4 * c[0] * c[1] for c in cases)
    off = 0
    for (w, h, is422, ys, cs, Y, U, V, which, quality, fix) in cases:
        got = got_all[off:off + 4 * w * h].reshape(h, 4 * w)
        off += 4 * w * h
        want = np.zeros((h, 4 * w), np.uint8)
        st = (ctypes.c_int * 3)(ys, cs, cs)
        assert orc.orc_yuv420p_to_rgb(P(Y), P(U), P(V), st, U.size, V.size, P(want), 4 * w, w, h, 4, 0, is422, which, quality, None, fix) == 0
        bad = np.argwhere(got != want)
        assert bad.size == 0, "%dx%d 422=%d stride %d which=%d quality=%d fix=%d: %d bytes differ, first at row %d byte %d (got %d, oracle %d)" % (
            w, h, is422, ys, which, quality, fix, len(bad), bad[0][0], bad[0][1], got[tuple(bad[0])], want[tuple(bad[0])])
