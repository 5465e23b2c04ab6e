"""Device frames at a chosen address class, for tests/test_address_alignment.py.

tests/util.py:dev() uploads through torch.from_numpy(...).cuda(), and the allocator hands such buffers out at multiples of 256 bytes or more.  dev_at() places a
frame inside a larger flat allocation so that its base address is any residue mod 64 the caller asks for, with known random bytes in front of and behind it;
same_whole_at() then holds the WHOLE allocation -- the bytes in front of the frame, the image, the row padding, the guard rows and the bytes behind -- to what
the oracle left in a host copy of the same layout.  lives_amd/ops.py takes base and pitch from data_ptr() and stride(0), so the views pass straight through.
"""
import zlib

import numpy as np

SLACK = 64          # the residue is taken mod 64: every alignment any dispatcher looks at (2 .. 16) with room to spare


def dev_at(host_2d, off, lead=64, trail=64, device="cuda"):
    """a [rows, pitch] uint8 view with data_ptr() % 64 == off inside one flat tensor of lead + 64 + nbytes + trail bytes; lead and trail (and the slack of the 64)
    hold random bytes that whole() / same_whole_at() check afterwards.  device="cpu" builds the same thing in host memory (the construction is checked without a GPU)"""
    import torch
    assert host_2d.ndim == 2 and host_2d.dtype == np.uint8 and 0 <= off < SLACK
    rows, pitch = host_2d.shape
    n = rows * pitch
    total = lead + SLACK + n + trail
    flat = torch.empty(total, dtype=torch.uint8, device=device)
    s = lead + (off - (flat.data_ptr() + lead)) % SLACK
    image = np.random.default_rng(zlib.crc32(repr((rows, pitch, off, lead, trail)).encode())).integers(0, 256, total, dtype=np.uint8)
    image[s:s + n] = host_2d.reshape(-1)
    flat.copy_(torch.from_numpy(image))
    view = flat[s:s + n].view(rows, pitch)
    assert view.data_ptr() % SLACK == off and view.stride(0) == pitch and view.stride(1) == 1
    view.lgpu_flat, view.lgpu_image, view.lgpu_start = flat, image, s          # what whole() and same_whole_at() need; the view keeps the allocation alive
    return view


def whole(view):
    """the entire flat buffer behind a dev_at() view, as a host array"""
    import torch
    if view.is_cuda:
        torch.cuda.synchronize()
    return view.lgpu_flat.cpu().numpy()


def same_whole_at(view, want, before, rows, what):
    """the flat buffer behind `view` equals the upload with the oracle's result `want` in the frame's place -- bytes in front, image, row padding, guard rows and the
    bytes behind, all at once -- and the oracle itself left everything outside the first `rows` rows as it was in `before`"""
    assert want.shape == before.shape == tuple(view.shape), what
    assert (want[rows:] == before[rows:]).all(), what + ": the oracle wrote past the frame"
    s, pitch = view.lgpu_start, want.shape[1]
    expect = view.lgpu_image.copy()
    assert (expect[s:s + before.size] == before.reshape(-1)).all(), what + ": the upload was not `before`"
    expect[s:s + want.size] = want.reshape(-1)
    got = whole(view)
    bad = np.flatnonzero(got != expect)
    if len(bad):
        i = int(bad[0]) - s
        where = ("%d bytes in front of the frame" % -i if i < 0 else "%d bytes behind the buffer" % (i - want.size) if i >= want.size else
                 "row %d byte %d (of %d rows + %d guard rows, pitch %d)" % (i // pitch, i % pitch, rows, want.shape[0] - rows, pitch))
        raise AssertionError("%s (base %% 64 = %d): %d bytes differ, first at %s: got %d want %d" % (
            what, view.data_ptr() % SLACK, len(bad), where, got[bad[0]], expect[bad[0]]))
