"""The descriptions of a decoded YUV source (lgpu_yuv_source, lgpu_yuv422_source) and of a YUV sink (lgpu_chain_sink) are checked the same way by every one-launch
form of the tick that takes them: ONE table of bad source descriptions and ONE table of bad sink descriptions, each row through every entry point that takes the
struct (src and src2 of the mix form included).  Every combination returns LGPU_E_BADARG and leaves every destination plane as it was.

Shapes: two tracks; 16x8 -> 8x4 for the 2:1 forms (the smallest with sw % 4 == 0, dw % 4 == 0 and dh even), 16x8 unscaled for the flat forms.  A refused call
launches nothing; the one good call per entry point that opens each test shows that the row alone is what is refused."""
import pytest

E_BADARG = -2
PIXBUF = 0x100
UYVY, YUV420P, YUV422P = 2, 4, 5
W, H, NT, FILL = 16, 8, 2, 0x5C

# a row that the entry points answer differently: {(row, entry point): code}, taken from the commit before the checks were shared.  Empty: they all agree.
EXPECT = {}


@pytest.fixture(scope="module")
def bufs(gpu):
    import torch
    z = lambda rows, cols: [torch.zeros((rows, cols), dtype=torch.uint8, device="cuda") for _ in range(NT)]      # noqa: E731
    b = dict(Y=z(H, W * 2), U=z(H, W), V=z(H, W), Y2=z(H, W), U2=z(H // 2, W // 2), V2=z(H // 2, W // 2), RGBA=z(H, W * 4), L2=z(H, W * 4))
    b["D"] = [[torch.full((H, W * 4), FILL, dtype=torch.uint8, device="cuda") for _ in range(3)] for _ in range(NT)]
    return b


def base_source(fmt):
    """a good description of a W x H frame: 4 YUV420P, 5 YUV422P, 2 UYVY"""
    hw, ch = W // 2, (H if fmt == YUV422P else (H + 1) // 2)
    if fmt == UYVY:
        return dict(strides=[W * 2, 0, 0], u_size=0, v_size=0, out_order=0, which_tables=0, pb_quality=2, flags=0)
    return dict(strides=[W, hw, hw], u_size=ch * hw, v_size=ch * hw, out_order=0, which_tables=0, pb_quality=2, flags=0)


def base_sink(dw, fmt=YUV420P):
    return dict(out_fmt=fmt, orow=[dw, dw // 2, dw // 2] if fmt >= 4 else [dw * 2, 0, 0], which_tables=0, in_order=0)


def entry_points(ops, b):
    """name -> (call(source description, second source description, sink description) -> the library's code, the source format, takes a sink)"""
    def prm(scaled):
        dw, dh = (W // 2, H // 2) if scaled else (W, H)
        return ops.chain_params(W, H, W * 4, dw, dh, dw * 4, dw * 4, swap_rb=0, interp=3 | PIXBUF, do_blur=0, bf=0)

    def src(d):
        return ops.yuv_source(d["strides"], d["u_size"], d["v_size"], out_order=d["out_order"], which_tables=d["which_tables"], pb_quality=d["pb_quality"], flags=d["flags"])

    def src422(fmt, d):
        return ops.yuv422_source(fmt, d["strides"], d["u_size"], d["v_size"], out_order=d["out_order"], which_tables=d["which_tables"], pb_quality=d["pb_quality"])

    def sink(k):
        return ops.chain_sink(k["out_fmt"], k["orow"], which_tables=k["which_tables"], in_order=k["in_order"]) if k is not None else None

    am = [9] * NT
    yuv_tracks = ops.chain_yuv_tracks(b["Y"], b["U"], b["V"], b["L2"], [d[0] for d in b["D"]])
    yuv_sink_tracks = ops.chain_yuv_sink_tracks(b["Y"], b["U"], b["V"], b["L2"], b["D"])
    packed_tracks = ops.chain_yuv_sink_tracks(b["Y"], None, None, b["L2"], b["D"])
    sink_tracks = ops.chain_sink_tracks(b["RGBA"], b["L2"], b["D"])
    mix_tracks = ops.chain_yuv_mix_tracks(b["Y"], b["U"], b["V"], b["Y2"], b["U2"], b["V2"], b["D"])
    return {
        "chain_yuv420p": (lambda s, s2, k: ops.chain_yuv420p(prm(True), src(s), yuv_tracks, am, check=False), YUV420P, False),
        "chain_to_yuv": (lambda s, s2, k: ops.chain_to_yuv(prm(True), sink(k), sink_tracks, am, check=False), None, True),
        "chain_yuv420p_to_yuv": (lambda s, s2, k: ops.chain_yuv420p_to_yuv(prm(True), src(s), sink(k), yuv_sink_tracks, am, check=False), YUV420P, True),
        "chain_flat_yuv420p": (lambda s, s2, k: ops.chain_flat_yuv420p(prm(False), src(s), yuv_tracks, am, check=False), YUV420P, False),
        "chain_flat_yuv420p_to_yuv": (lambda s, s2, k: ops.chain_flat_yuv420p_to_yuv(prm(False), src(s), sink(k), yuv_sink_tracks, am, check=False), YUV420P, True),
        "chain_flat_yuv420p_mix": (lambda s, s2, k: ops.chain_flat_yuv420p_mix(prm(False), src(s), src(s2), mix_tracks, am, sink=None, check=False), YUV420P, False),
        "chain_flat_yuv420p_mix+sink": (lambda s, s2, k: ops.chain_flat_yuv420p_mix(prm(False), src(s), src(s2), mix_tracks, am, sink=sink(k), check=False), YUV420P, True),
        "chain_flat_yuv422:yuv422p": (lambda s, s2, k: ops.chain_flat_yuv422(prm(False), src422(YUV422P, s), yuv_sink_tracks, am, check=False), YUV422P, False),
        "chain_flat_yuv422:yuv422p+sink": (lambda s, s2, k: ops.chain_flat_yuv422(prm(False), src422(YUV422P, s), yuv_sink_tracks, am, sink=sink(k), check=False), YUV422P, True),
        "chain_flat_yuv422:uyvy": (lambda s, s2, k: ops.chain_flat_yuv422(prm(False), src422(UYVY, s), packed_tracks, am, check=False), UYVY, False),
    }


def sink_width(name):
    return W if "flat" in name else W // 2


def run(ops, b, name, call, s, s2, k, want, what, failures):
    """one call: its code against `want`, and every destination plane still as it was"""
    import torch
    from lives_amd import lib
    rc = call(s, s2, k)
    torch.cuda.synchronize()
    if rc != want:
        failures.append("%s, %s: %d, expected %d (%s)" % (what, name, rc, want, lib.load().lgpu_last_error()))
    if not all(bool((p == FILL).all()) for d in b["D"] for p in d):
        failures.append("%s, %s: a destination plane was written" % (what, name))
        for d in b["D"]:
            for p in d:
                p.fill_(FILL)


def good_calls(ops, b, eps):
    """every entry point takes the descriptions the rows start from"""
    import torch
    for name, (call, fmt, takes_sink) in eps.items():
        s = base_source(fmt) if fmt is not None else None
        rc = call(s, base_source(YUV420P), base_sink(sink_width(name)) if takes_sink else None)
        torch.cuda.synchronize()
        assert rc == 0, "%s refuses the good descriptions: %d" % (name, rc)
        assert not all(bool((p == FILL).all()) for d in b["D"] for p in d), "%s wrote nothing" % name
        for d in b["D"]:
            for p in d:
                p.fill_(FILL)


def _set(**kw):
    return lambda d: d.update(kw)


def _short(key, idx=None):
    def f(d):
        if idx is None:
            d[key] -= 1
        else:
            d[key][idx] -= 1
    return f


# (what, the change to a good description, the source formats the row applies to)
BAD_SOURCES = [
    ("out_order 2", _set(out_order=2), (YUV420P, YUV422P, UYVY)),
    ("which_tables 4", _set(which_tables=4), (YUV420P, YUV422P, UYVY)),
    ("pb_quality 0", _set(pb_quality=0), (YUV420P, YUV422P, UYVY)),
    ("pb_quality 4", _set(pb_quality=4), (YUV420P, YUV422P, UYVY)),
    ("an unknown flag bit", _set(flags=2), (YUV420P,)),                      # (lgpu_yuv422_source has no flags)
    ("luma rowstride one byte short", _short("strides", 0), (YUV420P, YUV422P, UYVY)),
    ("chroma rowstride one byte short", _short("strides", 1), (YUV420P, YUV422P)),
    ("u_size one byte short", _short("u_size"), (YUV420P, YUV422P)),
    ("v_size one byte short", _short("v_size"), (YUV420P, YUV422P)),
]

# (what, the change to a good 4:2:0 sink of the entry point's width, entry points with a YUV source only)
BAD_SINKS = [
    ("out_fmt 1", _set(out_fmt=1), False),
    ("out_fmt 6", _set(out_fmt=6), False),
    ("in_order 2", _set(in_order=2), False),
    ("which_tables 4", _set(which_tables=4), False),
    ("which_tables 2 with UYVY", lambda k: k.update(out_fmt=UYVY, which_tables=2, orow=[k["orow"][0] * 2, 0, 0]), False),
    ("in_order opposite to the chain's result", _set(in_order=1), True),
    ("luma rowstride one byte short", _short("orow", 0), False),
    ("packed rowstride one byte short", lambda k: k.update(out_fmt=UYVY, orow=[k["orow"][0] * 2 - 1, 0, 0]), False),
    ("chroma rowstride one byte short", _short("orow", 2), False),
]


@pytest.mark.gpu
def test_bad_source_descriptions(gpu, bufs):
    eps = entry_points(gpu, bufs)
    good_calls(gpu, bufs, eps)
    failures = []
    for what, change, fmts in BAD_SOURCES:
        for name, (call, fmt, takes_sink) in eps.items():
            if fmt not in fmts:
                continue
            k = base_sink(sink_width(name)) if takes_sink else None
            bad = base_source(fmt)
            change(bad)
            run(gpu, bufs, name, call, bad, base_source(YUV420P), k, EXPECT.get((what, name), E_BADARG), what, failures)
            if "mix" in name:
                bad2 = base_source(YUV420P)
                change(bad2)
                run(gpu, bufs, name + " (src2)", call, base_source(fmt), bad2, k, EXPECT.get((what, name + " (src2)"), E_BADARG), what, failures)
    assert not failures, "\n".join(failures)


@pytest.mark.gpu
def test_bad_sink_descriptions(gpu, bufs):
    eps = entry_points(gpu, bufs)
    good_calls(gpu, bufs, eps)
    failures = []
    for what, change, yuv_source_only in BAD_SINKS:
        for name, (call, fmt, takes_sink) in eps.items():
            if not takes_sink or (yuv_source_only and fmt is None):
                continue
            k = base_sink(sink_width(name))
            change(k)
            run(gpu, bufs, name, call, base_source(fmt) if fmt is not None else None, base_source(YUV420P), k, EXPECT.get((what, name), E_BADARG), what, failures)
    assert not failures, "\n".join(failures)
