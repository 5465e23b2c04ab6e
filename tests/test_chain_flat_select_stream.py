"""lgpu_chain_flat_yuv_select's stream contract (include/lives_gpu_select.h): the call is ordered behind the work in front of it on a busy non-default stream and
does not wait once warm; captured into a graph after a warm-up and replayed twice over changed inputs it gives the eager call's bytes -- the oracle's -- each time.
The proxies are tests/stream_order.py's and tests/graph_replay.py's, the runner and the case are tests/test_chain_flat_select.py's: UYVY over YUV420P, iris circle,
to YUV420P, 3 tracks, at 66x10 -- the 4:2:0 sink refuses an odd height, so the 66x9 shape goes to the second case: one dissolve to RGBA under capture, because the
mask pointers are kernel arguments."""
import pytest

from tests import graph_replay as gr
from tests import stream_order as so
from tests.test_chain_flat_mix422 import UYVY, YUV420P, layer
from tests.test_chain_flat_select import CIRCLE, DISSOLVE, run, spec, with_lut

NAME = "chain_flat_yuv_select"


def the_case(orc, kind):
    return with_lut(orc, spec(orc, [0x57E, kind], (YUV420P, UYVY), 66, 10 if kind == CIRCLE else 9, kind, YUV420P if kind == CIRCLE else 0, ntracks=3, L1=layer(wt=1, pad=(2, 1, 3)),
                              L2=layer(pad=(4, 0, 0)), lut="gamma", swap=1, wt_sink=2, yvu_sink=True))


def test_the_case_is_what_the_docstring_says(orc):
    """no GPU: 66 wide, three tracks, UYVY over YUV420P; the circle goes to the 4:2:0 sink (which wants an even height: 66x10), the dissolve to RGBA at 66x9"""
    for kind, fmt, sh in ((CIRCLE, YUV420P, 10), (DISSOLVE, 0, 9)):
        s = the_case(orc, kind)
        c = s["c"]
        assert (c["f1"], c["f2"], c["sw"], c["sh"], c["ntracks"], s["fmt"], s["kind"]) == (YUV420P, UYVY, 66, sh, 3, fmt, kind)
        assert len(set(s["amounts"])) == 3 and all(0. < a < 1. for a in s["amounts"])


@pytest.mark.gpu
def test_select_on_a_busy_stream(gpu, orc):
    """the call is made behind 20 ms of work on a side stream that the default stream overtakes, over inputs that are complemented until that work is over: it must
    return while the stream is busy, and its result must be the oracle's (run()'s own comparison)"""
    px = so.StreamProxy(gpu, so.side_stream())
    run(px, orc, the_case(orc, CIRCLE))
    calls = px.finish()
    assert [c.name for c in calls] == [NAME] and not calls[0].waited


@pytest.mark.gpu
def test_select_captured_and_replayed(gpu, orc):
    """the circle case, then the dissolve case: after a warm-up the call allocates nothing (the allocator probe) and captures; nothing runs during the capture; the graph
    is replayed twice over inputs that were put back in between, with the caller's host arrays complemented, and run()'s comparison with the oracle judges the last
    replay"""
    for kind in (CIRCLE, DISSOLVE):
        px = gr.GraphProxy(gpu, so.side_stream())
        run(px, orc, the_case(orc, kind))
        assert px.finish() == [NAME] and px.graphs == 1 and not px.flagged and not px.eager, kind
