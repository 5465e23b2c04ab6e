"""lgpu_chain_flat_yuv_luma's stream contract (include/lives_gpu_luma.h): the call is ordered behind the work in front of it on a busy non-default stream and does
not wait once warm; captured into a graph after a warm-up and replayed twice over changed inputs it gives the eager call's bytes -- the oracle's -- each time.  The
proxies are tests/stream_order.py's and tests/graph_replay.py's, the runner and the case are tests/test_chain_flat_luma.py's: UYVY over YUV420P, 3 tracks with distinct
thresholds, at 66x10 -- the negative overlay to YUV420P, and the underlay (the layers change places on the host) to RGBA at 66x9.  The thresholds are a host array of
the caller's and travel in the kernel's arguments: the replay must not read them again."""
import pytest

from tests import graph_replay as gr
from tests import stream_order as so
from tests.test_chain_flat_mix422 import UYVY, YUV420P, layer
from tests.test_chain_flat_luma import NEGATIVE, UNDERLAY, run, spec, with_lut

NAME = "chain_flat_yuv_luma"


def the_case(orc, type_):
    return with_lut(orc, spec(orc, [0x57F, type_], (YUV420P, UYVY), 66, 10 if type_ == NEGATIVE else 9, type_, YUV420P if type_ == NEGATIVE else 0, ntracks=3,
                              L1=layer(wt=1, pad=(2, 1, 3)), L2=layer(pad=(4, 0, 0)), lut="gamma", swap=1, wt_sink=2, yvu_sink=True))


def test_the_case_is_what_the_docstring_says(orc):
    """no GPU: 66 wide, three tracks, UYVY over YUV420P; the negative overlay goes to the 4:2:0 sink (which wants an even height: 66x10), the underlay to RGBA at 66x9"""
    for type_, fmt, sh in ((NEGATIVE, YUV420P, 10), (UNDERLAY, 0, 9)):
        s = the_case(orc, type_)
        c = s["c"]
        assert (c["f1"], c["f2"], c["sw"], c["sh"], c["ntracks"], s["fmt"], s["type"]) == (YUV420P, UYVY, 66, sh, 3, fmt, type_)
        assert len(set(s["thresholds"])) == 3 and all(1 <= t <= 255 for t in s["thresholds"])


@pytest.mark.gpu
def test_luma_on_a_busy_stream_then_captured_and_replayed(gpu, orc):
    """Busy stream: the call is made behind 20 ms of work on a side stream that the default stream overtakes, over inputs that are complemented until that work is
    over: it must return while the stream is busy, and its result must be the oracle's (run()'s own comparison).  Then capture and replay (captured_and_replayed)"""
    px = so.StreamProxy(gpu, so.side_stream())
    run(px, orc, the_case(orc, NEGATIVE))
    calls = px.finish()
    assert [c.name for c in calls] == [NAME] and not calls[0].waited
    captured_and_replayed(gpu, orc)


def captured_and_replayed(gpu, orc):
    """the second half of the test above.  The negative overlay, then the underlay: after a warm-up the call allocates nothing (the allocator probe) and captures;
    nothing runs during the capture; the graph is replayed twice over inputs that were put back in between, with the caller's host arrays complemented, and run()'s
    comparison with the oracle judges the last replay"""
    for type_ in (NEGATIVE, UNDERLAY):
        px = gr.GraphProxy(gpu, so.side_stream())
        run(px, orc, the_case(orc, type_))
        assert px.finish() == [NAME] and px.graphs == 1 and not px.flagged and not px.eager, type_
