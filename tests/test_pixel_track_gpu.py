"""-m gpu: the device pixel tracker (ops.track_pixels, csrc/pixtrack_kernels.hpp; vdet.track.pixel_tracker) against
tests/pixtrack_spec.py ON BITS: the NaN masks are equal and every other element has the same bit pattern.  The spec is all
integer but for one f32 division and one f32 subtraction per step, so nothing is left to a tolerance.
  f. one call over a [3,5] slot table that mixes every kind of slot, for four (grid, radius) pairs;
  g. step and max_frames, and interpolate_tracks on the result;  h. min_conf, with a confidence equal to the threshold;
  i. invalid anchor data (latched, the slot written as an empty one);  j. argument errors;  k. the context's prep cache;
  l. top_anchors -> track_pixels -> rescore_tubelets -> nms_tracks;  m. the dict level."""
import numpy as np
import pytest

import pixtrack_cases as pc
import pixtrack_harness as ph
import pixtrack_spec as px
from pixtrack_cases import FM, HM, LEAVES, WM, mixed_case
from pixtrack_harness import assert_spec, bits_equal, g

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------------------------
# f. the mixed slot table (pixtrack_cases.mixed_case)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,R", ((8, 2), (32, 8), (64, 16), (12, 3)))
def test_mixed_slot_table(S, R):
    images, fr, bx, sc, pos, (w, h) = mixed_case(S, R)
    tracks, anchors, nt, _ = assert_spec(images, fr, bx, sc, grid=S, radius=R, min_conf=0.0)
    assert nt.tolist() == [4, 5, 3]
    # the case is what it says: the planted mover is followed exactly from every one of its three anchors ...
    for c, t in ((0, 1), (2, 1), (2, 2)):
        assert np.array_equal(tracks[c, t], pc.rows_from_positions(pos, w, h, range(FM))), (c, t)
    # ... every live slot walks (min_conf = 0: only the video's ends and the image's edges stop a chain) ...
    live = np.isfinite(tracks[..., 0])
    assert live[fr > 0].sum(axis=-1).min() >= 2 and not live[fr == 0].any()
    # ... and the leaver's chain ends because its box is wholly outside, before the video does
    assert live[2, 0].tolist() == [True] * LEAVES + [False] * (FM - LEAVES) and (tracks[2, 0, :LEAVES, 4] == 1).all()
    # the default threshold is a second call: the noise slots stop early, the bits still agree
    assert_spec(images, fr, bx, None, grid=S, radius=R)


def test_larger_image_and_default_settings():
    """240 x 200: more rows than columns, the default grid 32 / radius 8, a 64 x 96 mover."""
    images, pos = pc.planted_video(3300, 8, 240, 200, 64, 96, 32, 8, 4)
    x, y = pos[4]
    fr = np.array([[5, 1], [0, 8]], np.int32)
    bx = np.array([[[x + 1, y + 1, x + 64, y + 96], [150, 200, 230, 260]], [[0, 0, 0, 0], [-40, -10, 30.5, 90]]], np.float32)
    tracks, _, nt, _ = assert_spec(images, fr, bx)
    assert nt.tolist() == [2, 2]
    assert np.array_equal(tracks[0, 0], pc.rows_from_positions(pos, 64, 96, range(8)))


# ---------------------------------------------------------------------------------------------------------------------
# g. step and max_frames
# ---------------------------------------------------------------------------------------------------------------------
def test_step_and_max_frames_then_interpolation():
    import torch
    from vdetlib_amd import ops
    images, fr, bx, sc, pos, _ = mixed_case(8, 2)
    for mf in (0, 5, 6):
        tracks, anchors, nt, _ = assert_spec(images, fr, bx, sc, grid=8, radius=2, min_conf=0.0, max_frames=mf, step=3)
        live = np.isfinite(tracks[..., 0])
        reach = px.reach_of(mf, FM)
        for c in range(3):
            for t in range(5):
                f0 = int(fr[c, t]) - 1
                on = np.flatnonzero(live[c, t])
                assert all((f - f0) % 3 == 0 and abs(f - f0) // 3 <= reach for f in on), (mf, c, t)
        # anchored on the last frame, index 11: 8, 5, 2 are in reach; max_frames = 5 allows ceil(6/2) - 1 = 2 steps, 6 allows 3
        assert np.flatnonzero(live[2, 1]).tolist() == ([5, 8, 11] if mf == 5 else [2, 5, 8, 11])
    # the strided result goes into interpolate_tracks as it is: rows on the visited frames, the dense axis between them
    tracks, anchors, nt, _ = px.track_pixels(images, fr, bx, sc, 8, 2, 0.0, 0, 3)
    from vdetlib_amd import ops
    out = ops.track_pixels(g(images), g(fr), g(bx), g(sc), grid=8, radius=2, min_conf=0.0, step=3)
    dense = ops.interpolate_tracks(out[0], out[2], out[1], [])
    dt = dense['tracks'].cpu().numpy()
    assert dt.shape == tracks.shape
    on = np.isfinite(tracks[..., 0])
    assert bits_equal(dt[on], tracks[on])
    filled = np.isfinite(dt[0, 1, :, 0])
    assert filled[0:10].all() and not filled[10:].any()           # between the first and the last visited frame
    assert torch.equal(dense['ntracks'].cpu(), torch.from_numpy(nt))


# ---------------------------------------------------------------------------------------------------------------------
# h. min_conf
# ---------------------------------------------------------------------------------------------------------------------
def test_min_conf_stops_where_the_object_vanishes():
    S, R, w, h = 16, 4, 16, 32
    images, pos = pc.planted_video(2000 + S, 10, 64, 48, w, h, S, R, 3, vanish_from=7)
    x, y = pos[3]
    fr, bx = np.array([[4]], np.int32), np.array([[[x + 1, y + 1, x + w, y + h]]], np.float32)
    free = assert_spec(images, fr, bx, grid=S, radius=R, min_conf=0.0)[0][0, 0]
    assert free[7, 4] < 0.9 and np.isfinite(free).all()           # the precondition; min_conf <= 0 never stops
    assert bits_equal(assert_spec(images, fr, bx, grid=S, radius=R, min_conf=-1.0)[0][0, 0], free)
    tracks = assert_spec(images, fr, bx, grid=S, radius=R, min_conf=0.9)[0][0, 0]
    assert np.array_equal(tracks, pc.rows_from_positions(pos, w, h, range(7)), equal_nan=True)


def test_confidence_equal_to_the_threshold_goes_on():
    """A flat image; on the second frame one pixel inside the box is 51 brighter.  The 8 x 8 box has pitch 1 and every
    candidate's window holds that pixel once: SAD 51 everywhere, (0,0) wins, conf = 1 - 51/16320 in f32."""
    images = np.full((3, 32, 40, 3), 100, np.uint8)
    images[1, 14, 15] = 151
    images[2, 14, 15] = 152
    fr, bx = np.array([[1]], np.int32), np.array([[[12, 11, 19, 18]]], np.float32)
    c51 = np.float32(1.0) - np.float32(51) / np.float32(255 * 64)
    c52 = np.float32(1.0) - np.float32(52) / np.float32(255 * 64)
    assert c52 < c51
    row = lambda c: np.array([12, 11, 19, 18, c], np.float32)
    tracks = assert_spec(images, fr, bx, grid=8, radius=2, min_conf=float(c51))[0][0, 0]
    assert bits_equal(tracks[0], row(1.0)) and bits_equal(tracks[1], row(c51)) and np.isnan(tracks[2]).all()
    tracks = assert_spec(images, fr, bx, grid=8, radius=2, min_conf=float(c52))[0][0, 0]
    assert bits_equal(tracks[2], row(c52))
    tracks = assert_spec(images, fr, bx, grid=8, radius=2, min_conf=float(np.nextafter(c51, np.float32(2))))[0][0, 0]
    assert np.isnan(tracks[1:]).all()


# ---------------------------------------------------------------------------------------------------------------------
# i. invalid anchor data
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(ph.BAD_SLOTS)))
def test_invalid_anchor_data_is_latched(k):
    ph.invalid_anchor_data_is_latched('track_pixels', k, 3400, grid=8, radius=2)


# ---------------------------------------------------------------------------------------------------------------------
# j. argument errors
# ---------------------------------------------------------------------------------------------------------------------
def test_argument_errors():
    from vdetlib_amd import _lib, ops
    images, fr, bx, sc, _, _ = mixed_case(8, 2)
    ti, tf, tb, ts = g(images), g(fr), g(bx), g(sc)
    cx = _lib.Context()
    try:
        cx.set_timing(2)
        bad = [lambda: ops.track_pixels(ti[:, :, ::2], tf, tb, ctx=cx),                      # not contiguous
               lambda: ops.track_pixels(ti.float(), tf, tb, ctx=cx),
               lambda: ops.track_pixels(ti[0], tf, tb, ctx=cx),
               lambda: ops.track_pixels(ti, tf, tb, grid=6, ctx=cx),
               lambda: ops.track_pixels(ti, tf, tb, grid=68, ctx=cx),
               lambda: ops.track_pixels(ti, tf, tb, grid=0, ctx=cx),
               lambda: ops.track_pixels(ti, tf, tb, radius=0, ctx=cx),
               lambda: ops.track_pixels(ti, tf, tb, radius=17, ctx=cx),
               lambda: ops.track_pixels(ti, tf, tb, step=0, ctx=cx),
               lambda: ops.track_pixels(ti, tf, tb, max_frames=-1, ctx=cx),
               lambda: ops.track_pixels(ti, tf, tb, min_conf=float('nan'), ctx=cx),
               lambda: ops.track_pixels(ti, tf, tb, min_conf=float('inf'), ctx=cx),
               lambda: ops.track_pixels(ti.cpu(), tf, tb, ctx=cx),                           # tensors on the host
               lambda: ops.track_pixels(ti, tf.cpu(), tb, ctx=cx),
               lambda: ops.track_pixels(ti, tf, tb.cpu(), ctx=cx),
               lambda: ops.track_pixels(ti, tf, tb, ts.cpu(), ctx=cx),
               lambda: ops.track_pixels(ti, tf.long(), tb, ctx=cx),
               lambda: ops.track_pixels(ti, tf, tb.double(), ctx=cx),
               lambda: ops.track_pixels(ti, tf, tb[:, :4], ctx=cx),
               lambda: ops.track_pixels(ti, tf, tb, ts[:2], ctx=cx)]
        for k, fn in enumerate(bad):
            with pytest.raises(ValueError):
                fn()
                pytest.fail("case %d raised nothing" % k)
        assert sum(n for _, n in cx.last_timing().values()) == 0, "an argument error launched a kernel"
        # the C-ABI refuses the same settings on its own
        L, z = cx.lib, None
        p = (ti.data_ptr(), FM, HM, WM, tf.data_ptr(), tb.data_ptr(), z, 3, 5)
        o = tuple(x.data_ptr() for x in (ti, ti, ti))       # (never written: every call below is refused)
        for S, R, mc, mf, st in ((6, 2, .5, 0, 1), (68, 2, .5, 0, 1), (8, 0, .5, 0, 1), (8, 17, .5, 0, 1), (8, 2, .5, 0, 0),
                                 (8, 2, .5, -1, 1), (8, 2, float('nan'), 0, 1)):
            assert L.vdet_track_pixels(cx.h, *p, S, R, mc, mf, st, *o) == _lib.VDET_EINVAL, (S, R, mc, mf, st)
        assert L.vdet_track_pixels(cx.h, ti.data_ptr(), FM, 32768, WM, *p[4:], 8, 2, .5, 0, 1, *o) == _lib.VDET_EINVAL
        out = ops.track_pixels(ti, tf, tb, ts, grid=8, radius=2, ctx=cx)                     # the context still works
        assert cx.last_timing()['other'][1] == 1                                             # ONE launch, timed under 'other'
        want = px.track_pixels(images, fr, bx, sc, 8, 2)
        for a, b in zip(out, want[:3]):
            assert bits_equal(a.cpu().numpy(), b)
    finally:
        cx.close()


# ---------------------------------------------------------------------------------------------------------------------
# k. the prep cache
# ---------------------------------------------------------------------------------------------------------------------
def test_prep_cache_is_left_alone():
    import synth
    import torch
    from vdetlib_amd import _lib, ops
    boxes, scores = synth.coherent_video(7433, 12, 120, 3, frac=True)
    tb, ts = g(boxes), g(scores)
    images, fr, bx, sc, _, _ = mixed_case(8, 2)
    cx = _lib.Context(torch.cuda.current_device())
    try:
        cx.set_cache(True)
        run = lambda: tuple(x.cpu().numpy() for x in ops.nms_track_volume(tb, ts, max_tracks=4, ctx=cx))
        first = run()
        mine = ops.track_pixels(g(images), g(fr), g(bx), g(sc), grid=8, radius=2, ctx=cx)
        second = run()
    finally:
        cx.close()
    for a, b in zip(first, second):
        assert a.shape == b.shape and np.array_equal(a, b, equal_nan=True)
    want = px.track_pixels(images, fr, bx, sc, 8, 2)
    for a, b in zip(mine, want[:3]):
        assert bits_equal(a.cpu().numpy(), b)


# ---------------------------------------------------------------------------------------------------------------------
# l. downstream
# ---------------------------------------------------------------------------------------------------------------------
def test_downstream_from_top_anchors_to_nms_tracks():
    import rescore_spec
    from vdetlib_amd import ops
    S, R, w, h, F, B, C, T = 8, 2, 16, 8, 8, 6, 2, 2
    images, pos = pc.planted_video(3500, F, 48, 64, w, h, S, R, 4)
    rng = np.random.RandomState(3501)
    boxes = np.zeros((F, B, 4), np.float32)
    x1 = rng.randint(1, 40, size=(F, B))
    y1 = rng.randint(1, 30, size=(F, B))
    boxes[..., 0], boxes[..., 1] = x1, y1
    boxes[..., 2], boxes[..., 3] = x1 + rng.randint(6, 20, size=(F, B)), y1 + rng.randint(6, 16, size=(F, B))
    boxes[:, 0] = [(x + 1, y + 1, x + w, y + h) for x, y in pos]             # proposal 0 is the planted object
    scores = rng.rand(F, B, C).astype(np.float32)
    scores[4, 0, 0] = 2.0                                                     # class 0's first anchor: the object on frame 5
    tb, ts = g(boxes), g(scores)
    fr, ab, asc, _ = ops.top_anchors(tb, ts, T)
    tracks, anchors, nt = ops.track_pixels(g(images), fr, ab, asc, grid=S, radius=R, min_conf=0.0)
    want = px.track_pixels(images, fr.cpu().numpy(), ab.cpu().numpy(), asc.cpu().numpy(), S, R, 0.0)
    for a, b in zip((tracks, anchors, nt), want[:3]):
        assert bits_equal(a.cpu().numpy(), b)
    assert np.array_equal(want[0][0, 0], pc.rows_from_positions(pos, w, h, range(F))) and want[2].tolist() == [T, T]
    det, pooled, tboxes, src = ops.rescore_tubelets(tracks, nt, tb, ts, complete=False)
    wd, wp, wb, ws, _ = rescore_spec.spec(want[0], want[2], boxes, scores, complete=False)
    for a, b in ((det, wd), (pooled, wp), (tboxes, wb), (src, ws)):
        assert bits_equal(a.cpu().numpy(), b)
    assert (ws[0, 0] == 0).all()                                              # every box of the object's tubelet hits proposal 0
    out = ops.nms_tracks(tracks, nt, pooled, tboxes)
    assert tuple(out['tracks'].shape) == (C, T, F, 5) and int(out['cnt'].min()) >= 1


# ---------------------------------------------------------------------------------------------------------------------
# m. the dict level
# ---------------------------------------------------------------------------------------------------------------------
class Opts(object):
    def __init__(self, **kw):
        self.__dict__.update(kw)


def test_pixel_tracker_is_a_track_method():
    from vdetlib_amd.utils.protocol import tracks_proto_from_boxes
    from vdetlib_amd.vdet import track
    S, R, w, h, F = 8, 2, 16, 8, 9
    images, pos = pc.planted_video(3600, F, 48, 64, w, h, S, R, 4)
    vid = {'video': 'pixvid', 'root_path': '/nowhere', 'frames': [{'frame': f + 1, 'path': '%04d.JPEG' % f} for f in range(F)]}
    reads = []

    def reader(path):
        reads.append(path)
        return images[int(path.split('/')[-1].split('.')[0])]

    x, y = pos[4]
    obj = [x + 1, y + 1, x + w, y + h]
    other = [40, 30, 55, 37] if x < 20 else [3, 30, 18, 37]
    det_info = np.array([[5] + obj + [0.9, 0.1], [3] + other + [0.8, 0.2], [5] + [v + 1 for v in obj] + [0.7, 0.3]], np.float64)
    opts = Opts(step=2, max_frames=None, max_tracks=5, thres=0.5, nms_thres=0.3, grid=S, radius=R, min_conf=0.0)
    saved = track.imread
    track._pixel_video.clear()
    try:
        track.imread = reader
        got = track.greedily_track_from_raw_dets(vid, det_info, track.pixel_tracker, 1, opts)
        assert len(reads) == F and reads[0] == '/nowhere/0000.JPEG'          # one upload for both anchors
        assert track.pixel_tracker.__name__ == got['method'] == 'pixel_tracker' and got['video'] == 'pixvid'
        lumas = px.luma(images)
        want = []
        for frame, box in ((5, obj), (3, other)):          # the third detection lies on the first track: suppressed, no anchor
            rows = px.track_slot(lumas, frame, tuple(int(v) - 1 for v in box), S, R, 0.0, 0, 2)
            on = np.flatnonzero(np.isfinite(rows[:, 0]))
            assert np.array_equal(on, np.arange(on[0], on[-1] + 1, 2)) and len(on) >= 4
            want.extend(tracks_proto_from_boxes(rows[on], 'pixvid', frame, int(on[0]) + 1, 2))
        assert got['tracks'] == want
        assert [b['frame'] for b in got['tracks'][0]] == [1, 3, 5, 7, 9] and [b['anchor'] for b in got['tracks'][0]] == [-4, -2, 0, 2, 4]
        # max_frames as fcn_tracker reads it, and greedily_track_from_det / track_from_det take the same track_method
        opts.max_frames = 3
        one = track.pixel_tracker(vid, 5, obj, opts)
        assert [b['frame'] for b in one[0]] == [3, 5, 7] and len(reads) == F
    finally:
        track.imread = saved
        track._pixel_video.clear()
