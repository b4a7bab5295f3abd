"""-m gpu: the pixel tracker's scale search on the device (ops.track_pixels_scaled, ops.track_volume_pixels_scaled;
csrc/pixtrack_kernels.hpp) against tests/pixtrack_spec.py ON BITS: the NaN masks are equal and every other element has
the same bit pattern.  The rule is all integer but for one f32 division and one f32 subtraction per step.
  a. scales = 0 against ops.track_pixels;  b. a [3,5] slot table that mixes every kind of slot, four (grid, radius) pairs x four
  scale settings;  c. a tie on every key;  d. step and max_frames, interpolate_tracks;  e. invalid anchor data;  f. argument
  errors;  g. the context's prep cache;  h. top_anchors -> track_pixels_scaled -> rescore_tubelets -> nms_tracks;
  i. the greedy form and the dict level."""
import numpy as np
import pytest

import pixtrack_harness as ph
import pixtrack_scale_cases as sc
import pixtrack_spec as px
from pixtrack_harness import assert_same, assert_spec, bits_equal, device, g, greedy_device, host

pytestmark = pytest.mark.gpu


# a. -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", (dict(min_conf=0.0), dict(), dict(min_conf=0.0, step=2, max_frames=7)))
def test_no_levels_equals_the_fixed_scale_call(kw):
    from vdetlib_amd import ops
    images, fr, bx, scr, _ = sc.mixed_case(8, 2)
    want = tuple(x.cpu().numpy() for x in ops.track_pixels(g(images), g(fr), g(bx), g(scr), grid=8, radius=2, **kw))
    assert_same(device(images, fr, bx, scr, grid=8, radius=2, scales=0, scale_step=25, scale_penalty=65535, **kw), want)
    assert_same(want, px.track_pixels(images, fr, bx, scr, 8, 2, **kw))


# b. -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scales,scale_step,scale_penalty", ((1, 5, 0), (2, 5, 0), (3, 25, 0), (1, 10, 64)))
@pytest.mark.parametrize("S,R", ((8, 2), (32, 8), (64, 16), (12, 3)))
def test_mixed_slot_table(S, R, scales, scale_step, scale_penalty):
    images, fr, bx, scr, truth = sc.mixed_case(S, R)
    kw = dict(grid=S, radius=R, scales=scales, scale_step=scale_step, scale_penalty=scale_penalty)
    tracks, anchors, nt, _ = assert_spec(images, fr, bx, scr, min_conf=0.0, **kw)
    assert nt.tolist() == [4, 5, 3]
    # the case is what it says: every live slot walks (min_conf = 0: only the video's ends and the image's edges stop a chain),
    # no empty slot has a row ...
    live = np.isfinite(tracks[..., 0])
    assert live[fr > 0].sum(axis=-1).min() >= 2 and not live[fr == 0].any()
    # ... the first-frame and the last-frame anchors run the whole video in one direction ...
    assert live[0, 1].all() and live[0, 2].all()
    # ... the boxes do change size ...
    wid = tracks[..., 2] - tracks[..., 0]
    assert np.nanmax(wid[0, 1]) > wid[0, 1, 0] and np.nanmax(wid[0, 2]) > wid[0, 2, sc.F - 1]
    # ... and the leaver's chain ends because its box is wholly outside, before the video does
    assert live[2, 0].tolist() == [True] * sc.LEAVES + [False] * (sc.F - sc.LEAVES)
    if (S, R) == (32, 8) and (scales, scale_step, scale_penalty) == (1, 5, 0):
        # the setting of the planted scene: the growing and the shrinking object are followed (test_pixel_track_scaled_cpu.py)
        assert sc.largest_error(tracks[0, 1], truth['grow']) <= 4 and sc.largest_error(tracks[0, 2], truth['shrink']) <= 4


def test_default_settings():
    """grid 32, radius 8, min_conf 0.5, scales 1, scale_step 5, no scores: the call with nothing but the data"""
    from vdetlib_amd import ops
    images, fr, bx, _, _ = sc.mixed_case(32, 8)
    want = px.track_pixels(images, fr, bx, scales=1, scale_step=5, scale_penalty=0)
    assert not want[3]
    assert_same(host(ops.track_pixels_scaled(g(images), g(fr), g(bx))), want)
    tracks = want[0]
    assert np.isfinite(tracks[0, 1:4, :, 0]).all()


# c. -------------------------------------------------------------------------------------------------------------------
def test_every_key_ties_on_sad():
    """A flat video; on the ANCHOR frame one pixel inside the 8 x 8 box is 51 brighter, so the template has one cell of 151 and
    every window of every level on every other frame has SAD 51: level 0 and shift 0 win, the box never moves or changes size
    (at scale_step = 25 the levels are 2, 4, 6, 8, 10, 12 and 14 wide), conf = 1 - 51/16320 in f32."""
    F = 4
    images = np.full((F, 32, 40, 3), 100, np.uint8)
    images[1, 14, 15] = 151
    fr, bx = np.array([[2]], np.int32), np.array([[[12, 11, 19, 18]]], np.float32)
    c51 = np.float32(1.0) - np.float32(51) / np.float32(255 * 64)
    want = np.tile(np.array([12, 11, 19, 18, c51], np.float32), (F, 1))
    want[1, 4] = 1.0
    for q in (0, 7):
        kw = dict(grid=8, radius=2, scales=3, scale_step=25, scale_penalty=q)
        tracks = assert_spec(images, fr, bx, min_conf=float(c51), **kw)[0][0, 0]          # conf == min_conf: the chain goes on
        assert bits_equal(tracks, want)
        tracks = assert_spec(images, fr, bx, min_conf=float(np.nextafter(c51, np.float32(2))), **kw)[0][0, 0]
        assert bits_equal(tracks[1], want[1]) and np.isnan(tracks[[0, 2, 3]]).all()
    # the bright pixel on the NEXT frame instead, levels that collapse onto the box itself (scale_step = 5 on 8 pixels): the
    # three levels tie on every shift; level 0, shift 0
    images = np.full((3, 32, 40, 3), 100, np.uint8)
    images[1, 14, 15] = 151
    fr = np.array([[1]], np.int32)
    tracks = assert_spec(images, fr, bx, grid=8, radius=2, scales=1, scale_step=5, min_conf=float(c51))[0][0, 0]
    assert bits_equal(tracks, np.array([[12, 11, 19, 18, 1], [12, 11, 19, 18, c51], [12, 11, 19, 18, 1]], np.float32))


# d. -------------------------------------------------------------------------------------------------------------------
def test_step_and_max_frames_then_interpolation():
    import torch
    from vdetlib_amd import ops
    images, fr, bx, scr, _ = sc.mixed_case(8, 2)
    kw = dict(grid=8, radius=2, min_conf=0.0, scales=1, scale_step=10)
    for mf in (0, 5, 6):
        tracks, anchors, nt, _ = assert_spec(images, fr, bx, scr, max_frames=mf, step=3, **kw)
        live = np.isfinite(tracks[..., 0])
        reach = px.reach_of(mf, sc.F)
        for c in range(3):
            for t in range(5):
                f0 = int(fr[c, t]) - 1
                assert all((f - f0) % 3 == 0 and abs(f - f0) // 3 <= reach for f in np.flatnonzero(live[c, t])), (mf, c, t)
        # anchored on the last frame, index 11: 8, 5, 2 are in reach; max_frames = 5 allows ceil(6/2) - 1 = 2 steps, 6 allows 3
        assert np.flatnonzero(live[0, 2]).tolist() == ([5, 8, 11] if mf == 5 else [2, 5, 8, 11])
    tracks, anchors, nt, _ = px.track_pixels(images, fr, bx, scr, step=3, **kw)
    out = ops.track_pixels_scaled(g(images), g(fr), g(bx), g(scr), step=3, **kw)
    dense = ops.interpolate_tracks(out[0], out[2], out[1], [])
    dt = dense['tracks'].cpu().numpy()
    on = np.isfinite(tracks[..., 0])
    assert dt.shape == tracks.shape and bits_equal(dt[on], tracks[on])
    for c in range(3):
        for t in range(5):                    # hole-free between the chain ends, empty beyond them
            ends = np.flatnonzero(on[c, t])
            want = np.zeros(sc.F, bool)
            if len(ends) >= 2:                # (vdet_interp_tracks' end rule: a first knot on frame 2 reaches frame 1, a last one on F - 1 frame F)
                want[(0 if ends[0] == 1 else ends[0]):(sc.F if ends[-1] == sc.F - 2 else ends[-1] + 1)] = True
            elif len(ends):
                want[ends[0]] = True
            assert np.isfinite(dt[c, t, :, 0]).tolist() == want.tolist(), (c, t)
    assert torch.equal(dense['ntracks'].cpu(), torch.from_numpy(nt))


# e. -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(ph.BAD_SLOTS)))
def test_invalid_anchor_data_is_latched(k):
    ph.invalid_anchor_data_is_latched('track_pixels_scaled', k, 5500, grid=8, radius=2, scales=2, scale_step=10)


# f. -------------------------------------------------------------------------------------------------------------------
def test_argument_errors():
    from vdetlib_amd import _lib, ops
    images, fr, bx, scr, _ = sc.mixed_case(8, 2)
    ti, tf, tb, ts = g(images), g(fr), g(bx), g(scr)
    cx = _lib.Context()
    try:
        cx.set_timing(2)
        run = lambda i=ti, f=tf, b=tb, s=None, **kw: ops.track_pixels_scaled(i, f, b, s, ctx=cx, **kw)
        bad = [lambda: run(scales=-1), lambda: run(scales=4), lambda: run(scale_step=0), lambda: run(scale_step=26),
               lambda: run(scale_penalty=-1), lambda: run(scale_penalty=65536),
               lambda: run(i=ti[:, :, ::2]), lambda: run(i=ti.float()), lambda: run(i=ti[0]),
               lambda: run(grid=6), lambda: run(grid=68), lambda: run(grid=0), lambda: run(radius=0), lambda: run(radius=17),
               lambda: run(step=0), lambda: run(max_frames=-1), lambda: run(min_conf=float('nan')), lambda: run(min_conf=float('inf')),
               lambda: run(i=ti.cpu()), lambda: run(f=tf.cpu()), lambda: run(b=tb.cpu()), lambda: run(s=ts.cpu()),
               lambda: run(f=tf.long()), lambda: run(b=tb.double()), lambda: run(b=tb[:, :4]), lambda: run(s=ts[:2])]
        for k, fn in enumerate(bad):
            with pytest.raises(ValueError):
                fn()
                pytest.fail("case %d raised nothing" % k)
        # the C-ABI refuses the same settings on its own
        L, z = cx.lib, None
        o = tuple(x.data_ptr() for x in (ti, ti, ti))       # (never written: every call below is refused)
        call = lambda S=8, R=2, mc=.5, mf=0, st=1, ns=1, p=5, q=0, H=sc.H: L.vdet_track_pixels_scaled(
            cx.h, ti.data_ptr(), sc.F, H, sc.W, tf.data_ptr(), tb.data_ptr(), z, 3, 5, S, R, mc, mf, st, ns, p, q, *o)
        for kw in (dict(ns=-1), dict(ns=4), dict(p=0), dict(p=26), dict(q=-1), dict(q=65536), dict(S=6), dict(S=68), dict(R=0),
                   dict(R=17), dict(st=0), dict(mf=-1), dict(mc=float('nan')), dict(H=32768)):
            assert call(**kw) == _lib.VDET_EINVAL, kw
        assert sum(n for _, n in cx.last_timing().values()) == 0, "an argument error launched a kernel"
        kw = dict(grid=8, radius=2, scales=3, scale_step=25, scale_penalty=65535)          # the bounds themselves are legal
        out = run(s=ts, **kw)
        assert cx.last_timing()['other'][1] == 1                                             # ONE launch, timed under 'other'
        assert_same(host(out), px.track_pixels(images, fr, bx, scr, **kw))
    finally:
        cx.close()


# g. -------------------------------------------------------------------------------------------------------------------
def test_prep_cache_is_left_alone():
    import synth
    import torch
    from vdetlib_amd import _lib, ops
    boxes, scores = synth.coherent_video(7433, 12, 120, 3, frac=True)
    tb, ts = g(boxes), g(scores)
    images, fr, bx, scr, _ = sc.mixed_case(8, 2)
    cx = _lib.Context(torch.cuda.current_device())
    try:
        cx.set_cache(True)
        run = lambda: tuple(x.cpu().numpy() for x in ops.nms_track_volume(tb, ts, max_tracks=4, ctx=cx))
        first = run()
        mine = ops.track_pixels_scaled(g(images), g(fr), g(bx), g(scr), grid=8, radius=2, ctx=cx)
        second = run()
    finally:
        cx.close()
    for a, b in zip(first, second):
        assert a.shape == b.shape and np.array_equal(a, b, equal_nan=True)
    assert_same(host(mine), px.track_pixels(images, fr, bx, scr, 8, 2, scales=1))


# h. -------------------------------------------------------------------------------------------------------------------
def test_downstream_from_top_anchors_to_nms_tracks():
    import rescore_spec
    from vdetlib_amd import ops
    images, boxes, scores, truth = sc.greedy_case()
    T = 2
    tb, ts = g(boxes), g(scores)
    fr, ab, asc, _ = ops.top_anchors(tb, ts, T)
    kw = dict(grid=sc.S, radius=sc.R, min_conf=0.0, scales=1, scale_step=5)
    tracks, anchors, nt = ops.track_pixels_scaled(g(images), fr, ab, asc, **kw)
    want = px.track_pixels(images, fr.cpu().numpy(), ab.cpu().numpy(), asc.cpu().numpy(), **kw)
    assert_same(tuple(x.cpu().numpy() for x in (tracks, anchors, nt)), want)
    assert want[2].tolist() == [T, T] and fr.cpu().numpy()[0, 0] == 1           # class 0's first anchor: the growing object
    assert sc.largest_error(want[0][0, 0], truth['grow']) <= 4
    det, pooled, tboxes, src = ops.rescore_tubelets(tracks, nt, tb, ts, complete=False)
    wd, wp, wb, ws, _ = rescore_spec.spec(want[0], want[2], boxes, scores, complete=False)
    for a, b in ((det, wd), (pooled, wp), (tboxes, wb), (src, ws)):
        assert bits_equal(a.cpu().numpy(), b)
    assert np.isin(ws[0, 0], (sc.GIA,) + sc.GIJA).all()                 # every box of the growing tubelet hits one of A's proposals
    out = ops.nms_tracks(tracks, nt, pooled, tboxes)
    assert tuple(out['tracks'].shape) == (sc.GC, T, sc.F, 5) and int(out['cnt'].min()) >= 1


# i. -------------------------------------------------------------------------------------------------------------------
SCALE = dict(scales=1, scale_step=5, scale_penalty=0)


def test_greedy_loop_against_the_spec():
    images, boxes, scores, _ = sc.greedy_case()
    want, fixed = sc.greedy_specs()
    got = greedy_device(images, boxes, scores, **dict(sc.GREEDY, **SCALE))
    assert_same(got, want)
    # (what the case is: test_pixel_track_scaled_cpu.py::test_greedy_case_design) the third anchor of class 0 is a distractor
    # with the search and one of the growing object's late proposals without it
    assert int(got[1][0, 2, 1]) in sc.GIDIS and int(fixed[1][0, 2, 1]) in (sc.GIA,) + sc.GIJA
    kw = dict(sc.GREEDY, step=2, max_frames=7, scales=2, scale_step=10, scale_penalty=32)
    assert_same(greedy_device(images, boxes, scores, **kw), px.track_volume_pixels(images, boxes, scores, **kw))


def test_greedy_loop_without_levels_equals_the_fixed_scale_call():
    from vdetlib_amd import ops
    images, boxes, scores, _ = sc.greedy_case()
    _, fixed = sc.greedy_specs()
    want = tuple(x.cpu().numpy() for x in ops.track_volume_pixels(g(images), g(boxes), g(scores), **sc.GREEDY))
    assert_same(greedy_device(images, boxes, scores, scales=0, scale_step=25, scale_penalty=9, **sc.GREEDY), want)
    assert_same(want, fixed)


def test_greedy_loop_eager_and_lazy_list_maintenance_agree(monkeypatch):
    import torch
    from vdetlib_amd import _lib
    images, boxes, scores, _ = sc.greedy_case()
    want, _ = sc.greedy_specs()
    monkeypatch.setenv('VDET_NO_LAZY', '1')
    cx = _lib.Context(torch.cuda.current_device())
    try:
        got = greedy_device(images, boxes, scores, ctx=cx, **dict(sc.GREEDY, **SCALE))
    finally:
        cx.close()
    monkeypatch.delenv('VDET_NO_LAZY')
    assert_same(got, want)
    assert_same(greedy_device(images, boxes, scores, **dict(sc.GREEDY, **SCALE)), want)


def test_greedy_loop_argument_errors_and_timing():
    import torch
    from vdetlib_amd import _lib, ops
    images, boxes, scores, _ = sc.greedy_case()
    want, _ = sc.greedy_specs()
    ti, tb, ts = g(images), g(boxes), g(scores)
    cx = _lib.Context(torch.cuda.current_device())
    try:
        cx.set_timing(2)
        run = lambda **kw: ops.track_volume_pixels_scaled(ti, tb, ts, ctx=cx, **dict(sc.GREEDY, **dict(SCALE, **kw)))
        for kw in (dict(scales=-1), dict(scales=4), dict(scale_step=0), dict(scale_step=26), dict(scale_penalty=-1),
                   dict(scale_penalty=65536), dict(grid=6), dict(radius=17), dict(step=0), dict(max_tracks=-1)):
            with pytest.raises(ValueError):
                run(**kw)
                pytest.fail("%r raised nothing" % (kw,))
        L = cx.lib
        o = tuple(x.data_ptr() for x in (ti, ti, ti))       # (never written: every call below is refused)
        call = lambda B=sc.GB, S=sc.S, R=sc.R, st=1, ns=1, p=5, q=0: L.vdet_track_volume_pixels_scaled(
            cx.h, ti.data_ptr(), sc.H, sc.W, tb.data_ptr(), ts.data_ptr(), sc.F, B, sc.GC, 0.5, 0.3, 3, S, R, 0.0, 0, st, ns, p, q, *o)
        for kw in (dict(ns=-1), dict(ns=4), dict(p=0), dict(p=26), dict(q=-1), dict(q=65536), dict(B=32768), dict(S=68), dict(R=0),
                   dict(st=0)):
            assert call(**kw) == _lib.VDET_EINVAL, kw
        assert sum(n for _, n in cx.last_timing().values()) == 0, "an argument error launched a kernel"
        assert_same(host(run()), want)           # the context still works
        assert cx.last_timing()['track_loop'][1] == 1          # the loop's launches are ONE timed span, under 'track_loop'
    finally:
        cx.close()


class Opts(object):
    def __init__(self, **kw):
        self.__dict__.update(kw)


def test_dict_level_loop_with_and_without_the_scale_options():
    from vdetlib_amd import ops
    from vdetlib_amd.vdet import track
    images, boxes, scores, _ = sc.greedy_case()
    vid = {'video': 'pixvid', 'root_path': '/nowhere', 'frames': [{'frame': f + 1, 'path': '%04d.JPEG' % f} for f in range(sc.F)]}
    det_info = np.hstack([np.repeat(np.arange(1, sc.F + 1), sc.GB)[:, None].astype(np.float64), boxes.reshape(-1, 4).astype(np.float64),
                          scores.reshape(-1, sc.GC).astype(np.float64)])
    base = dict(step=1, max_frames=None, max_tracks=sc.GREEDY['max_tracks'], thres=sc.GREEDY['thres'], nms_thres=sc.GREEDY['nms_thres'],
                grid=sc.S, radius=sc.R, min_conf=sc.GREEDY['min_conf'])
    view = lambda proto: [[(b['frame'], b['bbox'], b['score'], b['anchor']) for b in t] for t in proto['tracks']]
    scaled = greedy_device(images, boxes, scores, **dict(sc.GREEDY, **SCALE))
    plain = tuple(x.cpu().numpy() for x in ops.track_volume_pixels(g(images), g(boxes), g(scores), **sc.GREEDY))
    assert not bits_equal(scaled[0], plain[0])
    saved = track.imread
    track._pixel_video.clear()
    try:
        track.imread = lambda path: images[int(path.split('/')[-1].split('.')[0])]
        # opts.scales = 1: the device loop with the search, class by class; opts without scales, and scales = 0: today's call
        for opts, (tracks, anchors, ntracks) in ((Opts(scales=1, **base), scaled), (Opts(scales=1, scale_step=5, scale_penalty=0, **base), scaled),
                                                 (Opts(**base), plain), (Opts(scales=0, scale_step=25, **base), plain)):
            for c in range(sc.GC):
                hostp = track.greedily_track_from_raw_dets(vid, det_info, track.pixel_tracker, c + 1, opts)
                mine = ops.tracks_to_proto('pixvid', tracks[c], anchors[c], ntracks[c], method='pixel_tracker')
                assert hostp['method'] == mine['method'] == 'pixel_tracker'
                assert len(hostp['tracks']) == int(ntracks[c]) and view(hostp) == view(mine), (sorted(opts.__dict__), c)
    finally:
        track.imread = saved
        track._pixel_video.clear()
