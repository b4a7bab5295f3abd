"""-m gpu: box-filter sampling for the pixel tracker on the device (ops.luma_integral; ``sampling='box'`` of ops.track_pixels,
track_pixels_scaled, track_volume_pixels, track_volume_pixels_scaled and of vdet.track.pixel_tracker;
csrc/pixtrack_kernels.hpp) against tests/pixtrack_spec.py (``sampling='box'``) ON BITS: the NaN masks are equal and every other element has
the same bit pattern.
  a. luma_integral;  b. the mixed [3,5] slot table, four (grid, radius) pairs x four scale settings;  c. where box sampling is
  point sampling, and the degenerate cells;  d. ties, step and max_frames, the defaults;  e. the ``integral=`` argument;
  f. the greedy forms and the dict level;  g. invalid anchor data, argument errors, the context's prep cache;
  h. the sub-cell videos of test_pixel_track_box_cpu.py."""
import numpy as np
import pytest

import functools

import pixtrack_box_cases as bc
import pixtrack_harness as ph
import pixtrack_scale_cases as sc
import pixtrack_spec as px
from pixtrack_harness import assert_same, bits_equal, g, host

pytestmark = pytest.mark.gpu

BOX = dict(sampling='box')
device = functools.partial(ph.device, **BOX)                # ops.track_pixels without ``scales``, ops.track_pixels_scaled with
assert_spec = functools.partial(ph.assert_spec, **BOX)      # device == spec on bits; returns the spec's outputs

# a. -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ((1, 1, 1), (2, 3, 5), (3, 37, 259), (2, 130, 64)))
def test_luma_integral(shape):
    """random frames; [3,37,259]: a row crosses the 64- and 256-pixel trips of the row scan and W + 1 is no multiple of 4.  The
    C-ABI call on a buffer of ones in every bit: every element, the zero row and column included, is written"""
    import torch
    from vdetlib_amd import _lib, ops
    F, H, W = shape
    images = np.random.RandomState(7800 + W).randint(0, 256, size=(F, H, W, 3)).astype(np.uint8)
    want = px.luma_integral(images)
    ti = g(images)
    out = ops.luma_integral(ti)
    assert out.dtype == torch.uint32 and tuple(out.shape) == (F, H + 1, W + 1) and out.is_contiguous() and out.device == ti.device
    assert np.array_equal(out.cpu().numpy(), want)
    raw = torch.full((F, H + 1, W + 1), -1, dtype=torch.int32, device=ti.device)
    cx = _lib.get_context(ti.device.index)
    cx.check(cx.lib.vdet_luma_integral(cx.h, ti.data_ptr(), F, H, W, raw.data_ptr()))
    cx.sync()
    assert np.array_equal(raw.cpu().numpy().view(np.uint32), want)


@pytest.mark.parametrize("H,W", ((4096, 2049), (4096, 4096)))
def test_luma_integral_of_a_white_frame(H, W):
    """all 255: luma 255, I[y, x] = 255 * y * x.  [4096,2049]: an odd width whose sums end 0.3 % below 2^31 (2 140 139 520);
    [4096,4096]: the limit H*W = 2^24, whose last entry is 255 * 2^24: the sums pass 2^31, so a signed or saturating
    accumulator fails"""
    import torch
    from vdetlib_amd import ops
    out = ops.luma_integral(torch.full((1, H, W, 3), 255, dtype=torch.uint8, device='cuda')).cpu().numpy()
    want = (255 * np.outer(np.arange(H + 1, dtype=np.uint64), np.arange(W + 1, dtype=np.uint64))).astype(np.uint32)[None]
    assert int(want.max()) == int(want[0, H, W]) == 255 * H * W and (W != 4096 or int(want.max()) == 255 << 24 > 1 << 31)
    assert out.dtype == np.uint32 and np.array_equal(out, want)


# b. -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", (None, (1, 5, 0), (3, 25, 0), (1, 10, 64)))
@pytest.mark.parametrize("S,R", ((8, 2), (32, 8), (64, 16), (12, 3)))
def test_mixed_slot_table(S, R, scale):
    """scale None: ops.track_pixels (scales = 0); else ops.track_pixels_scaled"""
    images, fr, bx, scr, truth = sc.mixed_case(S, R)
    kw = dict(grid=S, radius=R)
    if scale is not None:
        kw.update(scales=scale[0], scale_step=scale[1], scale_penalty=scale[2])
    tracks, anchors, nt, _ = assert_spec(images, fr, bx, scr, min_conf=0.0, **kw)
    assert nt.tolist() == [4, 5, 3]
    # the case is still what it says under box sampling: every live slot walks, no empty slot has a row ...
    live = np.isfinite(tracks[..., 0])
    assert live[fr > 0].sum(axis=-1).min() >= 2 and not live[fr == 0].any()
    # ... the first-frame and the last-frame anchors run the whole video in one direction ...
    assert live[0, 1].all() and live[0, 2].all()
    # ... with levels the boxes do change size, without them they cannot ...
    wid = tracks[..., 2] - tracks[..., 0]
    if scale is not None:
        assert np.nanmax(wid[0, 1]) > wid[0, 1, 0] and np.nanmax(wid[0, 2]) > wid[0, 2, sc.F - 1]
    else:
        assert np.nanmax(wid[0, 1]) == np.nanmin(wid[0, 1]) == wid[0, 1, 0]
    # ... and the leaver's chain ends because its box is wholly outside, before the video does
    assert live[2, 0].tolist() == [True] * sc.LEAVES + [False] * (sc.F - sc.LEAVES)


# c. -------------------------------------------------------------------------------------------------------------------
def test_one_pixel_cells_give_the_point_calls_bits():
    """w == h == S, scales = 0: the anchors of test_pixel_track_box_cpu.py in the corners and on the sides of the image"""
    from vdetlib_amd import ops
    rng = np.random.RandomState(7602)
    S, R, F, H, W = 8, 3, 6, 20, 24
    images = rng.randint(0, 256, size=(F, H, W, 3)).astype(np.uint8)
    xs, ys = (-3, 8, W - 5), (-3, 6, H - 5)
    boxes = [[x + 1, y + 1, x + S, y + S] for y in ys for x in xs]
    fr = np.array([[1 + k % F for k in range(len(boxes))]], np.int32)
    bx = np.array([boxes], np.float32)
    ti, tf, tb = g(images), g(fr), g(bx)
    for kw in (dict(min_conf=0.0), dict(min_conf=0.0, step=2), dict()):
        point = host(ops.track_pixels(ti, tf, tb, grid=S, radius=R, **kw))
        assert_same(host(ops.track_pixels(ti, tf, tb, grid=S, radius=R, sampling='box', **kw)), point)
        assert_same(host(ops.track_pixels_scaled(ti, tf, tb, grid=S, radius=R, scales=0, sampling='box', **kw)), point)
        assert_same(point, px.track_pixels(images, fr, bx, None, S, R, **BOX, **kw))
    assert np.isfinite(point[0][0, :, :, 0]).sum(axis=1).min() >= 2


def test_degenerate_cells():
    """an anchor of 5 x 3 pixels under grid 8: cells narrower than a pixel; an anchor half outside the image; an anchor of 2^20
    pixels a side around a small image: almost every cell is wholly outside"""
    rng = np.random.RandomState(7801)
    images = rng.randint(0, 256, size=(5, 40, 56, 3)).astype(np.uint8)
    big = 1 << 19
    fr = np.array([[2, 3, 1, 4, 5]], np.int32)
    bx = np.array([[[20, 15, 24, 17], [-15, 10, 16, 33], [30, 25.5, 70, 60], [-big + 1, -big + 1, big, big],
                    [-big + 40, -big + 30, big + 40, big + 30]]], np.float32)
    for kw in (dict(grid=8, radius=2), dict(grid=8, radius=2, scales=2, scale_step=25), dict(grid=16, radius=4, scales=1)):
        tracks = assert_spec(images, fr, bx, min_conf=0.0, **kw)[0]
        assert np.isfinite(tracks[0, :, :, 0]).sum(axis=1).min() >= 2


# d. -------------------------------------------------------------------------------------------------------------------
def test_every_key_ties_on_a_constant_image():
    """every cell of every box on every frame is 100: all keys tie on SAD 0; shift 0 (and level 0) wins, conf = 1"""
    F = 4
    images = np.full((F, 32, 40, 3), 100, np.uint8)
    fr, bx = np.array([[2]], np.int32), np.array([[[12, 11, 30, 22]]], np.float32)
    want = np.tile(np.array([12, 11, 30, 22, 1.0], np.float32), (F, 1))
    for kw in (dict(), dict(scales=3, scale_step=25, scale_penalty=0), dict(scales=1, scale_step=5, scale_penalty=7)):
        tracks = assert_spec(images, fr, bx, grid=8, radius=2, min_conf=1.0, **kw)[0][0, 0]
        assert bits_equal(tracks, want)


def test_step_and_max_frames():
    images, fr, bx, scr, _ = sc.mixed_case(8, 2)
    for kw in (dict(), dict(scales=1, scale_step=10)):
        for mf in (0, 5, 6):
            tracks = assert_spec(images, fr, bx, scr, grid=8, radius=2, min_conf=0.0, max_frames=mf, step=3, **kw)[0]
            live = np.isfinite(tracks[..., 0])
            reach = px.reach_of(mf, sc.F)
            for c in range(3):
                for t in range(5):
                    f0 = int(fr[c, t]) - 1
                    assert all((f - f0) % 3 == 0 and abs(f - f0) // 3 <= reach for f in np.flatnonzero(live[c, t])), (mf, c, t)
            assert np.flatnonzero(live[0, 2]).tolist() == ([5, 8, 11] if mf == 5 else [2, 5, 8, 11])


def test_default_settings():
    """grid 32, radius 8, min_conf 0.5, no scores: the calls with nothing but the data and sampling='box'"""
    images, fr, bx, _, _ = sc.mixed_case(32, 8)
    tracks = assert_spec(images, fr, bx)[0]
    assert np.isfinite(tracks[0, 1:4, :, 0]).sum() >= 6
    assert_same(device(images, fr, bx, scales=1), px.track_pixels(images, fr, bx, scales=1, scale_step=5, scale_penalty=0, **BOX))


# e. -------------------------------------------------------------------------------------------------------------------
def test_one_integral_serves_every_call():
    import greedy_pixel_cases as gc
    from vdetlib_amd import ops
    (images, boxes, scores, _, _), _ = gc.main_case()
    fr = np.array([[gc.FA + 1, 0, gc.FB + 1]], np.int32)
    bx = np.stack([boxes[gc.FA, gc.IA], boxes[0, 0], boxes[gc.FB, gc.IB]])[None]
    ti, tf, tb, tbx, ts = g(images), g(fr), g(bx), g(boxes), g(scores)
    integ = ops.luma_integral(ti)
    before = integ.cpu().numpy().copy()
    kw = dict(grid=gc.S, radius=gc.R, min_conf=0.0)
    sk = dict(scales=1, scale_step=10, scale_penalty=0)
    mine = host(ops.track_pixels(ti, tf, tb, sampling='box', integral=integ, **kw))
    assert_same(mine, host(ops.track_pixels(ti, tf, tb, sampling='box', **kw)))
    assert_same(mine, px.track_pixels(images, fr, bx, None, **BOX, **kw))
    mine = host(ops.track_pixels_scaled(ti, tf, tb, sampling='box', integral=integ, **dict(kw, **sk)))
    assert_same(mine, host(ops.track_pixels_scaled(ti, tf, tb, sampling='box', **dict(kw, **sk))))
    assert_same(mine, px.track_pixels(images, fr, bx, None, **BOX, **dict(kw, **sk)))
    mine = host(ops.track_volume_pixels_scaled(ti, tbx, ts, sampling='box', integral=integ, **dict(gc.MAIN, **sk)))
    assert_same(mine, host(ops.track_volume_pixels_scaled(ti, tbx, ts, sampling='box', **dict(gc.MAIN, **sk))))
    assert_same(mine, px.track_volume_pixels(images, boxes, scores, **BOX, **dict(gc.MAIN, **sk)))
    assert np.array_equal(integ.cpu().numpy(), before)                  # read, never written
    # with an integral the images are read for their shape only: frames of zeros give the same tubelets
    import torch
    assert_same(host(ops.track_pixels(torch.zeros_like(ti), tf, tb, sampling='box', integral=integ, **kw)),
                px.track_pixels(images, fr, bx, None, **BOX, **kw))


# f. -------------------------------------------------------------------------------------------------------------------
SCALE = dict(scales=1, scale_step=5, scale_penalty=0)
_greedy = {}


def greedy_wants():
    """the box spec's greedy loop on greedy_pixel_cases' main volume, fixed scale and with levels; computed once"""
    if not _greedy:
        import greedy_pixel_cases as gc
        (images, boxes, scores, _, _), point = gc.main_case()
        _greedy['fixed'] = px.track_volume_pixels(images, boxes, scores, **BOX, **gc.MAIN)
        _greedy['scaled'] = px.track_volume_pixels(images, boxes, scores, **BOX, **dict(gc.MAIN, **SCALE))
        assert not _greedy['fixed'][3] and not _greedy['scaled'][3] and int(_greedy['fixed'][2].sum()) >= 3
    return _greedy['fixed'], _greedy['scaled']


def greedy_device(scaled, ctx=None, **kw):
    """ops.track_volume_pixels_scaled at SCALE where ``scaled``, else ops.track_volume_pixels, on the main volume"""
    import greedy_pixel_cases as gc
    (images, boxes, scores, _, _), _ = gc.main_case()
    return ph.greedy_device(images, boxes, scores, ctx=ctx, **BOX, **dict(gc.MAIN, **dict(SCALE if scaled else {}, **kw)))


def test_greedy_forms_against_the_spec():
    import greedy_pixel_cases as gc
    fixed, scaled = greedy_wants()
    assert_same(greedy_device(False), fixed)
    assert_same(greedy_device(True), scaled)
    (images, boxes, scores, _, _), _ = gc.main_case()
    kw = dict(step=2, max_frames=7)
    assert_same(greedy_device(False, **kw), px.track_volume_pixels(images, boxes, scores, **BOX, **dict(gc.MAIN, **kw)))


def test_greedy_forms_eager_and_lazy_list_maintenance_agree(monkeypatch):
    import torch
    from vdetlib_amd import _lib
    fixed, scaled = greedy_wants()
    monkeypatch.setenv('VDET_NO_LAZY', '1')
    cx = _lib.Context(torch.cuda.current_device())
    try:
        got = greedy_device(False, ctx=cx), greedy_device(True, ctx=cx)
    finally:
        cx.close()
    monkeypatch.delenv('VDET_NO_LAZY')
    assert_same(got[0], fixed)
    assert_same(got[1], scaled)


class Opts(object):
    def __init__(self, **kw):
        self.__dict__.update(kw)


def test_dict_level_tracker_with_the_sampling_option():
    import greedy_pixel_cases as gc
    from vdetlib_amd import ops
    from vdetlib_amd.vdet import track
    (images, boxes, scores, _, _), _ = gc.main_case()
    vid = {'video': 'boxvid', 'root_path': '/nowhere', 'frames': [{'frame': f + 1, 'path': '%04d.JPEG' % f} for f in range(gc.F)]}
    det_info = np.hstack([np.repeat(np.arange(1, gc.F + 1), gc.B)[:, None].astype(np.float64), boxes.reshape(-1, 4).astype(np.float64),
                          scores.reshape(-1, gc.C).astype(np.float64)])
    base = dict(step=1, max_frames=None, max_tracks=gc.MAIN['max_tracks'], thres=gc.MAIN['thres'], nms_thres=gc.MAIN['nms_thres'],
                grid=gc.S, radius=gc.R, min_conf=gc.MAIN['min_conf'])
    view = lambda proto: [[(b['frame'], b['bbox'], b['score'], b['anchor']) for b in t] for t in proto['tracks']]
    point = host(ops.track_volume_pixels(g(images), g(boxes), g(scores), **gc.MAIN))
    saved = track.imread
    track._pixel_video.clear()
    try:
        track.imread = lambda path: images[int(path.split('/')[-1].split('.')[0])]
        for opts, (tracks, anchors, ntracks) in ((Opts(sampling='box', **base), greedy_device(False)),
                                                 (Opts(sampling='box', scales=1, **base), greedy_device(True)),
                                                 (Opts(sampling='point', **base), point), (Opts(**base), point)):
            for c in range(gc.C):
                hostp = track.greedily_track_from_raw_dets(vid, det_info, track.pixel_tracker, c + 1, opts)
                mine = ops.tracks_to_proto('boxvid', tracks[c], anchors[c], ntracks[c], method='pixel_tracker')
                assert len(hostp['tracks']) == int(ntracks[c]) and view(hostp) == view(mine), (sorted(opts.__dict__), c)
        # the tracker alone against the array call, one anchor
        box = [float(v) for v in boxes[gc.FA, gc.IA]]
        proto = track.pixel_tracker(vid, gc.FA + 1, box, Opts(sampling='box', **base))
        rows = host(ops.track_pixels(g(images), g(np.array([[gc.FA + 1]], np.int32)), g(np.array([[box]], np.float32)), grid=gc.S,
                                     radius=gc.R, min_conf=gc.MAIN['min_conf'], sampling='box'))[0][0, 0]
        on = np.flatnonzero(np.isfinite(rows[:, 0]))
        assert [b['frame'] for b in proto[0]] == (on + 1).tolist()
        assert all(b['bbox'] == rows[f, :4].tolist() and b['score'] == float(rows[f, 4]) for b, f in zip(proto[0], on))
        with pytest.raises(ValueError):
            track.pixel_tracker(vid, gc.FA + 1, box, Opts(sampling='area', **base))
    finally:
        track.imread = saved
        track._pixel_video.clear()


# g. -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(ph.BAD_SLOTS)))
def test_invalid_anchor_data_is_latched(k):
    ph.invalid_anchor_data_is_latched('track_pixels', k, 5500, grid=8, radius=2, **BOX)


def test_argument_errors():
    import greedy_pixel_cases as gc
    import torch
    from vdetlib_amd import _lib, ops
    images, fr, bx, scr, _ = sc.mixed_case(8, 2)
    (gimages, gboxes, gscores, _, _), _ = gc.main_case()
    ti, tf, tb = g(images), g(fr), g(bx)
    gi, gb, gs_ = g(gimages), g(gboxes), g(gscores)
    huge = torch.empty((1, 4097, 4096, 3), dtype=torch.uint8, device='cuda')         # H*W = 2^24 + 4096
    f1, b1 = g(np.array([[1]], np.int32)), g(np.array([[[5, 5, 40, 40]]], np.float32))
    cx = _lib.Context()
    try:
        cx.set_timing(2)
        integ = ops.luma_integral(ti, ctx=cx)
        assert cx.last_timing()['other'][1] == 1                 # the two launches are ONE timed span, under 'other'
        ginteg = ops.luma_integral(gi, ctx=cx)
        calls = (lambda **kw: ops.track_pixels(ti, tf, tb, grid=8, radius=2, ctx=cx, **kw),
                 lambda **kw: ops.track_pixels_scaled(ti, tf, tb, grid=8, radius=2, ctx=cx, **kw),
                 lambda **kw: ops.track_volume_pixels(gi, gb, gs_, ctx=cx, **dict(gc.MAIN, **kw)),
                 lambda **kw: ops.track_volume_pixels_scaled(gi, gb, gs_, ctx=cx, **dict(gc.MAIN, **kw)))
        cx.last_timing()
        for n, run in enumerate(calls):
            mine = integ if n < 2 else ginteg
            bad = [dict(sampling='area'), dict(sampling=None), dict(sampling='Box'),
                   dict(sampling='point', integral=mine), dict(integral=mine),
                   dict(sampling='box', integral=mine.view(torch.int32)), dict(sampling='box', integral=mine.to(torch.int64)),
                   dict(sampling='box', integral=mine[:, :-1]), dict(sampling='box', integral=mine[:-1]),
                   dict(sampling='box', integral=mine[:, :, :-1]), dict(sampling='box', integral=mine.cpu()),
                   dict(sampling='box', integral=mine.cpu().numpy()),
                   dict(sampling='box', integral=torch.empty((mine.shape[0], mine.shape[2], mine.shape[1]), dtype=torch.uint32,
                                                             device=mine.device).transpose(1, 2))]
            for kw in bad:
                with pytest.raises(ValueError):
                    run(**kw)
                    pytest.fail("call %d: %r raised nothing" % (n, sorted(kw)))
        for fn in (lambda: ops.luma_integral(huge, ctx=cx), lambda: ops.track_pixels(huge, f1, b1, sampling='box', ctx=cx),
                   lambda: ops.track_pixels_scaled(huge, f1, b1, sampling='box', ctx=cx),
                   lambda: ops.luma_integral(ti.float(), ctx=cx), lambda: ops.luma_integral(ti[:, :, ::2], ctx=cx),
                   lambda: ops.luma_integral(ti.cpu(), ctx=cx)):
            with pytest.raises(ValueError):
                fn()
        # (the point call takes the same frames: the limit is box sampling's)
        assert np.isfinite(host(ops.track_pixels(huge.zero_(), f1, b1, ctx=cx))[0][0, 0, 0]).all()
        cx.last_timing()
        # the C-ABI refuses on its own: H*W > 2^24, a NULL integral, and what the mirrored calls refuse
        L, z = cx.lib, None
        o = tuple(x.data_ptr() for x in (ti, ti, ti))            # (never written: every call below is refused)
        ip = integ.data_ptr()
        assert L.vdet_luma_integral(cx.h, huge.data_ptr(), 1, 4097, 4096, ip) == _lib.VDET_EINVAL
        assert L.vdet_luma_integral(cx.h, ti.data_ptr(), sc.F, sc.H, sc.W, z) == _lib.VDET_EINVAL
        assert L.vdet_luma_integral(cx.h, z, sc.F, sc.H, sc.W, ip) == _lib.VDET_EINVAL
        assert L.vdet_luma_integral(cx.h, ti.data_ptr(), 0, sc.H, sc.W, ip) == _lib.VDET_EINVAL
        assert L.vdet_luma_integral(cx.h, ti.data_ptr(), 1, 32768, 16, ip) == _lib.VDET_EINVAL
        call = lambda I=ip, S=8, R=2, mc=.5, mf=0, st=1, ns=0, p=5, q=0, H=sc.H, W=sc.W: L.vdet_track_pixels_box(
            cx.h, I, sc.F, H, W, tf.data_ptr(), tb.data_ptr(), z, 3, 5, S, R, mc, mf, st, ns, p, q, *o)
        for kw in (dict(I=z), dict(H=4097, W=4096), dict(ns=-1), dict(ns=4), dict(p=0), dict(p=26), dict(q=-1), dict(q=65536),
                   dict(S=6), dict(S=68), dict(R=0), dict(R=17), dict(st=0), dict(mf=-1), dict(mc=float('nan')), dict(H=32768)):
            assert call(**kw) == _lib.VDET_EINVAL, kw
        gcall = lambda I=ginteg.data_ptr(), B=gc.B, S=gc.S, R=gc.R, st=1, ns=0, p=5, q=0, H=gc.H, W=gc.W: L.vdet_track_volume_pixels_box(
            cx.h, I, H, W, gb.data_ptr(), gs_.data_ptr(), gc.F, B, gc.C, 0.3, 0.3, 3, S, R, 0.0, 0, st, ns, p, q, *o)
        for kw in (dict(I=z), dict(H=4097, W=4096), dict(ns=4), dict(p=0), dict(q=65536), dict(B=32768), dict(S=68), dict(R=0), dict(st=0)):
            assert gcall(**kw) == _lib.VDET_EINVAL, kw
        assert sum(n for _, n in cx.last_timing().values()) == 0, "an argument error launched a kernel"
        # the context still works; with the integral passed in the tracker is ONE launch, timed under 'other'
        out = ops.track_pixels_scaled(ti, tf, tb, g(scr), grid=8, radius=2, scales=3, scale_step=25, scale_penalty=65535, sampling='box',
                                      integral=integ, ctx=cx)
        assert cx.last_timing()['other'][1] == 1
        assert_same(host(out), px.track_pixels(images, fr, bx, scr, grid=8, radius=2, scales=3, scale_step=25, scale_penalty=65535, **BOX))
    finally:
        cx.close()


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
        run = lambda: host(ops.nms_track_volume(tb, ts, max_tracks=4, ctx=cx))
        first = run()
        integ = ops.luma_integral(g(images), ctx=cx)
        mine = ops.track_pixels(g(images), g(fr), g(bx), g(scr), grid=8, radius=2, ctx=cx, sampling='box', integral=integ)
        second = run()
    finally:
        cx.close()
    for a, b in zip(first, second):
        assert a.shape == b.shape and np.array_equal(a, b, equal_nan=True)
    assert np.array_equal(integ.cpu().numpy(), px.luma_integral(images))
    assert_same(host(mine), px.track_pixels(images, fr, bx, scr, 8, 2, **BOX))


# h. -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", bc.SIZES)
@pytest.mark.parametrize("seed", bc.SEEDS)
def test_sub_cell_videos(seed, w, h):
    """the device follows the videos the point rule loses as the spec does (the bounds: test_pixel_track_box_cpu.py)"""
    import math
    images, pos = bc.sub_cell_video(seed, w, h)
    fr, bx = bc.anchor_of(pos, w, h)
    rows = assert_spec(images, fr, bx, **bc.KW)[0][0, 0]
    ex, ey = bc.errors(rows, pos)
    assert np.isfinite(rows).all() and ex.max() <= math.ceil(w / float(bc.S) / 2) and ey.max() <= math.ceil(h / float(bc.S) / 2)
