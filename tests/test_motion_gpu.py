"""-m gpu: motion-guided propagation on the device (ops.motion_field, ops.propagate_detections; csrc/motion_kernels.hpp) against
tests/motion_spec.py ON BITS: the NaN masks are equal and every other element has the same bit pattern.
  a. motion_field;  b. propagate_detections;  c. bad data;  d. argument errors before any launch;  e. the context's prep cache;
  f. end to end: nms_volume -> motion_field -> propagate_detections -> nms_tracks -> DetEvaluator on a planted scene."""
import functools

import numpy as np
import pytest

import motion_cases as mc
import motion_spec as ms
from pixtrack_harness import bits_equal, g

pytestmark = pytest.mark.gpu

FIELD_KEYS = ('field', 'cost', 'fsum')
PROP_KEYS = ('tracks', 'ntracks', 'score', 'src')


def field_device(images, P, R, **kw):
    from vdetlib_amd import ops
    out = ops.motion_field(g(images), block=P, radius=R, **kw)
    assert out['block'] == P and out['size'] == tuple(images.shape[1:3])
    return tuple(out[k].cpu().numpy() for k in FIELD_KEYS)


def assert_field(images, P, R):
    """device == spec; returns the spec's outputs"""
    want = ms.motion_field(images, P, R)
    got = field_device(images, P, R)
    for name, a, b in zip(FIELD_KEYS, got, want):
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), name
    return want


# a. -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F,H,W,P,R", ((5, 37, 53, 8, 2),       # partial blocks on both axes, W no multiple of 4
                                       (2, 70, 70, 32, 16),     # two tiles a side, the largest block and radius
                                       (3, 5, 7, 8, 3),         # the image is smaller than one block
                                       (1, 16, 16, 8, 2),       # one frame: no pair at all, everything zero
                                       (4, 40, 200, 8, 16),     # the region is wider than a tile, four tiles in a row
                                       (3, 33, 130, 16, 5),     # a candidate count (121) that fills 32-lane groups unevenly
                                       (2, 24, 40, 8, 1)))      # nine candidates in a 16-lane group
def test_motion_field_of_noise(F, H, W, P, R):
    images = np.random.RandomState(9200 + W).randint(0, 256, size=(F, H, W, 3)).astype(np.uint8)
    field, cost, fsum = assert_field(images, P, R)
    if F == 1:
        assert not field.any() and not cost.any() and not fsum.any()
    else:
        assert cost[0, :-1].min() > 0 and not cost[0, -1].any() and not cost[1, 0].any()


def test_motion_field_of_a_planted_translation():
    """a random canvas seen through a window that moves: every block whose search window stays inside the image finds the planted
    vector at cost 0, forward and backward"""
    F, H, W, P, R, vx, vy = 3, 64, 80, 16, 8, 5, -3
    canvas = np.random.RandomState(9201).randint(0, 256, size=(H + 32, W + 32, 3)).astype(np.uint8)
    images = np.stack([canvas[16 - vy * f:16 - vy * f + H, 16 - vx * f:16 - vx * f + W] for f in range(F)])
    field, cost, _ = assert_field(images, P, R)
    assert (field[0, :2, 1:3, 1:4] == [vx, vy]).all() and (field[1, 1:, 1:3, 1:4] == [-vx, -vy]).all()
    assert not cost[0, :2, 1:3, 1:4].any() and not cost[1, 1:, 1:3, 1:4].any()


def test_motion_field_ties():
    """a flat video: every key ties on SAD 0 and zero motion wins.  One brighter pixel on the middle frame: its own block pays
    for it at every shift (all keys tie on SAD 165: zero motion); the same block of the neighbouring frames steps aside by the
    shortest shift that leaves the pixel out, (0, 2), at SAD 0"""
    flat = np.full((3, 40, 72, 3), 90, np.uint8)
    field, cost, fsum = assert_field(flat, 8, 4)
    assert not field.any() and not cost.any() and not fsum.any()
    one = flat.copy()
    one[1, 17, 35] = 255
    field, cost, _ = assert_field(one, 8, 4)
    assert cost[0, 1, 2, 4] == cost[1, 1, 2, 4] == 165 and cost.sum() == 2 * 165 and not field[:, 1].any()
    assert field[0, 0, 2, 4].tolist() == field[1, 2, 2, 4].tolist() == [0, 2] and np.abs(field).sum() == 4
    assert_field(one, 16, 8)


@pytest.mark.parametrize("F,H,W,P,R", ((3, 37, 53, 8, 2), (2, 70, 140, 16, 8)))
def test_motion_field_writes_every_element(F, H, W, P, R):
    """the C-ABI on buffers of ones in every bit: the zero frames, the zero row and the zero column included.  The table alone
    (vdet_motion_table) from the field gives the same table"""
    import torch
    from vdetlib_amd import _lib
    images = np.random.RandomState(9202).randint(0, 256, size=(F, H, W, 3)).astype(np.uint8)
    want = ms.motion_field(images, P, R)
    Hb, Wb = ms.grid_of(H, W, P)
    ti = g(images)
    ones = lambda shape, dt: torch.full(shape, -1, dtype=dt, device=ti.device)
    field, cost, fsum = ones((2, F, Hb, Wb, 2), torch.int16), ones((2, F, Hb, Wb), torch.int32), ones((2, F, Hb + 1, Wb + 1, 2), torch.int32)
    cx = _lib.get_context(ti.device.index)
    cx.check(cx.lib.vdet_motion_field(cx.h, ti.data_ptr(), F, H, W, P, R, field.data_ptr(), cost.data_ptr(), fsum.data_ptr()))
    cx.sync()
    for a, b in zip((field, cost, fsum), want):
        assert np.array_equal(a.cpu().numpy(), b)
    again = ones((2, F, Hb + 1, Wb + 1, 2), torch.int32)
    cx.check(cx.lib.vdet_motion_table(cx.h, field.data_ptr(), F, Hb, Wb, again.data_ptr()))
    cx.sync()
    assert np.array_equal(again.cpu().numpy(), want[2])


def test_motion_table_of_a_wide_field():
    """more than 64 block columns: the carry between two column passes, on a field of the largest vectors"""
    import torch
    from vdetlib_amd import _lib
    F, Hb, Wb = 2, 7, 150
    field = np.random.RandomState(9203).randint(-16, 17, size=(2, F, Hb, Wb, 2)).astype(np.int16)
    field[0, 0] = 16
    field[1, 1] = -16
    tf = g(field)
    out = torch.full((2, F, Hb + 1, Wb + 1, 2), -1, dtype=torch.int32, device=tf.device)
    cx = _lib.get_context(tf.device.index)
    cx.check(cx.lib.vdet_motion_table(cx.h, tf.data_ptr(), F, Hb, Wb, out.data_ptr()))
    cx.sync()
    assert np.array_equal(out.cpu().numpy(), ms.summed(field))


# b. -------------------------------------------------------------------------------------------------------------------
FP, BP, CP, KCAP = 7, 12, 3, 5
HP, WP, PP = 60, 90, 8
LEAVER = 4          # the box that leaves the image on its second step forward


@functools.lru_cache(maxsize=None)
def propagate_case():
    """a random field (so that every source moves differently) whose last four block columns move 16 pixels right going
    forward; twelve boxes a frame: random ones, fractional and negative coordinates, the whole image, a degenerate box, the
    leaver; keep counts 0, 2 and 5 with the frames 0 and F-1 always populated"""
    rng = np.random.RandomState(9300)
    Hb, Wb = ms.grid_of(HP, WP, PP)
    field = rng.randint(-6, 7, size=(2, FP, Hb, Wb, 2)).astype(np.int16)
    field[0, :, :, -4:] = (16, 0)
    field[0, FP - 1] = 0
    field[1, 0] = 0
    fsum = ms.summed(field)
    x1 = rng.uniform(-10, WP - 20, size=(FP, BP))
    y1 = rng.uniform(-10, HP - 20, size=(FP, BP))
    boxes = np.stack([x1, y1, x1 + rng.uniform(4, 50, size=(FP, BP)), y1 + rng.uniform(4, 40, size=(FP, BP))], axis=-1).astype(np.float32)
    boxes[:, 0] = np.round(boxes[:, 0])
    boxes[:, 1] = (-7.5, -3.25, 14.75, 9.5)                 # fractional and negative
    boxes[:, 2] = (1, 1, WP, HP)                            # the whole image
    boxes[:, 3] = (40, 30, 35, 20)                          # degenerate: x2 < x1, y2 < y1
    boxes[:, LEAVER] = (WP - 21, 10, WP - 9, 30)
    boxes[:, 5] = (-300, -200, 500, 400)                    # far larger than the image
    scores = rng.uniform(-1, 1, size=(FP, BP, CP)).astype(np.float32)
    keep_idx = np.stack([np.stack([rng.permutation(BP)[:KCAP] for _ in range(CP)]) for _ in range(FP)]).astype(np.int32)
    keep_cnt = rng.choice([0, 2, 5], size=(FP, CP)).astype(np.int32)
    keep_cnt[0], keep_cnt[FP - 1] = (5, 2, 5), (2, 5, 5)
    keep_idx[2, 1, 0] = LEAVER
    keep_cnt[2, 1] = 5
    keep_idx[3, 0, :4] = (2, 3, 1, 5)
    keep_cnt[3, 0] = 5
    assert set(keep_cnt.reshape(-1).tolist()) == {0, 2, 5}
    return fsum, boxes, scores, keep_idx, keep_cnt


def motion_of(fsum):
    return dict(fsum=g(fsum), block=PP, size=(HP, WP))


def prop_device(fsum, still, **kw):
    from vdetlib_amd import ops
    out = ops.propagate_detections(motion_of(fsum), tuple(g(x) for x in still), **kw)
    return tuple(out[k].cpu().numpy() for k in PROP_KEYS)


def assert_prop(got, want):
    for name, a, b in zip(PROP_KEYS, got, want):
        assert bits_equal(a, b), name


@pytest.mark.parametrize("reach", (1, 2, 3, 8))
@pytest.mark.parametrize("top", (1, 4, 5))
def test_propagate_detections(top, reach):
    fsum, *still = propagate_case()
    for decay in (1.0, 0.5):
        want = ms.propagate(fsum, PP, HP, WP, *still, top=top, reach=reach, decay=decay)
        assert not want[4]
        assert_prop(prop_device(fsum, still, top=top, reach=reach, decay=decay), want)
    tracks, ntracks, score, src = want[:4]
    T = 2 * reach * top
    assert tracks.shape == (CP, T, FP, 5) and ntracks.tolist() == [T] * CP
    live = np.isfinite(tracks[..., 0])
    assert live.any() and not live.all()
    # a source on frame 0 reaches frame 1 and nothing before it; one on frame F-1 reaches F-2
    assert live[0, (reach + 0) * top, 1] and live[0, (reach - 1) * top, FP - 2]
    if reach >= 2:
        # the leaver (frame 2, class 1, entry 0): one step forward, none after it
        assert live[1, reach * top, 3] and not live[1, (reach + 1) * top, 4] and src[1, reach * top, 3] == LEAVER


def test_propagate_detections_defaults():
    """reach 3 and decay 1.0: the scores are the sources' bits"""
    fsum, *still = propagate_case()
    want = ms.propagate(fsum, PP, HP, WP, *still, top=2)
    assert_prop(prop_device(fsum, still, top=2), want)
    live = np.isfinite(want[2])
    assert np.isin(want[2][live].view(np.uint32), still[1].view(np.uint32)).all()


# c. -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("nan", "huge", "index", "count"))
def test_bad_data_is_latched(kind):
    """the call raises -- at once, or with sync=False at the context's next wait --, the bad source writes NaN rows, every
    other source's rows are the spec's, the latch is cleared by the wait that reports it"""
    from vdetlib_amd import _lib, ops
    fsum, boxes, scores, keep_idx, keep_cnt = propagate_case()
    boxes, keep_idx, keep_cnt = boxes.copy(), keep_idx.copy(), keep_cnt.copy()
    if kind == "nan":
        boxes[3, 2, 1] = np.nan
    elif kind == "huge":
        boxes[3, 2, 2] = 2.0 ** 20 + 1
    elif kind == "index":
        keep_idx[3, 0, 1] = BP
    else:
        keep_cnt[3, 0] = KCAP + 1
    still = (boxes, scores, keep_idx, keep_cnt)
    want = ms.propagate(fsum, PP, HP, WP, *still, top=4, reach=2)
    good = ms.propagate(fsum, PP, HP, WP, *propagate_case()[1:], top=4, reach=2)
    assert want[4] and not good[4] and not bits_equal(want[0], good[0])
    # frame 3, class 0: the entries 0 (the whole image) and 1 (the degenerate box) move without the bad value, not with it
    for di, delta in enumerate(ms.deltas(2)):
        for j in {"nan": (0,), "huge": (0,), "index": (1,), "count": (0, 1, 2, 3)}[kind]:
            assert np.isnan(want[0][0, di * 4 + j, 3 + delta]).all() and want[3][0, di * 4 + j, 3 + delta] == ms.INT32_MIN
            assert abs(delta) > 1 or j > 1 or np.isfinite(good[0][0, di * 4 + j, 3 + delta]).all()
    ts = tuple(g(x) for x in still)
    cx = _lib.Context()
    try:
        with pytest.raises(ValueError):
            ops.propagate_detections(motion_of(fsum), ts, top=4, reach=2, ctx=cx)
        out = ops.propagate_detections(motion_of(fsum), ts, top=4, reach=2, sync=False, ctx=cx)
        with pytest.raises(ValueError) as err:
            cx.sync()
        assert 'propagate_boxes' in str(err.value)
        assert_prop(tuple(out[k].cpu().numpy() for k in PROP_KEYS), want)
        cx.sync()                                                 # the latch is cleared ...
        out = ops.propagate_detections(motion_of(fsum), tuple(g(x) for x in propagate_case()[1:]), top=4, reach=2, ctx=cx)
        assert_prop(tuple(out[k].cpu().numpy() for k in PROP_KEYS), good)          # ... and the context works
    finally:
        cx.close()


# d. -------------------------------------------------------------------------------------------------------------------
def test_argument_errors():
    import torch
    from vdetlib_amd import _lib, ops
    fsum, boxes, scores, keep_idx, keep_cnt = propagate_case()
    images = np.random.RandomState(9400).randint(0, 256, size=(2, 24, 40, 3)).astype(np.uint8)
    ti = g(images)
    tb, ts, tk, tc = (g(x) for x in (boxes, scores, keep_idx, keep_cnt))
    still = (tb, ts, tk, tc)
    Hb, Wb = ms.grid_of(HP, WP, PP)
    cx = _lib.Context()
    try:
        cx.set_timing(2)
        m = ops.motion_field(ti, 8, 2, ctx=cx)
        assert cx.last_timing()['other'][1] == 1                 # the two launches are ONE timed span, under 'other'
        mo = motion_of(fsum)
        ops.propagate_detections(mo, still, top=2, ctx=cx)
        assert cx.last_timing()['other'][1] == 1
        for fn in (lambda: ops.motion_field(ti, 12, 2, ctx=cx), lambda: ops.motion_field(ti, 64, 2, ctx=cx),
                   lambda: ops.motion_field(ti, 8, 0, ctx=cx), lambda: ops.motion_field(ti, 8, 17, ctx=cx),
                   lambda: ops.motion_field(ti.float(), ctx=cx), lambda: ops.motion_field(ti[:, :, ::2], ctx=cx),
                   lambda: ops.motion_field(ti.cpu(), ctx=cx), lambda: ops.motion_field(ti[..., :2], ctx=cx),
                   lambda: ops.motion_field(torch.empty((1, 32768, 8, 3), dtype=torch.uint8, device='cuda'), ctx=cx),
                   lambda: ops.propagate_detections(mo, still, top=0, ctx=cx),
                   lambda: ops.propagate_detections(mo, still, top=KCAP + 1, ctx=cx),
                   lambda: ops.propagate_detections(mo, still, top=2, reach=0, ctx=cx),
                   lambda: ops.propagate_detections(mo, still, top=2, reach=17, ctx=cx),
                   lambda: ops.propagate_detections(mo, still, top=2, decay=-0.5, ctx=cx),
                   lambda: ops.propagate_detections(mo, still, top=2, decay=float('nan'), ctx=cx),
                   lambda: ops.propagate_detections(mo, still, top=2, decay=float('inf'), ctx=cx),
                   lambda: ops.propagate_detections(mo, still[:3], top=2, ctx=cx),
                   lambda: ops.propagate_detections(mo, (tb, ts, tk.long(), tc), top=2, ctx=cx),
                   lambda: ops.propagate_detections(mo, (tb, ts.double(), tk, tc), top=2, ctx=cx),
                   lambda: ops.propagate_detections(mo, (tb[:-1], ts, tk, tc), top=2, ctx=cx),
                   lambda: ops.propagate_detections(mo, (tb, ts, tk, tc[:, :-1]), top=2, ctx=cx),
                   lambda: ops.propagate_detections(mo, (tb, ts, tk, tc.cpu()), top=2, ctx=cx),
                   lambda: ops.propagate_detections(dict(mo, block=12), still, top=2, ctx=cx),
                   lambda: ops.propagate_detections(dict(mo, size=(HP + 8, WP)), still, top=2, ctx=cx),
                   lambda: ops.propagate_detections(dict(mo, fsum=mo['fsum'].long()), still, top=2, ctx=cx),
                   lambda: ops.propagate_detections(dict(mo, fsum=mo['fsum'][:, :-1]), still, top=2, ctx=cx),
                   lambda: ops.propagate_detections(mo['fsum'], still, top=2, ctx=cx),
                   lambda: ops.propagate_detections(m, still, top=2, ctx=cx)):           # the field of another video
            with pytest.raises(ValueError):
                fn()
        # 2*reach*top beyond nms_tracks' list limit, with lists wide enough for the top
        big = (tb, ts, torch.zeros((FP, CP, 40), dtype=torch.int32, device='cuda'), tc)
        with pytest.raises(ValueError):
            ops.propagate_detections(mo, big, top=33, reach=16, ctx=cx)
        # the C-ABI refuses on its own, one value beyond every limit
        L, z = cx.lib, None
        o = tuple(x.data_ptr() for x in (m['field'], m['cost'], m['fsum']))          # (never written: every call is refused)
        mf = lambda F=2, H=24, W=40, P=8, R=2, img=ti.data_ptr(), out=o: L.vdet_motion_field(cx.h, img, F, H, W, P, R, *out)
        for kw in (dict(P=4), dict(P=12), dict(P=64), dict(R=0), dict(R=17), dict(H=32768), dict(W=32768), dict(F=0), dict(H=0), dict(img=z),
                   dict(out=(z, o[1], o[2])), dict(out=(o[0], z, o[2])), dict(out=(o[0], o[1], z)),
                   dict(F=1 << 22, H=256, W=256)):           # 4 * 2^22 * 33 * 33 > 2^31
            assert mf(**kw) == _lib.VDET_EINVAL, kw
        mt = lambda F=2, Hb=3, Wb=5, fld=o[0], out=o[2]: L.vdet_motion_table(cx.h, fld, F, Hb, Wb, out)
        for kw in (dict(F=0), dict(Hb=0), dict(Wb=0), dict(Hb=4097), dict(Wb=4097), dict(fld=z), dict(out=z), dict(F=1 << 26)):
            assert mt(**kw) == _lib.VDET_EINVAL, kw
        po = tuple(x.data_ptr() for x in (tb, ts, tk, tc))                            # (outputs: never written either)
        pb = lambda F=FP, Hb=Hb, Wb=Wb, P=PP, H=HP, W=WP, B=BP, C=CP, kcap=KCAP, top=2, reach=3, decay=1.0, fs=mo['fsum'].data_ptr(), \
            bx=tb.data_ptr(), out=po: L.vdet_propagate_boxes(cx.h, fs, F, Hb, Wb, P, H, W, B, C, bx, ts.data_ptr(), tk.data_ptr(), kcap,
                                                             tc.data_ptr(), top, reach, decay, *out)
        for kw in (dict(top=0), dict(top=KCAP + 1), dict(reach=0), dict(reach=17), dict(top=33, kcap=40, reach=16), dict(B=32768),
                   dict(decay=-1.0), dict(decay=float('nan')), dict(decay=float('inf')), dict(P=12), dict(Hb=Hb + 1), dict(Wb=Wb - 1),
                   dict(H=32768), dict(F=0), dict(C=0), dict(B=0), dict(kcap=0), dict(fs=z), dict(bx=z), dict(out=(z,) + po[1:]),
                   dict(C=1 << 25, top=5, reach=16)):        # C*T*F = 2^25 * 160 * 7 > 2^31
            assert pb(**kw) == _lib.VDET_EINVAL, kw
        assert sum(n for _, n in cx.last_timing().values()) == 0, "an argument error launched a kernel"
        # the context still works
        got = ops.propagate_detections(mo, still, top=2, ctx=cx)
        assert_prop(tuple(got[k].cpu().numpy() for k in PROP_KEYS), ms.propagate(fsum, PP, HP, WP, boxes, scores, keep_idx, keep_cnt, top=2))
    finally:
        cx.close()


# e. -------------------------------------------------------------------------------------------------------------------
def test_prep_cache_is_left_alone():
    import synth
    import torch
    from vdetlib_amd import _lib, ops
    boxes, scores = synth.coherent_video(7433, 12, 120, 3, frac=True)
    tb, ts = g(boxes), g(scores)
    images = np.random.RandomState(9500).randint(0, 256, size=(3, 37, 53, 3)).astype(np.uint8)
    fsum, *still = propagate_case()
    cx = _lib.Context(torch.cuda.current_device())
    try:
        cx.set_cache(True)
        run = lambda: tuple(x.cpu().numpy() for x in ops.nms_track_volume(tb, ts, max_tracks=4, ctx=cx))
        first = run()
        m = ops.motion_field(g(images), 8, 2, ctx=cx)
        p = ops.propagate_detections(motion_of(fsum), tuple(g(x) for x in still), top=2, ctx=cx)
        second = run()
    finally:
        cx.close()
    for a, b in zip(first, second):
        assert a.shape == b.shape and np.array_equal(a, b, equal_nan=True)
    for k, want in zip(FIELD_KEYS, ms.motion_field(images, 8, 2)):
        assert np.array_equal(m[k].cpu().numpy(), want)
    assert_prop(tuple(p[k].cpu().numpy() for k in PROP_KEYS), ms.propagate(fsum, PP, HP, WP, *still, top=2))


# f. -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", (0, 2))
def test_end_to_end_on_a_planted_scene(k):
    """nms_volume -> motion_field -> propagate_detections -> nms_tracks(still=...) equals the spec + oracle.nms lists; the frame
    the detector missed gains its detection; the class's AP with propagation is strictly above the AP without it (the same
    comparison on the spec: test_motion_cpu.py)"""
    from test_nms_tracks_cpu import outputs_equal
    from vdetlib_amd import ops
    from vdetlib_amd import eval as ev
    H, W, P, R = mc.SCENES[k][0], mc.SCENES[k][1], mc.SCENES[k][6], mc.SCENES[k][7]
    images, truth = mc.planted(k)
    boxes, scores, keep_idx, keep_cnt = mc.detector(k)
    tb, ts = g(boxes), g(scores)
    idx, cnt = ops.nms_volume(tb, ts, mc.THRESH)
    assert np.array_equal(idx.cpu().numpy(), keep_idx) and np.array_equal(cnt.cpu().numpy(), keep_cnt)
    still = (tb, ts, idx, cnt)
    m = ops.motion_field(g(images), block=P, radius=R)
    for name, want in zip(FIELD_KEYS, mc.field_of(k)):
        assert np.array_equal(m[name].cpu().numpy(), want), name
    p = ops.propagate_detections(m, still, top=mc.TOP, reach=mc.REACH)
    prop, lists = mc.pipeline_spec(k)
    assert_prop(tuple(p[key].cpu().numpy() for key in PROP_KEYS), prop)
    out = ops.nms_tracks(p['tracks'], p['ntracks'], p['score'], still=still, thresh=mc.THRESH)
    assert outputs_equal({key: v.cpu().numpy() for key, v in out.items()}, lists)
    dets = ev.detections_from_tracks(mc.VIDEO, lists['tracks'], lists['ntracks'], lists['score'])
    assert mc.best_iou_on(mc.MID, dets, truth) >= 0.5
    assert mc.best_iou_on(mc.MID, ev.detections_from_keep_lists(mc.VIDEO, boxes, scores, keep_idx, keep_cnt), truth) < 0.5
    table = mc.gt_table(k)
    plain, moved = ops.DetEvaluator(table), ops.DetEvaluator(table)
    plain.add_keep_lists(mc.VIDEO, tb, ts, idx, cnt)
    moved.add_detections(mc.VIDEO, out)
    ap_plain, ap_moved = plain.compute()[0][1], moved.compute()[0][1]
    want_plain, want_moved = mc.host_aps(k)
    assert ap_moved > ap_plain and abs(ap_plain - want_plain) < 1e-12 and abs(ap_moved - want_moved) < 1e-12
