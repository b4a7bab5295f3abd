"""-m gpu: ops.top_anchors (csrc/topanchor_kernels.hpp), the array form of protocol.top_detections / frame_top_detections.
The specification is the few lines of numpy in `want_video`: per class, mask the candidates, a STABLE argsort of the
negated scores over the flat index f*B + b (-0.0 and +0.0 compare equal), cut at T.  All four outputs are compared exactly,
scores and boxes on their bits.  The kernels have one path for every T; the shapes walk the sizes at which the row walk
changes: kTopaRows = 256 rows per segment (a wave), 4 segments per counting workgroup (1024 rows), 16 per histogram
workgroup (4096 rows), 64 classes per class tile."""
import numpy as np
import pytest

import synth

pytestmark = pytest.mark.gpu

ROWS = 256          # kTopaRows (csrc/topanchor_kernels.hpp): the kernel's row-chunk size


def g(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def make(seed, F, B, C):
    rng = np.random.RandomState(seed)
    boxes = (rng.rand(F, B, 4) * 500).astype(np.float32) + np.float32(0.25)
    scores = rng.randn(F, B, C).astype(np.float32)
    return boxes, scores


def select(s, T, thr):
    """flat indices of the T best candidates of the score column s, in slot order"""
    mask = ~np.isnan(s)
    if thr is not None:
        mask &= s > np.float32(thr)
    idx = np.nonzero(mask)[0]
    return idx[np.argsort(-s[idx], kind='stable')][:T]


def want_video(boxes, scores, T, thr=None):
    F, B, C = scores.shape
    fr, ix = np.zeros((C, T), np.int32), np.full((C, T), -1, np.int32)
    bx, sc = np.zeros((C, T, 4), np.float32), np.zeros((C, T), np.float32)
    fb, fs = boxes.reshape(F * B, 4), scores.reshape(F * B, C)
    for c in range(C):
        sel = select(fs[:, c], T, thr)
        n = len(sel)
        fr[c, :n], ix[c, :n], bx[c, :n], sc[c, :n] = sel // B + 1, sel % B, fb[sel], fs[sel, c]
    return fr, bx, sc, ix


def want_frame(boxes, scores, top, thr=None):
    F, B, C = scores.shape
    parts = []
    for f in range(F):
        fr, bx, sc, ix = want_video(boxes[f:f + 1], scores[f:f + 1], top, thr)
        fr[fr > 0] += f
        parts.append((fr, bx, sc, ix))
    return tuple(np.concatenate([p[k] for p in parts], 1) for k in range(4))


def check(got, want, what):
    fr, bx, sc, ix = (x.cpu().numpy() for x in got)
    assert fr.dtype == np.int32 and ix.dtype == np.int32 and bx.dtype == np.float32 and sc.dtype == np.float32
    assert fr.shape == want[0].shape and bx.shape == want[1].shape, what
    assert np.array_equal(fr, want[0]), (what, 'frames')
    assert np.array_equal(ix, want[3]), (what, 'index')
    assert np.array_equal(bits(sc), bits(want[2])), (what, 'scores')
    assert np.array_equal(bits(bx), bits(want[1])), (what, 'boxes')


def run_video(boxes, scores, T, thr=None, what=None):
    from vdetlib_amd import ops
    check(ops.top_anchors(g(boxes), g(scores), T, score_thresh=thr), want_video(boxes, scores, T, thr), what)


SHAPES = [(1, 1, 1), (3, 5, 1), (7, 129, 3), (2, 300, 65), (5, 70, 130),
          (1, ROWS - 1, 2), (1, ROWS, 2), (1, ROWS + 1, 2),          # one below, at, one above the row chunk
          (3, 4 * ROWS // 3 + 1, 2),                                   # past a counting workgroup (1024 rows)
          (1, 16 * ROWS + 3, 3)]                                       # past a histogram workgroup (4096 rows)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_video_mode_equals_the_numpy_rule(shape):
    F, B, C = shape
    boxes, scores = make(9000 + F * B + C, F, B, C)
    for T in (1, 2, 10, 64, 65, 1024, F * B + 3):
        if T <= 1024:
            run_video(boxes, scores, T, what=(shape, T))


def test_winners_all_in_one_chunk():
    F, B, C = 2, ROWS, 3
    boxes, scores = make(9100, F, B, C)
    last = scores.copy()
    last[1] += 100                  # every winner in the second chunk
    first = scores.copy()
    first[0] += 100                 # ... in the first
    for s in (last, first):
        for T in (1, 10, 65, ROWS, ROWS + 5):
            run_video(boxes, s, T, what=T)


def test_ties_by_flat_index():
    F, B, C = 3, 200, 2             # 600 rows: three chunks
    boxes, _ = make(9200, F, B, C)
    # all scores equal: slots are flat indices 0..T-1 across a chunk boundary
    eq = np.full((F, B, C), 0.5, np.float32)
    from vdetlib_amd import ops
    for T in (1, ROWS - 1, ROWS + 1, 600, 1024):
        got = ops.top_anchors(g(boxes), g(eq), T)
        flat = (got[0].cpu().numpy().astype(np.int64) - 1) * B + got[3].cpu().numpy()
        n = min(T, F * B)
        assert np.array_equal(flat[:, :n], np.tile(np.arange(n), (C, 1))) and (got[0].cpu().numpy()[:, n:] == 0).all()
        check(got, want_video(boxes, eq, T), T)
    # a tie group that straddles the cut AND a chunk boundary: 5 winners, then 40 equal scores on rows 240..279
    rng = np.random.RandomState(9201)
    s = rng.rand(F, B, C).astype(np.float32) * 0.1
    flat = s.reshape(F * B, C)
    flat[240:280] = 0.7
    flat[[3, 300, 599, 260 + 40, 17]] = 0.9
    for T in (5, 6, 20, 21, 22, 44, 45, 46):        # the cut before, inside (both sides of row 256) and behind the group
        run_video(boxes, s, T, what=T)
    # -0.0 and +0.0 are one score: flat index decides, the bits of each are kept
    z = np.full((F, B, C), -1.0, np.float32)
    zf = z.reshape(F * B, C)
    zf[[5, 7, 300], 0] = [-0.0, 0.0, -0.0]
    zf[[2, 4], 1] = [0.0, -0.0]
    got = ops.top_anchors(g(boxes), g(z), 4)
    idx = ((got[0].cpu().numpy().astype(np.int64) - 1) * B + got[3].cpu().numpy())
    assert idx[0, :3].tolist() == [5, 7, 300] and idx[1, :2].tolist() == [2, 4]
    assert bits(got[2].cpu().numpy())[0, :3].tolist() == [0x80000000, 0, 0x80000000]
    check(got, want_video(boxes, z, 4), 'zeros')


def test_inf_nan_and_threshold():
    from vdetlib_amd import ops
    F, B, C = 2, 150, 4
    boxes, scores = make(9300, F, B, C)
    scores[:, :, 1] = -np.inf                               # a column of all -inf
    scores[:, :, 2] = np.nan                                # a whole NaN class
    flat = scores.reshape(F * B, C)
    flat[[0, 17, 255, 256, 299], 0] = np.nan                # NaN scattered
    flat[[4, 9], 3] = -np.inf
    for T in (1, 10, 300, 305):
        run_video(boxes, scores, T, what=('plain', T))
        run_video(boxes, scores, T, thr=-np.inf, what=('-inf', T))
    fr = ops.top_anchors(g(boxes), g(scores), 10)[0].cpu().numpy()
    assert (fr[1] > 0).all() and (fr[2] == 0).all()          # without a threshold -inf is a candidate, NaN never
    fr = ops.top_anchors(g(boxes), g(scores), 10, score_thresh=-np.inf)[0].cpu().numpy()
    assert (fr[1] == 0).all()
    # a threshold exactly equal to some scores: strict
    t = np.float32(0.25)
    flat[[1, 50, 280], 0] = t
    flat[[2, 51], 0] = np.nextafter(t, np.float32(1))
    for T in (3, 300):
        run_video(boxes, scores, T, thr=float(t), what=('thr', T))
    got = ops.top_anchors(g(boxes), g(scores), 300, score_thresh=float(t))
    sc, fr = got[2].cpu().numpy()[0], got[0].cpu().numpy()[0]
    assert (sc[fr > 0] > t).all() and (sc[fr > 0] == np.nextafter(t, np.float32(1))).sum() == 2


@pytest.mark.parametrize("shape", [(4, 5, 2), (3, 130, 65)], ids=lambda s: "x".join(map(str, s)))
def test_frame_mode(shape):
    from vdetlib_amd import ops
    F, B, C = shape
    boxes, scores = make(9400 + B, F, B, C)
    scores[1, :, 0] = 0.5                                    # ties inside a frame
    scores[2, 1:, 1] = np.nan                                # a frame with one candidate
    scores[0, :, C - 1] = np.nan                             # ... with none
    for top in (1, 3, 128):
        got = ops.top_anchors(g(boxes), g(scores), top, mode='frame')
        assert tuple(got[0].shape) == (C, F * top)
        check(got, want_frame(boxes, scores, top), top)
    top = min(B + 2, 128)                                    # more than B where the limit of 128 allows it
    check(ops.top_anchors(g(boxes), g(scores), top, mode='frame', score_thresh=-0.3), want_frame(boxes, scores, top, -0.3), 'thr')
    fr = ops.top_anchors(g(boxes), g(scores), 3, mode='frame')[0].cpu().numpy()
    assert fr[0, 3:6].tolist() == [2, 2, 2] and fr[1, 6:9].tolist() == [3, 0, 0] and fr[C - 1, 0:3].tolist() == [0, 0, 0]


def test_reference_recorded_output(proto_golden):
    from vdetlib_amd import ops
    from vdetlib_amd.utils import protocol
    case = synth.proto_case()
    det, F, B = case['det'], case['F'], case['B']
    dets = det['detections']
    assert len(dets) == F * B and all(d['frame'] == i // B + 1 for i, d in enumerate(dets))      # frame-major, not ragged
    boxes = np.array([d['bbox'] for d in dets], np.float32).reshape(F, B, 4)
    scores = np.array([[s['score'] for s in d['scores']] for d in dets], np.float32).reshape(F, B, -1)
    assert np.array_equal(scores.astype(np.float64).ravel(), [s['score'] for d in dets for s in d['scores']])

    def hashes(frames, index, c):
        return [protocol.bbox_hash(det['video'], int(f), dets[(int(f) - 1) * B + int(b)]['bbox'])
                for f, b in zip(frames[c], index[c]) if f > 0]
    gold = proto_golden['protocol_misc']
    fr, _, _, ix = (x.cpu().numpy() for x in ops.top_anchors(g(boxes), g(scores), 7))
    assert hashes(fr, ix, 2) == gold['top_detections']
    fr, _, _, ix = (x.cpu().numpy() for x in ops.top_anchors(g(boxes), g(scores), 3, mode='frame'))
    assert sorted(hashes(fr, ix, 1)) == gold['frame_top_detections']


def test_first_slot_is_the_greedy_trackers_first_anchor():
    from vdetlib_amd import ops
    F, B, C = 6, 300, 8
    boxes, _ = synth.video(9500, F, B, C)
    scores = synth.tie_free_scores(np.random.RandomState(9501), F * B * C, "perm").reshape(F, B, C).astype(np.float32)
    tb, ts = g(boxes), g(scores)
    anchors = ops.nms_track_volume(tb, ts, max_tracks=2)[3].cpu().numpy()
    fr, bx, sc, ix = (x.cpu().numpy() for x in ops.top_anchors(tb, ts, 1))
    assert np.array_equal(anchors[:, 0, 0], fr[:, 0].astype(np.float32))
    assert np.array_equal(anchors[:, 0, 1], ix[:, 0].astype(np.float32))
    assert np.array_equal(bits(anchors[:, 0, 2]), bits(sc[:, 0]))
    assert np.array_equal(bx[:, 0], boxes[fr[:, 0] - 1, ix[:, 0]])


def test_errors_before_any_launch():
    import torch
    from vdetlib_amd import _lib, ops
    boxes, scores = make(9600, 3, 5, 2)
    tb, ts = g(boxes), g(scores)
    cx = _lib.Context()
    try:
        ops.top_anchors(tb, ts, 2, ctx=cx)
        cases = [lambda: ops.top_anchors(tb.double(), ts, 2, ctx=cx), lambda: ops.top_anchors(tb, ts.double(), 2, ctx=cx),
                 lambda: ops.top_anchors(tb, ts, 0, ctx=cx), lambda: ops.top_anchors(tb, ts, -1, ctx=cx),
                 lambda: ops.top_anchors(tb, ts, 1025, ctx=cx), lambda: ops.top_anchors(tb, ts, 129, mode='frame', ctx=cx),
                 lambda: ops.top_anchors(tb[:2], ts, 2, ctx=cx), lambda: ops.top_anchors(tb, ts[:, :4], 2, ctx=cx),
                 lambda: ops.top_anchors(tb[..., :3], ts, 2, ctx=cx), lambda: ops.top_anchors(tb, ts[0], 2, ctx=cx),
                 lambda: ops.top_anchors(tb, ts.cpu(), 2, ctx=cx), lambda: ops.top_anchors(tb.cpu(), ts, 2, ctx=cx),
                 lambda: ops.top_anchors(tb, ts, 2, mode='frame', frame_off=[0, 1, 3], ctx=cx),
                 lambda: ops.top_anchors(tb, ts, 2, mode='clip', ctx=cx),
                 lambda: ops.top_anchors(tb, ts, 2, frame_off=[0, 2], ctx=cx),
                 lambda: ops.top_anchors(tb, ts, 2, frame_off=[0, 2, 2, 3], ctx=cx)]
        if torch.cuda.device_count() > 1:
            cases.append(lambda: ops.top_anchors(tb, ts.to('cuda:1'), 2, ctx=cx))
        cx.set_timing(2)                 # accumulate the launches of every call until they are read
        for k, fn in enumerate(cases):
            with pytest.raises(ValueError):
                fn()
                pytest.fail("case %d raised nothing" % k)
        # the C-ABI's own checks (a caller that bypasses ops): an error code, nothing enqueued
        lib = cx.lib
        outs = [torch.empty(2 * 2 * 4, dtype=torch.float32, device='cuda') for _ in range(4)]
        ptrs = [o.data_ptr() for o in outs]
        for top, mode in ((0, 0), (1025, 0), (129, 1), (2, 2)):
            assert lib.vdet_top_anchors(cx.h, tb.data_ptr(), ts.data_ptr(), 3, 5, 2, top, mode, 0, 0.0, None, 0, *ptrs) == _lib.VDET_EINVAL
        assert sum(n for _, n in cx.last_timing().values()) == 0, "a refused call launched something"
        ops.top_anchors(tb, ts, 2, ctx=cx)
        assert sum(n for _, n in cx.last_timing().values()) == 1      # (the counter does see this call's launches)
        cx.set_timing(0)
        check(ops.top_anchors(tb, ts, 2, ctx=cx), want_video(boxes, scores, 2), 'after the errors')
    finally:
        cx.close()


def test_async_call_never_waits_and_leaves_the_prep_cache_alone():
    from vdetlib_amd import _lib, ops
    F, B, C = 5, 300, 3
    boxes, scores = synth.video(9700, F, B, C)
    tb, ts = g(boxes), g(scores)
    want = want_video(boxes, scores, 10)
    cx = _lib.Context()
    try:
        cx.set_async(True)
        cx.set_cache(True)
        ref = [x.cpu().numpy() for x in ops.nms_track_volume(tb, ts, ctx=cx)]
        first = ops.top_anchors(tb, ts, 10, ctx=cx)
        before = cx.query(8)
        second = ops.top_anchors(tb, ts, 10, sync=False, ctx=cx)
        third = ops.top_anchors(tb, ts, 3, mode='frame', sync=False, ctx=cx)
        assert cx.query(8) == before, "an asynchronous top_anchors call waited for the device"
        cx.sync()
        assert cx.query(8) == before + 1
        check(first, want, 'first')
        check(second, want, 'second')
        check(third, want_frame(boxes, scores, 3), 'frame')
        again = [x.cpu().numpy() for x in ops.nms_track_volume(tb, ts, ctx=cx)]
        for a, b in zip(ref, again):
            assert np.array_equal(a, b, equal_nan=True)
    finally:
        cx.close()
