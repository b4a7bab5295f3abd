"""Seeded videos for the tests of the pixel tracker's template update (CPU: tests/pixtrack_adapt_spec.py against planted
positions; GPU: the device against that spec).  Grey frames (three equal channels, so the luma is the grey value) of 96 x 128.

The planted walk: a square object of ``obj`` = grid * pitch pixels that moves by whole pitches -- ``MX[pitch]`` cells a frame
along x, one cell every second frame along y -- over a background of noise that is fixed to the image.

  morph      the object's texture goes linearly from one random texture to another over the video: the anchor's template loses
             confidence frame by frame; only an updated template follows it to the end
  passenger  the object keeps its (low-contrast) texture; a foreign full-contrast patch rides on its right half for RIDE frames
             and then stays where it is, on top of the static background, while the object moves on to the left: a template that
             absorbed the patch stays with it
  shrink     pixtrack_scale_cases' shrinking object: the scale search wins at levels -1, 0 and +1
"""
import numpy as np

import pixtrack_scale_cases as sc

F, H, W = 24, 96, 128
MX = {1: 2, 2: 1}                       # cells a frame along x, by pitch
SIZES = ((32, 8, 32), (8, 2, 16))       # (grid, radius, object side): the CPU tests' two
GPU_SIZES = SIZES + ((64, 16, 64), (12, 3, 24), (4, 1, 8))
RIDE_FROM, RIDE = 6, 8                  # the passenger rides on frames RIDE_FROM .. RIDE_FROM + RIDE - 1
_cache = {}


def grey(planes):
    return np.repeat(np.asarray(planes, dtype=np.uint8)[..., None], 3, axis=-1)


def walk(S, obj, frames=F, leftward=False):
    """positions [frames,2] of the object's 0-based (x1, y1)"""
    pitch = obj // S
    assert obj == S * pitch and pitch in MX
    dx, span = MX[pitch] * pitch, MX[pitch] * pitch * (frames - 1)
    assert 8 + span + obj <= W and 8 + pitch * ((frames - 1) // 2) + obj <= H
    pos = np.zeros((frames, 2), np.int64)
    for f in range(frames):
        pos[f] = (8 + span - dx * f if leftward else 8 + dx * f, 8 + pitch * (f // 2))
    return pos


def anchor_of(pos, obj, f=0):
    """([[frame]], [[box]]) of the 1-based anchor on frame f"""
    x, y = (int(v) for v in pos[f])
    return np.array([[f + 1]], np.int32), np.array([[[x + 1, y + 1, x + obj, y + obj]]], np.float32)


def errors(rows, pos):
    """per frame max(|x1 error|, |y1 error|) of the rows [F,5] (1-based) against the planted positions; NaN where no row"""
    return np.maximum(np.abs(rows[:, 0] - (pos[:, 0] + 1)), np.abs(rows[:, 1] - (pos[:, 1] + 1)))


def morph_video(S, R, obj, seed=8100, frames=F):
    """-> (images uint8 [frames,H,W,3], positions [frames,2]); computed once and shared (do not modify)"""
    key = ('morph', S, R, obj, seed, frames)
    if key not in _cache:
        rng = np.random.RandomState(seed + S)
        bg = rng.randint(0, 256, size=(H, W))
        t0 = rng.randint(0, 256, size=(obj, obj)).astype(np.float64)
        t1 = rng.randint(0, 256, size=(obj, obj)).astype(np.float64)
        pos = walk(S, obj, frames)
        planes = np.repeat(bg[None], frames, axis=0)
        for f in range(frames):
            t = f / float(frames - 1)
            x, y = pos[f]
            planes[f, y:y + obj, x:x + obj] = np.rint((1 - t) * t0 + t * t1)
        _cache[key] = (grey(planes), pos)
    return _cache[key]


def passenger_video(S, R, obj, seed=8200, frames=F):
    """-> (images uint8 [frames,H,W,3], positions [frames,2]); computed once and shared (do not modify)"""
    key = ('passenger', S, R, obj, seed, frames)
    if key not in _cache:
        rng = np.random.RandomState(seed + S)
        bg = rng.randint(0, 256, size=(H, W))
        tex = rng.randint(96, 161, size=(obj, obj))
        patch = rng.randint(0, 256, size=(obj, obj // 2))
        pos = walk(S, obj, frames, leftward=True)
        planes = np.repeat(bg[None], frames, axis=0)
        for f in range(frames):
            x, y = pos[f]
            planes[f, y:y + obj, x:x + obj] = tex
            if f >= RIDE_FROM:
                px, py = pos[min(f, RIDE_FROM + RIDE - 1)]            # rides, then stays where it was last
                planes[f, py:py + obj, px + obj // 2:px + obj] = patch
        _cache[key] = (grey(planes), pos)
    return _cache[key]


def passenger_guard(S, R, obj, min_conf=0.7):
    """the drift_conf for passenger_video(S, R, obj), read from the spec's own trace of the fixed template anchored on frame 1:
    half way between the largest c0 of a window the passenger rides on and the smallest c0 before it came"""
    key = ('guard', S, R, obj, min_conf)
    if key not in _cache:
        import pixtrack_adapt_spec as pa
        images, pos = passenger_video(S, R, obj)
        fr, bx = anchor_of(pos, obj)
        traces = {}
        rows = pa.track_pixels(images, fr, bx, None, grid=S, radius=R, min_conf=min_conf, traces=traces)[0][0, 0]
        assert np.isfinite(rows).all()
        c0 = np.array([1.0] + [traces[(0, 0)][f][4] for f in range(1, F)])
        ridden, before = c0[RIDE_FROM:RIDE_FROM + RIDE].max(), c0[:RIDE_FROM].min()
        assert ridden < before
        _cache[key] = (float(ridden + before) / 2, float(ridden), float(before))
    return _cache[key][0]


GS, GR, GOBJ = 8, 2, 16
GB, GC = 4, 2
GREEDY = dict(nms_thres=0.3, thres=0.3, max_tracks=3, grid=GS, radius=GR, min_conf=0.8)
GUPDATE = dict(update=128, update_conf=0.8, drift_conf=0.0)


def greedy_volume():
    """The morph video at (GS, GR, GOBJ) with proposals, B = 4: 0 the object's true box, 1 the true box jittered by (1, 1),
    2-3 two fixed boxes on the static background (distractors).  Scores, class 0: the true box on frame 1 0.99, the other
    object proposals in (0.5, 0.9), the distractors in (0.31, 0.49); class 1: the true box on frame 13 0.95, the other object
    proposals in (0.5, 0.8), the distractors below the threshold.  A fixed template loses the object on the way, so the object's
    proposals beyond its end stay and the best of them is the second anchor; the updated template follows the object to the
    end, every object proposal goes, and the second anchor is a distractor.
    -> (images, boxes [F,4,4], scores [F,4,2], positions); computed once and shared (do not modify)"""
    if 'greedy' not in _cache:
        images, pos = morph_video(GS, GR, GOBJ)
        rng = np.random.RandomState(8400)
        boxes = np.zeros((F, GB, 4), np.float32)
        for f in range(F):
            x, y = (int(v) for v in pos[f])
            boxes[f, 0] = [x + 1, y + 1, x + GOBJ, y + GOBJ]
            boxes[f, 1] = boxes[f, 0] + 1
            boxes[f, 2] = [100, 70, 115, 85]
            boxes[f, 3] = [20, 72, 35, 87]
        scores = np.zeros((F, GB, GC), np.float32)
        scores[:, :2, 0] = rng.uniform(0.5, 0.9, size=(F, 2))
        scores[:, 2:, 0] = rng.uniform(0.31, 0.49, size=(F, 2))
        scores[0, 0, 0] = 0.99
        scores[:, :2, 1] = rng.uniform(0.5, 0.8, size=(F, 2))
        scores[:, 2:, 1] = rng.uniform(0.05, 0.25, size=(F, 2))
        scores[12, 0, 1] = 0.95
        _cache['greedy'] = (images, boxes, scores, pos)
    return _cache['greedy']


def shrink_scene():
    """pixtrack_scale_cases.scene('shrink') cut to 96 x 128 around the object: (images uint8 [12,96,128,3], true boxes [12,4])"""
    if 'shrink' not in _cache:
        images, truth = sc.scene('shrink')
        y0, x0 = 40, 50
        cut = np.ascontiguousarray(images[:, y0:y0 + H, x0:x0 + W])
        _cache['shrink'] = (cut, truth - np.array([x0, y0, x0, y0]))
    return _cache['shrink']
