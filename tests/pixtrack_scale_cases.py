"""Seeded videos for the scaled pixel tracker's tests (CPU: the spec against known boxes; GPU: the device against the spec).

The planted scene: a square object whose texture is a sum of a few seeded sinusoids DEFINED ON THE UNIT SQUARE and rendered
into the object's box at its current size, so the object really grows and shrinks; the background is another smooth texture,
fixed to the image.  F = 12 frames of 200 x 240.  Frame f: half-side hs(f), centre (100 + 3f, 90 + f); the true box is
columns cx-hs .. cx+hs-1, rows cy-hs .. cy+hs-1 (0-based), side 2 hs."""
import numpy as np

import pixtrack_cases as pc

F, H, W = 12, 200, 240
S, R = 32, 8
KINDS = {'grow': lambda f: 20 + f, 'shrink': lambda f: 32 - f, 'const': lambda f: 24}


def _waves(seed, n, fmin, fmax):
    rng = np.random.RandomState(seed)
    return (rng.uniform(fmin, fmax, size=n) * rng.choice([-1.0, 1.0], size=n), rng.uniform(fmin, fmax, size=n),
            rng.uniform(0, 2 * np.pi, size=n), rng.uniform(0.5, 1.0, size=n))


def _texture(waves, u, v):
    """uint8 plane of the sinusoid sum at the points (u, v) (arrays of one shape): mean 128, full swing"""
    fx, fy, ph, am = waves
    t = sum(a * np.sin(2 * np.pi * (x * u + y * v) + p) for x, y, p, a in zip(fx, fy, ph, am)) / am.sum()
    return np.clip(np.rint(128 + 127 * t), 0, 255).astype(np.uint8)


def background(seed, h=H, w=W):
    y, x = np.mgrid[0:h, 0:w]
    return _texture(_waves(seed, 4, 0.5, 2.0), x / float(w), y / float(h))


def true_box(kind, f, cx0=100, cy0=90):
    """0-based inclusive (x1, y1, x2, y2) of the object on frame f"""
    hs = KINDS[kind](f)
    cx, cy = cx0 + 3 * f, cy0 + f
    return (cx - hs, cy - hs, cx + hs - 1, cy + hs - 1)


def paint(plane, waves, box):
    """render the unit-square texture into ``box`` (0-based inclusive, inside the plane) at the box's size"""
    x1, y1, x2, y2 = box
    w, h = x2 - x1 + 1, y2 - y1 + 1
    v, u = np.mgrid[0:h, 0:w]
    plane[y1:y2 + 1, x1:x2 + 1] = _texture(waves, (u + 0.5) / w, (v + 0.5) / h)


def grey(plane):
    return np.repeat(np.asarray(plane, dtype=np.uint8)[..., None], 3, axis=-1)


_scenes = {}


def scene(kind, seed=5100):
    """-> (images uint8 [F,H,W,3], true boxes [F,4] int, 0-based inclusive); computed once and shared (do not modify)"""
    if (kind, seed) not in _scenes:
        waves = _waves(seed, 5, 1.0, 4.0)
        bg = background(seed + 1)
        planes = np.repeat(bg[None], F, axis=0)
        truth = np.zeros((F, 4), np.int64)
        for f in range(F):
            truth[f] = true_box(kind, f)
            paint(planes[f], waves, truth[f])
        _scenes[(kind, seed)] = (grey(planes), truth)
    return _scenes[(kind, seed)]


def anchor_of(truth, f=0):
    """([[frame]], [[box]]) of the 1-based anchor on frame f"""
    return np.array([[f + 1]], np.int32), np.array([[truth[f] + 1]], np.float32)


def largest_error(rows, truth):
    """the largest coordinate error of the rows [F,5] (1-based) against the true boxes [F,4] (0-based), over the frames with a row"""
    on = np.isfinite(rows[:, 0])
    return float(np.abs(rows[on, :4] - (truth[on] + 1)).max())


# ---------------------------------------------------------------------------------------------------------------------
# the mixed [3,5] slot table: one video per (grid, radius), every kind of slot in one call
# ---------------------------------------------------------------------------------------------------------------------
LEAVES = pc.LEAVES        # the leaver's chain ends on this frame (pixtrack_cases' LEAVER construction)
MIXED_AT = {'grow': (30, 40), 'shrink': (130, 40), 'const': (60, 140)}      # (cx0, cy0): the three objects never overlap
_mixed = {}


def mixed_case(S, R):
    """12 frames of 200 x 240, smooth background, with (1) the growing, the shrinking and the constant object of the planted
    scene at MIXED_AT, (2) a 37 x 53 white-noise object that moves (2, 2) pixels a frame, (3) on the right pixtrack_cases'
    strip for the box that leaves the image (see LEAVER there).
    -> (images, anchor_frames [3,5], anchor_boxes [3,5,4], anchor_scores [3,5], truth {kind: [F,4]})"""
    if (S, R) not in _mixed:
        rng = np.random.RandomState(5300 + S)
        planes = np.repeat(background(5301)[None], F, axis=0)
        truth = {}
        for k, kind in enumerate(('grow', 'shrink', 'const')):
            waves = _waves(5310 + k, 5, 1.0, 4.0)
            truth[kind] = np.array([true_box(kind, f, *MIXED_AT[kind]) for f in range(F)], np.int64)
            for f in range(F):
                paint(planes[f], waves, truth[kind][f])
        images = grey(planes)
        tex = rng.randint(0, 256, size=(53, 37, 3)).astype(np.uint8)
        for f in range(F):
            images[f, 100 + 2 * f:153 + 2 * f, 118 + 2 * f:155 + 2 * f] = tex
        images[:, :, W - pc.strip_width(S, R):] = pc.leaver_strip(rng, F, H, S, R)
        fr = np.array([[0, 1, F, 6, 0],
                       [4, 3, 5, 7, 9],
                       [1, 11, 2, 0, 0]], np.int32)
        bx = np.zeros((3, 5, 4), np.float32)
        bx[0, 1] = truth['grow'][0] + 1                                        # anchored on the first frame: forward only
        bx[0, 2] = truth['shrink'][F - 1] + 1                                  # on the last frame: backward only
        bx[0, 3] = (truth['const'][5] + 1) + np.float32([0.75, 0.5, 0.25, 0.99])     # fractional: truncated to the true box
        bx[0, 4] = [7, 7, 9, 9]                                                # (an empty slot's box is not looked at)
        bx[1, 0] = [118 + 6 + 1, 100 + 6 + 1, 118 + 6 + 37, 100 + 6 + 53]      # the white-noise object on frame 4 (index 3)
        bx[1, 1] = [60, 90, 64, 96]                                            # 5 x 7: levels collapse onto level 0
        bx[1, 2] = [100, 95, 101, 96]                                          # 2 x 2: levels collapse or are skipped
        bx[1, 3] = [-30.5, -25, 25, 40.25]                                     # over the left and the top edge, negative
        bx[1, 4] = [150, -15, 185.75, 30]                                      # the top
        bx[2, 0] = pc.leaver_box(W, S, R)                                      # the leaver, anchored on frame 1
        bx[2, 1] = [80, 170, 130, 230]                                         # the bottom
        bx[2, 2] = [W - 20, 80, W + 25.5, 140]                                 # the right
        sc = rng.rand(3, 5).astype(np.float32)
        _mixed[(S, R)] = (images, fr, bx, sc, truth)
    return _mixed[(S, R)]


# ---------------------------------------------------------------------------------------------------------------------
# the greedy loop's video: greedy_pixel_cases' layout with a growing object
# ---------------------------------------------------------------------------------------------------------------------
GB, GC = 12, 2
GIA, GIB, GIJA, GIJB, GIDIS = 0, 1, (2, 3), (4, 5), tuple(range(6, 12))
GJITTER = ((1, 1), (2, -1))
GAT = {'grow': (40, 60), 'const': (150, 120)}
GREEDY = dict(nms_thres=0.5, thres=0.3, max_tracks=3, grid=S, radius=R, min_conf=0.0)
_greedy = {}


def _iou(a, b):
    iw = min(a[2], b[2]) - max(a[0], b[0]) + 1
    ih = min(a[3], b[3]) - max(a[1], b[1]) + 1
    if iw <= 0 or ih <= 0:
        return 0.0
    inter = float(iw * ih)
    return inter / ((a[2] - a[0] + 1) * (a[3] - a[1] + 1) + (b[2] - b[0] + 1) * (b[3] - b[1] + 1) - inter)


def greedy_case():
    """Object A grows (the planted scene's 'grow' at GAT), object B keeps its size.  Proposals per frame, B = 12: 0 A's true
    box AT ITS TRUE SIZE, 1 B's true box, 2-3 / 4-5 their copies jittered by 1-2 px, 6-11 distractors (IoU < 0.2 with both).
    Scores, class 0: A's true box on frame 1 0.99, B's on frame 6 0.95, every other object proposal in (0.5, 0.9), the
    distractors in (0.31, 0.49); class 1: B's true box on frame 3 0.9, B's other proposals in (0.5, 0.8), the rest below thres.
    -> (images, boxes [F,12,4], scores [F,12,2], truth {kind: [F,4]}); computed once and shared (do not modify)"""
    if 'case' not in _greedy:
        rng = np.random.RandomState(5400)
        planes = np.repeat(background(5401)[None], F, axis=0)
        truth = {}
        for k, kind in enumerate(('grow', 'const')):
            waves = _waves(5410 + k, 5, 1.0, 4.0)
            truth[kind] = np.array([true_box(kind, f, *GAT[kind]) for f in range(F)], np.int64)
            for f in range(F):
                paint(planes[f], waves, truth[kind][f])
        boxes = np.zeros((F, GB, 4), np.float32)
        for f in range(F):
            ta, tb = truth['grow'][f] + 1, truth['const'][f] + 1
            boxes[f, GIA], boxes[f, GIB] = ta, tb
            for k, (jx, jy) in enumerate(GJITTER):
                boxes[f, GIJA[k]] = [ta[0] + jx, ta[1] + jy, ta[2] + jx, ta[3] + jy]
                boxes[f, GIJB[k]] = [tb[0] - jx, tb[1] + jy, tb[2] - jx, tb[3] + jy]
            for i in GIDIS:
                while True:
                    w, h = (int(v) for v in rng.randint(10, 31, size=2))
                    x, y = int(rng.randint(1, W - w + 1)), int(rng.randint(1, H - h + 1))
                    d = [x, y, x + w - 1, y + h - 1]
                    if _iou(d, ta) < 0.2 and _iou(d, tb) < 0.2:
                        break
                boxes[f, i] = d
        scores = np.zeros((F, GB, GC), np.float32)
        scores[:, :6, 0] = rng.uniform(0.5, 0.9, size=(F, 6))
        scores[:, 6:, 0] = rng.uniform(0.31, 0.49, size=(F, 6))
        scores[0, GIA, 0], scores[5, GIB, 0] = 0.99, 0.95
        scores[:, :, 1] = rng.uniform(0.05, 0.25, size=(F, GB))
        for i in (GIB,) + GIJB:
            scores[:, i, 1] = rng.uniform(0.5, 0.8, size=F)
        scores[2, GIB, 1] = 0.9
        _greedy['case'] = (grey(planes), boxes, scores, truth)
    return _greedy['case']


def greedy_specs():
    """the scaled and the fixed-scale spec's results on greedy_case(), computed once and shared (do not modify)"""
    if 'specs' not in _greedy:
        import pixtrack_spec as px
        images, boxes, scores, _ = greedy_case()
        _greedy['specs'] = (px.track_volume_pixels(images, boxes, scores, scales=1, scale_step=5, scale_penalty=0, **GREEDY),
                            px.track_volume_pixels(images, boxes, scores, **GREEDY))
    return _greedy['specs']
