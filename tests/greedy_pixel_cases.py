"""Seeded videos with proposals for the greedy pixel tracker's tests (CPU: the spec against the design; GPU: the device
against the spec).  pixtrack_cases.planted_video's style, with TWO textures: object A walks in the left half of the image,
object B in the right half, so their boxes never overlap.

Proposals per frame, B = 12:  0 A's true box, 1 B's true box, 2-3 A jittered by 1-2 px, 4-5 B jittered by 1-2 px (IoU with the
true box >= 0.3), 6-11 distractors (IoU < 0.3 with both objects on that frame)."""
import numpy as np

F, H, W, B, C = 10, 96, 128, 12, 2
S, R = 8, 3
WA, HA = 16, 24          # object A: whole multiples of the grid
WB, HB = 24, 16
FA, FB = 4, 6            # 0-based frames of the two designed anchors of class 0
JITTER = ((1, 1), (2, -1))
IA, IB, IJA, IJB, IDIS = 0, 1, (2, 3), (4, 5), tuple(range(6, 12))
THRES = 0.3


def iou(a, b):
    """f64 IoU of two 1-based inclusive boxes"""
    iw = min(a[2], b[2]) - max(a[0], b[0]) + 1
    ih = min(a[3], b[3]) - max(a[1], b[1]) + 1
    if iw <= 0 or ih <= 0:
        return 0.0
    inter = float(iw * ih)
    return inter / ((a[2] - a[0] + 1) * (a[3] - a[1] + 1) + (b[2] - b[0] + 1) * (b[3] - b[1] + 1) - inter)


def _walk(rng, n, x0, x1, y0, y1, w, h):
    """positions [n,2] of a w x h box inside columns x0..x1-1, rows y0..y1-1: moves of whole grid pitches, at most R - 1 cells"""
    px, py = w // S, h // S
    x, y = x0 + ((x1 - x0 - w) // (2 * px)) * px, y0 + ((y1 - y0 - h) // (2 * py)) * py
    pos = np.zeros((n, 2), np.int64)
    for f in range(n):
        if f:
            mx, my = (int(v) for v in rng.randint(-(R - 1), R, size=2))
            if not x0 <= x + mx * px <= x1 - w:
                mx = -mx
            if not x0 <= x + mx * px <= x1 - w:
                mx = 0
            if not y0 <= y + my * py <= y1 - h:
                my = -my
            if not y0 <= y + my * py <= y1 - h:
                my = 0
            x, y = x + mx * px, y + my * py
        pos[f] = (x, y)
    return pos


def box_of(pos, w, h):
    return [pos[0] + 1, pos[1] + 1, pos[0] + w, pos[1] + h]


def two_objects(seed, vanish_a_from=None):
    """-> images uint8 [F,H,W,3], boxes [F,B,4] f32, scores [F,B,C] f32, posA [F,2], posB [F,2] (0-based x1, y1).
    From frame ``vanish_a_from`` on object A is not pasted (its proposals stay).

    Scores, class 0: A's true box on frame FA 0.99, then A's first jittered copy on frame FA + 1 0.98 (second in the order: a
    duplicate), then B's true box on frame FB 0.95; every other object proposal in (0.5, 0.9), the distractors in (0.31, 0.49):
    above THRES, below every object proposal.  Class 1: B's true box on frame 2 0.9, B's other proposals in (0.5, 0.8),
    everything else below THRES."""
    rng = np.random.RandomState(seed)
    texa = rng.randint(0, 256, size=(HA, WA, 3)).astype(np.uint8)
    texb = rng.randint(0, 256, size=(HB, WB, 3)).astype(np.uint8)
    images = rng.randint(0, 256, size=(F, H, W, 3)).astype(np.uint8)
    posa = _walk(rng, F, 0, W // 2, 0, H, WA, HA)
    posb = _walk(rng, F, W // 2, W, 0, H, WB, HB)
    boxes = np.zeros((F, B, 4), np.float32)
    for f in range(F):
        if vanish_a_from is None or f < vanish_a_from:
            images[f, posa[f, 1]:posa[f, 1] + HA, posa[f, 0]:posa[f, 0] + WA] = texa
        images[f, posb[f, 1]:posb[f, 1] + HB, posb[f, 0]:posb[f, 0] + WB] = texb
        ta, tb = box_of(posa[f], WA, HA), box_of(posb[f], WB, HB)
        boxes[f, IA], boxes[f, IB] = ta, tb
        for k, (jx, jy) in enumerate(JITTER):
            boxes[f, IJA[k]] = [ta[0] + jx, ta[1] + jy, ta[2] + jx, ta[3] + jy]
            boxes[f, IJB[k]] = [tb[0] - jx, tb[1] + jy, tb[2] - jx, tb[3] + jy]
            assert iou(boxes[f, IJA[k]], ta) >= 0.3 and iou(boxes[f, IJB[k]], tb) >= 0.3
        for i in IDIS:
            while True:
                w, h = (int(v) for v in rng.randint(10, 31, size=2))
                x, y = int(rng.randint(1, W - w + 1)), int(rng.randint(1, H - h + 1))
                d = [x, y, x + w - 1, y + h - 1]
                if iou(d, ta) < 0.3 and iou(d, tb) < 0.3:
                    break
            boxes[f, i] = d
    scores = np.zeros((F, B, C), np.float32)
    scores[:, :6, 0] = rng.uniform(0.5, 0.9, size=(F, 6))
    scores[:, 6:, 0] = rng.uniform(0.31, 0.49, size=(F, 6))
    scores[FA, IA, 0], scores[FA + 1, IJA[0], 0], scores[FB, IB, 0] = 0.99, 0.98, 0.95
    scores[:, :, 1] = rng.uniform(0.05, 0.25, size=(F, B))
    for i in (IB,) + IJB:
        scores[:, i, 1] = rng.uniform(0.5, 0.8, size=F)
    scores[2, IB, 1] = 0.9
    return images, boxes, scores, posa, posb


MAIN = dict(nms_thres=0.3, thres=THRES, max_tracks=3, grid=S, radius=R, min_conf=0.0)
_cache = {}


def main_case():
    """the main case and the spec's result on it, computed once and shared (do not modify)"""
    if 'main' not in _cache:
        import pixtrack_spec as px
        case = two_objects(4100)
        _cache['main'] = (case, px.track_volume_pixels(case[0], case[1], case[2], **MAIN))
    return _cache['main']
