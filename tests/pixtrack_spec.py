"""The pixel tracker's rule in numpy: the specification of vdet_track_pixels (include/vdet_hip.h, csrc/pixtrack_kernels.hpp).
Integers only, except the confidence (one f32 division and one f32 subtraction).  The device must match it bit for bit.

Terms: ``//`` is python's floor division; image columns and rows are 0-based here; the API's boxes are 1-based inclusive.
An anchor box is truncated toward zero, then 1 is subtracted.

  luma      L = (29*c0 + 150*c1 + 77*c2 + 128) >> 8 on the stored channel order (BGR from cv2.imread, never swapped)
  grid      box (x1,y1,x2,y2), w = x2-x1+1, h = y2-y1+1, side S: cell k samples column clamp(x1 + ((2k+1)*w) // (2S), 0, W-1),
            rows likewise with h and H; k < 0 and k >= S are defined by the floor division and the clamp (edge replication)
  template  the grid k = 0..S-1 of the anchor box on the anchor frame; fixed for both directions, never updated
  step      f -> g = f +- step with box b: the region is the grid k = -R..S+R-1 of b on frame g; for every (dy,dx) in [-R,R]^2
            SAD = sum |Tm[i,j] - Rg[i+R+dy, j+R+dx]|; the smallest key (SAD, dy*dy+dx*dx, dy, dx) wins;
            conf = 1.0f - float(SAD) / float(255*S*S) in f32; conf < (float)min_conf ends the chain; else the box moves by
            sx = (2*dx*w + S) // (2S), sy = (2*dy*h + S) // (2S) (its size never changes); a moved box wholly outside the image
            ends the chain; else the row (x1+1, y1+1, x2+1, y2+1, conf) is written
  chain     also ends at the video's end and after ceil((max_frames+1)/2) - 1 steps when max_frames > 0.  Rows a slot does not
            write are NaN.  The anchor row is (truncated box, 1.0)
  bad data  an anchor frame outside 0..F, or -- on a live slot -- a box that is not finite, has |coordinate| > 2^20, w < 1 or
            h < 1 after truncation, or lies wholly outside the image: the slot is written as an empty one and the call is bad
"""
import math

import numpy as np

COORD_MAX = 1 << 20


def luma(img):
    """uint8 [...,3] -> uint8 [...]"""
    c = np.asarray(img).astype(np.int64)
    return ((29 * c[..., 0] + 150 * c[..., 1] + 77 * c[..., 2] + 128) >> 8).astype(np.uint8)


def grid_index(x1, w, S, k, W):
    """the column (row) of cell k; k an int or an int array"""
    return np.clip(x1 + ((2 * np.asarray(k, dtype=np.int64) + 1) * w) // (2 * S), 0, W - 1)


def sample(L, box, S, k0, k1):
    """the grid k0..k1-1 (both axes) of ``box`` (0-based ints) on the luma plane L [H,W] -> uint8 [k1-k0, k1-k0]"""
    x1, y1, x2, y2 = box
    H, W = L.shape
    k = np.arange(k0, k1)
    cols = grid_index(x1, x2 - x1 + 1, S, k, W)
    rows = grid_index(y1, y2 - y1 + 1, S, k, H)
    return L[rows[:, None], cols[None, :]]


def best_shift(Tm, Rg, R):
    """(SAD, dy, dx) of the smallest key (SAD, dy^2+dx^2, dy, dx)"""
    S = Tm.shape[0]
    n = 2 * R + 1
    win = np.lib.stride_tricks.sliding_window_view(Rg.astype(np.int32), (S, S))          # [n,n,S,S]: win[a,b] = Rg[a:a+S, b:b+S]
    assert win.shape[:2] == (n, n)
    sad = np.abs(win - Tm.astype(np.int32)[None, None]).sum(axis=(2, 3)).astype(np.int64)
    d = np.arange(-R, R + 1, dtype=np.int64)
    key = (sad << 32) | ((d[:, None] ** 2 + d[None, :] ** 2) << 16) | ((d[:, None] + R) << 8) | (d[None, :] + R)
    a, b = np.unravel_index(np.argmin(key), key.shape)
    assert (key == key[a, b]).sum() == 1
    return int(sad[a, b]), int(a) - R, int(b) - R


def confidence(sad, S):
    return np.float32(1.0) - np.float32(sad) / np.float32(255 * S * S)


def step_once(Tm, L, box, S, R):
    """one step onto the luma plane L: (moved box, conf, (dy, dx), SAD); the caller applies min_conf and the outside test"""
    x1, y1, x2, y2 = box
    w, h = x2 - x1 + 1, y2 - y1 + 1
    sad, dy, dx = best_shift(Tm, sample(L, box, S, -R, S + R), R)
    sx = (2 * dx * w + S) // (2 * S)
    sy = (2 * dy * h + S) // (2 * S)
    return (x1 + sx, y1 + sy, x2 + sx, y2 + sy), confidence(sad, S), (dy, dx), sad


def outside(box, H, W):
    x1, y1, x2, y2 = box
    return x2 < 0 or y2 < 0 or x1 > W - 1 or y1 > H - 1


def anchor_state(frame, box, F, H, W):
    """0: empty slot; -1: bad data; else 1 and the 0-based integer box"""
    frame = int(frame)
    if frame < 0 or frame > F:
        return -1, None
    if frame == 0:
        return 0, None
    b = np.asarray(box, dtype=np.float32)
    if not np.all(np.isfinite(b)) or np.any(np.abs(b) > np.float32(COORD_MAX)):
        return -1, None
    ib = tuple(int(v) - 1 for v in b)               # int(): toward zero
    if ib[2] - ib[0] + 1 < 1 or ib[3] - ib[1] + 1 < 1 or outside(ib, H, W):
        return -1, None
    return 1, ib


def reach_of(max_frames, F):
    return int(math.ceil((max_frames + 1) / 2.0)) - 1 if max_frames > 0 else F


def row_of(box, conf):
    return np.array([box[0] + 1, box[1] + 1, box[2] + 1, box[3] + 1, conf], dtype=np.float32)


def track_slot(lumas, frame, box, S, R, min_conf=0.5, max_frames=0, step=1):
    """rows [F,5] f32 of one live slot (``frame`` 1-based, ``box`` the 0-based integer anchor box)"""
    F, H, W = lumas.shape
    rows = np.full((F, 5), np.nan, np.float32)
    af = frame - 1
    rows[af] = row_of(box, np.float32(1.0))
    Tm = sample(lumas[af], box, S, 0, S)
    thr = np.float32(min_conf)
    for d in (1, -1):
        cur = box
        for n in range(1, reach_of(max_frames, F) + 1):
            g = af + d * n * step
            if g < 0 or g >= F:
                break
            cur, conf, _, _ = step_once(Tm, lumas[g], cur, S, R)
            if conf < thr or outside(cur, H, W):
                break
            rows[g] = row_of(cur, conf)
    return rows


def track_pixels(images, anchor_frames, anchor_boxes, anchor_scores=None, grid=32, radius=8, min_conf=0.5, max_frames=0, step=1):
    """images uint8 [F,H,W,3]; anchor_frames [C,T] int; anchor_boxes [C,T,4] f32 -> (tracks [C,T,F,5] f32, anchors [C,T,3] f32,
    ntracks [C] int32, bad: True where the device latches VDET_EINVAL)"""
    images = np.asarray(images)
    F, H, W = images.shape[:3]
    lumas = luma(images)
    C, T = anchor_frames.shape
    tracks = np.full((C, T, F, 5), np.nan, np.float32)
    anchors = np.zeros((C, T, 3), np.float32)
    ntracks = np.zeros(C, np.int32)
    bad = False
    for c in range(C):
        for t in range(T):
            anchors[c, t] = (np.float32(anchor_frames[c, t]), -1.0, 0.0 if anchor_scores is None else anchor_scores[c, t])
            st, ib = anchor_state(anchor_frames[c, t], anchor_boxes[c, t], F, H, W)
            if st < 0:
                bad = True
            if st == 1:
                tracks[c, t] = track_slot(lumas, int(anchor_frames[c, t]), ib, grid, radius, min_conf, max_frames, step)
                ntracks[c] = t + 1
    return tracks, anchors, ntracks, bad
