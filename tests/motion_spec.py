"""Motion-guided propagation of detections in numpy: the specification of vdet_motion_field, vdet_motion_table and
vdet_propagate_boxes (include/vdet_hip.h, csrc/motion_kernels.hpp; ops.motion_field, ops.propagate_detections).  Integers only,
except the output rows (one f32 add per coordinate, one f32 multiplication per step of the score).  The device must match it bit
for bit: equal NaN masks, and equal bit patterns elsewhere.

Terms: ``//`` is python's floor division; image columns and rows are 0-based here; the API's boxes are 1-based inclusive.

The motion field (``motion_field``): images uint8 [F,H,W,3], block P, radius R, Hb = ceil(H/P), Wb = ceil(W/P)

  luma      L = pixtrack_spec.luma, the tracker's, on the stored channel order
  pairs     direction 0 is f -> f+1 (f = 0..F-2), direction 1 is f -> f-1 (f = 1..F-1); the frame without a partner ([0,F-1] and
            [1,0]) is all zero in field, cost and fsum
  match     block (by,bx) of frame f against frame g: for every (dy,dx) in [-R,R]^2
            SAD = sum over i,j in 0..P-1 of |L_f[cy(by*P+i), cx(bx*P+j)] - L_g[cy(by*P+i+dy), cx(bx*P+j+dx)]|, cx / cy clamp to
            0..W-1 / 0..H-1 (edge replication; it also defines the partial blocks at the right and at the bottom);
            the smallest key (SAD, dy*dy+dx*dx, dy, dx) wins -- the tracker's tie order: zero motion on flat content
  outputs   field int16 [2,F,Hb,Wb,2] = (dx, dy), cost int32 [2,F,Hb,Wb] = the winner's SAD,
            fsum int32 [2,F,Hb+1,Wb+1,2]: fsum[d,f,y,x,:] = sum of field[d,f,r,c,:] over r < y, c < x (``summed``)

The motion of a box (``box_shift``): the mean of the field's vectors over the blocks whose CENTRE pixel P*b + P//2 lies in the box

  range     one axis, the box X1..X2 (0-based inclusive integers), h = P//2, N blocks: a0 = -((h - X1) // P), a1 = (X2 - h) // P;
            a1 < a0 (no centre inside; a degenerate box X2 < X1 too): a0 = a1 = ((X1 + X2) // 2) // P; both clamped to 0..N-1,
            then a1 = max(a1, a0)
  shift     n = blocks in the column range times blocks in the row range, s = the component summed over them (four entries of
            fsum): (2*s + n) // (2*n), the mean rounded half up

Propagation (``propagate``): the sources are the first min(top, keep_cnt[f,c]) entries of every keep list of the still-image
detections (boxes [F,B,4], scores [F,B,C], keep_idx [F,C,k], keep_cnt [F,C]: nms_tracks' ``still``)

  source    (f,c,j), b = keep_idx[f,c,j], ib = int(v) - 1 per coordinate of boxes[f,b] (toward zero, as the tracker's anchors)
  walk      per direction, m = 1..reach: the shift of step m is box_shift on the field of the frame the box is on, in that
            direction, at ib + (Sx,Sy), the shift accumulated so far; after the move, pixtrack_spec.outside(ib + (Sx,Sy)) ends the
            chain, as does the video's end
  rows      tubelet layout with T = 2*reach*top, slot t = di*top + j with di enumerating delta = -reach..-1, 1..reach:
            tracks[c,t,g] = (x1 + f32(Sx), y1 + f32(Sy), x2 + f32(Sx), y2 + f32(Sy), s_m) on g = f + delta -- one f32 add to the
            source's own f32 coordinate; s_0 = scores[f,b,c], s_m = f32(s_{m-1} * f32(decay)); score[c,t,g] = s_m; src[c,t,g] = b;
            ntracks[c] = T.  Rows no chain reaches are NaN with src = INT32_MIN
  bad data  a keep_cnt outside 0..k, a read keep_idx outside 0..B-1, a source box that is not finite or has |coordinate| > 2^20:
            the source writes NaN rows and the call is bad.  A degenerate box is not bad data
"""
import numpy as np

import pixtrack_spec as px

COORD_MAX = px.COORD_MAX
BLOCKS = (8, 16, 32)
INT32_MIN = -2 ** 31


def grid_of(H, W, P):
    return -(-H // P), -(-W // P)


def summed(field):
    """int [...,Hb,Wb,2] -> int32 [...,Hb+1,Wb+1,2]"""
    field = np.asarray(field)
    out = np.zeros(field.shape[:-3] + (field.shape[-3] + 1, field.shape[-2] + 1, 2), np.int32)
    out[..., 1:, 1:, :] = field.astype(np.int64).cumsum(axis=-3).cumsum(axis=-2)
    return out


def match_pair(Lf, Lg, P, R):
    """luma planes uint8 [H,W] of frame f and its partner g -> (field int16 [Hb,Wb,2], cost int32 [Hb,Wb])"""
    H, W = Lf.shape
    Hb, Wb = grid_of(H, W, P)
    ys, xs = np.arange(Hb * P), np.arange(Wb * P)
    Tm = Lf[np.clip(ys, 0, H - 1)[:, None], np.clip(xs, 0, W - 1)[None, :]].astype(np.int32)
    best = np.full((Hb, Wb), np.iinfo(np.int64).max, np.int64)
    for dy in range(-R, R + 1):
        rows = np.clip(ys + dy, 0, H - 1)[:, None]
        for dx in range(-R, R + 1):
            G = Lg[rows, np.clip(xs + dx, 0, W - 1)[None, :]].astype(np.int32)
            sad = np.abs(Tm - G).reshape(Hb, P, Wb, P).sum(axis=(1, 3)).astype(np.int64)
            key = (sad << 32) | ((dy * dy + dx * dx) << 16) | ((dy + R) << 8) | (dx + R)
            best = np.minimum(best, key)
    field = np.stack([(best & 0xFF) - R, ((best >> 8) & 0xFF) - R], axis=-1).astype(np.int16)
    return field, (best >> 32).astype(np.int32)


def motion_field(images, block=16, radius=8):
    """images uint8 [F,H,W,3] -> (field int16 [2,F,Hb,Wb,2], cost int32 [2,F,Hb,Wb], fsum int32 [2,F,Hb+1,Wb+1,2])"""
    images = np.asarray(images)
    assert block in BLOCKS and 1 <= radius <= 16
    F, H, W = images.shape[:3]
    L = px.luma(images)
    Hb, Wb = grid_of(H, W, block)
    field = np.zeros((2, F, Hb, Wb, 2), np.int16)
    cost = np.zeros((2, F, Hb, Wb), np.int32)
    for d, step in enumerate((1, -1)):
        for f in range(F):
            if 0 <= f + step < F:
                field[d, f], cost[d, f] = match_pair(L[f], L[f + step], block, radius)
    return field, cost, summed(field)


def block_range(X1, X2, P, N):
    """the blocks (of N on the axis) whose centre pixel lies in X1..X2: (first, last), never empty"""
    h = P // 2
    a0 = -((h - X1) // P)
    a1 = (X2 - h) // P
    if a1 < a0:
        a0 = a1 = ((X1 + X2) // 2) // P
    a0 = min(max(a0, 0), N - 1)
    a1 = min(max(a1, 0), N - 1)
    return a0, max(a1, a0)


def box_shift(fs, P, box):
    """fs: ONE (direction, frame) of fsum, int32 [Hb+1,Wb+1,2]; box 0-based inclusive integers -> (shift x, shift y)"""
    Hb, Wb = fs.shape[0] - 1, fs.shape[1] - 1
    x1, y1, x2, y2 = (int(v) for v in box)
    c0, c1 = block_range(x1, x2, P, Wb)
    r0, r1 = block_range(y1, y2, P, Hb)
    n = (c1 - c0 + 1) * (r1 - r0 + 1)
    J = fs.astype(np.int64)
    s = J[r1 + 1, c1 + 1] - J[r0, c1 + 1] - J[r1 + 1, c0] + J[r0, c0]
    return int((2 * s[0] + n) // (2 * n)), int((2 * s[1] + n) // (2 * n))


def source_state(box):
    """-1: bad data; else 1 and the 0-based integer box"""
    b = np.asarray(box, dtype=np.float32)
    if not np.all(np.isfinite(b)) or np.any(np.abs(b) > np.float32(COORD_MAX)):
        return -1, None
    return 1, tuple(int(v) - 1 for v in b)               # int(): toward zero


def deltas(reach):
    return list(range(-reach, 0)) + list(range(1, reach + 1))


def walk(fsum, P, H, W, f, ib, direction, reach):
    """the accumulated shifts [(Sx, Sy)] of the steps m = 1.. that a chain from frame f takes in ``direction`` (0: forward)"""
    F = fsum.shape[1]
    step = 1 if direction == 0 else -1
    Sx = Sy = 0
    out = []
    for m in range(1, reach + 1):
        g = f + step * m
        if g < 0 or g >= F:
            break
        cur = (ib[0] + Sx, ib[1] + Sy, ib[2] + Sx, ib[3] + Sy)
        sx, sy = box_shift(fsum[direction, g - step], P, cur)
        Sx, Sy = Sx + sx, Sy + sy
        if px.outside((ib[0] + Sx, ib[1] + Sy, ib[2] + Sx, ib[3] + Sy), H, W):
            break
        out.append((Sx, Sy))
    return out


def propagate(fsum, P, H, W, boxes, scores, keep_idx, keep_cnt, top, reach=3, decay=1.0):
    """-> (tracks [C,T,F,5] f32, ntracks [C] int32, score [C,T,F] f32, src [C,T,F] int32, bad: True where the device latches
    VDET_EINVAL), T = 2*reach*top"""
    fsum = np.asarray(fsum)
    boxes, scores = np.asarray(boxes, dtype=np.float32), np.asarray(scores, dtype=np.float32)
    F, B, C = scores.shape
    kcap = keep_idx.shape[2]
    assert fsum.shape[:2] == (2, F) and fsum.shape[2:4] == tuple(n + 1 for n in grid_of(H, W, P))
    assert 1 <= top <= kcap and 1 <= reach <= 16
    T = 2 * reach * top
    tracks = np.full((C, T, F, 5), np.nan, np.float32)
    score = np.full((C, T, F), np.nan, np.float32)
    src = np.full((C, T, F), INT32_MIN, np.int32)
    ntracks = np.full(C, T, np.int32)
    dec = np.float32(decay)
    slot = {delta: di for di, delta in enumerate(deltas(reach))}
    bad = False
    for f in range(F):
        for c in range(C):
            cnt = int(keep_cnt[f, c])
            if cnt < 0 or cnt > kcap:
                bad = True
                continue
            for j in range(min(top, cnt)):
                b = int(keep_idx[f, c, j])
                if b < 0 or b >= B:
                    bad = True
                    continue
                st, ib = source_state(boxes[f, b])
                if st < 0:
                    bad = True
                    continue
                for direction, step in enumerate((1, -1)):
                    s = scores[f, b, c]
                    for m, (Sx, Sy) in enumerate(walk(fsum, P, H, W, f, ib, direction, reach), 1):
                        s = np.float32(s * dec)
                        t, g = slot[step * m] * top + j, f + step * m
                        fx, fy = np.float32(Sx), np.float32(Sy)
                        tracks[c, t, g] = (boxes[f, b, 0] + fx, boxes[f, b, 1] + fy, boxes[f, b, 2] + fx, boxes[f, b, 3] + fy, s)
                        score[c, t, g] = s
                        src[c, t, g] = b
    return tracks, ntracks, score, src, bad
