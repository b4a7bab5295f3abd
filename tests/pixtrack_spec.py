"""The pixel tracker's rule in numpy: the specification of vdet_track_pixels, vdet_track_pixels_scaled, vdet_track_pixels_box,
vdet_track_volume_pixels, vdet_track_volume_pixels_scaled, vdet_track_volume_pixels_box and vdet_luma_integral
(include/vdet_hip.h, csrc/pixtrack_kernels.hpp; ops.track_pixels, track_pixels_scaled, track_volume_pixels,
track_volume_pixels_scaled and their ``sampling='box'``, ops.luma_integral).  Integers only, except the confidence (one f32
division and one f32 subtraction).  The device must match it bit for bit.

ONE walk serves every call: ``track_slot`` follows one anchor, ``track_pixels`` runs it over a slot table, and
``greedy_track_pixels_class`` / ``track_volume_pixels`` run it as the tracker of the greedy loop.  The scale search
(``scales``, ``scale_step``, ``scale_penalty``) and the sampling (``sampling='point'`` or ``'box'``) are parameters of that
walk; with none of them given it is the fixed-scale point rule.  The per-frame planes a walk reads -- the luma planes for
'point', their integral for 'box' -- are computed once per call by the top-level functions and passed down.

Terms: ``//`` is python's floor division; image columns and rows are 0-based here; the API's boxes are 1-based inclusive.
An anchor box is truncated toward zero, then 1 is subtracted; inside the rule boxes are 0-based inclusive integers.

The point rule (scales = 0, sampling = 'point')

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

The scale search (scales > 0).  Luma, the grid, the template, the confidence, the anchor checks, ``reach`` and the rows are the
point rule's.

  scales = ns (0..3) levels each side, scale_step = p (1..25) percent per level, scale_penalty = q (0..65535) SAD units per level

  levels    current box b = (x1,y1,x2,y2), w = x2-x1+1, h = y2-y1+1.  For l in -ns..ns: ex = sgn(l) * ((|l|*p*w + 100) // 200),
            ey likewise with h; b_l = (x1-ex, y1-ey, x2+ex, y2+ey), w_l = w + 2*ex, h_l = h + 2*ey (the centre is kept exactly).
            Level 0 is always admissible; l != 0 is skipped when w_l < 1, h_l < 1, w_l > 2^21 or h_l > 2^21.  Levels that give
            the same box are all searched; the key decides
  search    per admissible level the region is the grid k = -R..S+R-1 of b_l on frame g (S x S cells whatever the level), and
            every (dy,dx) in [-R,R]^2 gets the SAD against the anchor's S x S template, which is never rescaled or updated
  winner    the smallest key (SAD + |l|*q, |l|, dy*dy+dx*dx, dy, dx, l) over all admissible levels and shifts
  conf      1.0f - float(SAD) / float(255*S*S) from the winner's RAW SAD; conf < (float)min_conf ends the chain
  move      b_l moved by sx = (2*dx*w_l + S) // (2S), sy = (2*dy*h_l + S) // (2S); the box is now w_l x h_l; a moved box wholly
            outside the image ends the chain; else the row (x1+1, y1+1, x2+1, y2+1, conf) is written

With ns = 0 only level 0 is searched and this is the point rule's step exactly.  ``step_once`` finds the winner with
``sad_table`` + ``pick``; ``best_shift`` is a second, independent computation of the fixed-scale winner (one 4-D sliding
window, a 64-bit key, an assertion that the minimum is unique) that test_pixel_track_scaled_cpu.py holds against it on every
step of its walks.

Box sampling (sampling = 'box').  Only a cell's VALUE differs from the point rule.

  integral  I[f, y, x] = sum of L[f, r, c] over r < y, c < x: uint32 [F, H+1, W+1], row 0 and column 0 zero.  H*W <= 2^24, so
            the largest entry, 255 * 2^24, and every tot + (area >> 1) below fit in 32 bits
  edges     on one axis, from the box origin o, the extent e (w or h), the side S, the limit N (W or H), for ANY integer k:
            a = o + (k*e) // S, b = o + ((k+1)*e) // S; a' = clamp(a, 0, N-1), b' = min(max(b, a'+1), N).  A cell partly
            outside the image averages its inside part; a cell wholly outside, or narrower than a pixel (e < S), becomes the
            nearest single column or row (edge replication, as in the point rule)
  value     tot = I[rb', cb'] - I[ra', cb'] - I[rb', ca'] + I[ra', ca'], area = (rb'-ra') * (cb'-ca'),
            v = (tot + (area >> 1)) // area, a uint8: the rounded mean of the cell's pixels

Everything else is unchanged: the template is cells 0..S-1 of the anchor box on the anchor frame and the region cells
-R..S+R-1; SAD, key, tie order, f32 confidence, move, outside test, bad anchors, step and max_frames; levels, margins, penalty
and key of the scale search; the greedy loop.  With w == h == S every cell is one pixel and the rule is the point rule's, at
the image's edges too.

The greedy loop (``greedy_track_pixels_class``, ``track_volume_pixels``) is ``oracle.greedy_track_volume``'s loop
(vdet/track.py:189-252 for one class on arrays), line for line, with ``anchor_state`` + ``track_slot`` in the place of
``iou_link_rows``:

  order     a stable descending sort of the float64 scores over the flat (frame, box) index
  cursor    monotone: a detection passed over is never an anchor again; the next anchor is the first kept one at or after it
  stop      no kept detection at or after the cursor, ``max_tracks`` tubelets, or an anchor scoring below ``thres``
  tracker   the anchor's box, truncated toward zero (vdet/track.py:224, map(int, bbox)), on its frame: the chain above
  suppress  ``oracle.track_det_nms`` on every frame the new tubelet has a row on, against that row, over the kept
            detections of the frame; frames ``step`` skips have no row, so their detections stay
  bad data  an anchor whose box ``anchor_state`` refuses takes its slot (anchors written, all rows NaN), suppresses nothing,
            and makes the call bad; the loop goes on
"""
import math

import numpy as np

from oracle import oracle

COORD_MAX = 1 << 20
SIDE_MAX = 1 << 21
AREA_MAX = 1 << 24


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


def integral(lumas):
    """uint8 [F,H,W] -> uint32 [F,H+1,W+1]"""
    lumas = np.asarray(lumas)
    F, H, W = lumas.shape
    assert H * W <= AREA_MAX
    out = np.zeros((F, H + 1, W + 1), np.uint32)
    out[:, 1:, 1:] = lumas.astype(np.uint64).cumsum(axis=1).cumsum(axis=2).astype(np.uint32)
    return out


def luma_integral(images):
    """uint8 [F,H,W,3] -> uint32 [F,H+1,W+1]: what vdet_luma_integral writes"""
    return integral(luma(np.asarray(images)))


def cell_edges(o, e, S, k, N):
    """(a', b') of cell k on one axis; k an int or an int array"""
    k = np.asarray(k, dtype=np.int64)
    a = o + (k * e) // S
    b = o + ((k + 1) * e) // S
    a = np.clip(a, 0, N - 1)
    b = np.minimum(np.maximum(b, a + 1), N)
    return a, b


def sample_box(I, box, S, k0, k1):
    """the cells k0..k1-1 (both axes) of ``box`` (0-based ints) from ONE frame's integral I [H+1,W+1] -> uint8 [k1-k0, k1-k0]"""
    x1, y1, x2, y2 = box
    H, W = I.shape[0] - 1, I.shape[1] - 1
    k = np.arange(k0, k1)
    ca, cb = cell_edges(x1, x2 - x1 + 1, S, k, W)
    ra, rb = cell_edges(y1, y2 - y1 + 1, S, k, H)
    J = I.astype(np.int64)
    tot = J[rb[:, None], cb[None, :]] - J[ra[:, None], cb[None, :]] - J[rb[:, None], ca[None, :]] + J[ra[:, None], ca[None, :]]
    area = (rb - ra)[:, None] * (cb - ca)[None, :]
    assert area.min() >= 1 and tot.min() >= 0 and (tot <= 255 * area).all()
    return ((tot + (area >> 1)) // area).astype(np.uint8)


SAMPLERS = {'point': sample, 'box': sample_box}


def planes_of(images, sampling='point'):
    """what a walk reads, one plane per frame: the luma planes uint8 [F,H,W] for 'point', their integral uint32 [F,H+1,W+1]
    for 'box'"""
    assert sampling in SAMPLERS, sampling
    lumas = luma(np.asarray(images))
    return lumas if sampling == 'point' else integral(lumas)


def image_size(planes, sampling='point'):
    """(H, W) of the frames behind ``planes``"""
    pad = 0 if sampling == 'point' else 1
    return planes.shape[-2] - pad, planes.shape[-1] - pad


def check_settings(scales, scale_step, scale_penalty):
    assert 0 <= scales <= 3 and 1 <= scale_step <= 25 and 0 <= scale_penalty <= 65535


def level_box(box, l, p):
    """the box of level ``l`` at ``p`` percent per level, or None where the level is skipped"""
    if l == 0:
        return tuple(box)
    x1, y1, x2, y2 = box
    w, h = x2 - x1 + 1, y2 - y1 + 1
    sgn = 1 if l > 0 else -1
    ex = sgn * ((abs(l) * p * w + 100) // 200)
    ey = sgn * ((abs(l) * p * h + 100) // 200)
    wl, hl = w + 2 * ex, h + 2 * ey
    if wl < 1 or hl < 1 or wl > SIDE_MAX or hl > SIDE_MAX:
        return None
    return (x1 - ex, y1 - ey, x2 + ex, y2 + ey)


def best_shift(Tm, Rg, R):
    """(SAD, dy, dx) of the smallest key (SAD, dy^2+dx^2, dy, dx): the fixed-scale winner, computed independently of
    ``sad_table`` + ``pick`` (the walk uses those; the tests hold the two against each other)"""
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


def sad_table(Tm, Rg, R):
    """int64 [2R+1, 2R+1]: the SAD of every (dy, dx), indexed [dy+R, dx+R]"""
    S, n = Tm.shape[0], 2 * R + 1
    assert Tm.shape == (S, S) and Rg.shape == (S + 2 * R, S + 2 * R)
    T, G = Tm.astype(np.int16), Rg.astype(np.int16)
    out = np.empty((n, n), np.int64)
    for a in range(n):             # (a row of shifts at a time: the differences of one dy stay in the cache)
        win = np.lib.stride_tricks.sliding_window_view(G[a:a + S], S, axis=1)          # [S, n, S]: win[i, b] = G[a+i, b:b+S]
        out[a] = np.abs(win - T[:, None, :]).sum(axis=(0, 2), dtype=np.int64)
    return out


def pick(tables, R, q):
    """tables: {level: SAD table} of the admissible levels -> (raw SAD, level, dy, dx) of the smallest key
    (SAD + |l|*q, |l|, dy*dy+dx*dx, dy, dx, l)"""
    d = np.arange(-R, R + 1, dtype=np.int64)
    best = None
    for l, sad in tables.items():
        sad = np.asarray(sad, dtype=np.int64)
        assert sad.shape == (2 * R + 1, 2 * R + 1) and sad.min() >= 0
        # the tuple packed into one integer: every field is non-negative and below its field's width
        key = ((sad + abs(l) * q) << 40) | (abs(l) << 36) | ((d[:, None] ** 2 + d[None, :] ** 2) << 24) | ((d[:, None] + R) << 16) \
            | ((d[None, :] + R) << 8) | (l + 3)
        a, b = np.unravel_index(np.argmin(key), key.shape)
        if best is None or key[a, b] < best[0]:
            best = (int(key[a, b]), int(sad[a, b]), l, int(a) - R, int(b) - R)
    return best[1:]


def confidence(sad, S):
    return np.float32(1.0) - np.float32(sad) / np.float32(255 * S * S)


def step_once(Tm, plane, box, S, R, scales=0, scale_step=5, scale_penalty=0, sampling='point'):
    """one step onto the frame whose plane (luma for 'point', integral for 'box') is ``plane``: (moved box, conf,
    (level, dy, dx), raw SAD); the caller applies min_conf and the outside test"""
    cells = SAMPLERS[sampling]
    tables = {}
    for l in range(-scales, scales + 1):
        bl = level_box(box, l, scale_step)
        if bl is not None:
            tables[l] = sad_table(Tm, cells(plane, bl, S, -R, S + R), R)
    sad, l, dy, dx = pick(tables, R, scale_penalty)
    x1, y1, x2, y2 = level_box(box, l, scale_step)
    wl, hl = x2 - x1 + 1, y2 - y1 + 1
    sx = (2 * dx * wl + S) // (2 * S)
    sy = (2 * dy * hl + S) // (2 * S)
    return (x1 + sx, y1 + sy, x2 + sx, y2 + sy), confidence(sad, S), (l, dy, dx), sad


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


def track_slot(planes, frame, box, S, R, min_conf=0.5, max_frames=0, step=1, scales=0, scale_step=5, scale_penalty=0,
               sampling='point', trace=None):
    """rows [F,5] f32 of one live slot (``frame`` 1-based, ``box`` the 0-based integer anchor box) on ``planes_of(images,
    sampling)``.  ``trace``: a dict that receives {frame: (level, dy, dx)} of the steps taken"""
    check_settings(scales, scale_step, scale_penalty)
    F = planes.shape[0]
    H, W = image_size(planes, sampling)
    rows = np.full((F, 5), np.nan, np.float32)
    af = frame - 1
    rows[af] = row_of(box, np.float32(1.0))
    Tm = SAMPLERS[sampling](planes[af], box, S, 0, S)
    thr = np.float32(min_conf)
    for d in (1, -1):
        cur = tuple(box)
        for n in range(1, reach_of(max_frames, F) + 1):
            g = af + d * n * step
            if g < 0 or g >= F:
                break
            cur, conf, won, _ = step_once(Tm, planes[g], cur, S, R, scales, scale_step, scale_penalty, sampling)
            if conf < thr or outside(cur, H, W):
                break
            rows[g] = row_of(cur, conf)
            if trace is not None:
                trace[g] = won
    return rows


def track_pixels(images, anchor_frames, anchor_boxes, anchor_scores=None, grid=32, radius=8, min_conf=0.5, max_frames=0, step=1,
                 scales=0, scale_step=5, scale_penalty=0, sampling='point'):
    """images uint8 [F,H,W,3]; anchor_frames [C,T] int; anchor_boxes [C,T,4] f32 -> (tracks [C,T,F,5] f32, anchors [C,T,3] f32,
    ntracks [C] int32, bad: True where the device latches VDET_EINVAL)"""
    images = np.asarray(images)
    F, H, W = images.shape[:3]
    planes = planes_of(images, sampling)
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
                tracks[c, t] = track_slot(planes, int(anchor_frames[c, t]), ib, grid, radius, min_conf, max_frames, step, scales,
                                          scale_step, scale_penalty, sampling)
                ntracks[c] = t + 1
    return tracks, anchors, ntracks, bad


def greedy_track_pixels_class(planes, boxes, scores_c, nms_thres=0.3, thres=0.0, max_tracks=10, grid=32, radius=8, min_conf=0.5,
                              max_frames=0, step=1, scales=0, scale_step=5, scale_penalty=0, sampling='point'):
    """ONE class: planes = planes_of(images, sampling), boxes [F,B,4] f32, scores_c [F,B] f32 ->
    (tracks [max_tracks,F,5], anchors [max_tracks,3], ntracks, bad)"""
    F, B = scores_c.shape
    H, W = image_size(planes, sampling)
    frame = np.repeat(np.arange(1, F + 1), B).astype(np.float64)
    det = np.hstack([frame[:, None], boxes.reshape(-1, 4).astype(np.float64),
                     scores_c.reshape(-1, 1).astype(np.float64)])
    order = np.argsort(-det[:, 5], kind='stable')
    det_info = det[order].astype(np.float32)
    ids_by_frame = {}
    for i, fr in enumerate(det_info[:, 0]):
        ids_by_frame.setdefault(int(fr), []).append(i)
    keep = np.ones(len(det_info), dtype=bool)
    cur = 0
    tracks = np.full((max_tracks, F, 5), np.nan, dtype=np.float32)
    anchors = np.zeros((max_tracks, 3), dtype=np.float32)
    nt = 0
    bad = False
    while keep.any() and nt < max_tracks:
        while cur < len(keep) and not keep[cur]:
            cur += 1
        if cur == len(keep):
            break
        top = det_info[cur]
        top_flat = order[cur]
        cur += 1
        if top[-1] < thres:
            break
        af0 = int(top[0]) - 1
        ab = int(top_flat - af0 * B)
        state, ib = anchor_state(af0 + 1, boxes[af0, ab], F, H, W)
        if state == 1:
            rows = track_slot(planes, af0 + 1, ib, grid, radius, min_conf, max_frames, step, scales, scale_step, scale_penalty,
                              sampling)
        else:
            bad = True
            rows = np.full((F, 5), np.nan, dtype=np.float32)
        tracks[nt] = rows
        anchors[nt] = [af0 + 1, ab, top[-1]]
        nt += 1
        for f in range(F):
            if np.isnan(rows[f, 0]):
                continue
            det_ids = [i for i in ids_by_frame.get(f + 1, []) if keep[i]]
            if not det_ids:
                continue
            t = np.asarray([[f + 1, rows[f, 0], rows[f, 1], rows[f, 2], rows[f, 3]]], dtype=np.float32)
            kp = set(oracle.track_det_nms(t, det_info[det_ids], nms_thres))
            for i, det_id in enumerate(det_ids):
                if i not in kp:
                    keep[det_id] = False
    return tracks, anchors, nt, bad


def track_volume_pixels(images, boxes, scores, nms_thres=0.3, thres=0.0, max_tracks=10, grid=32, radius=8, min_conf=0.5,
                        max_frames=0, step=1, scales=0, scale_step=5, scale_penalty=0, sampling='point'):
    """images uint8 [F,H,W,3], boxes [F,B,4] f32, scores [F,B,C] f32 -> (tracks [C,max_tracks,F,5] f32, anchors
    [C,max_tracks,3] f32, ntracks [C] int32, bad: True where the device latches VDET_EINVAL)"""
    planes = planes_of(images, sampling)
    boxes = np.asarray(boxes, dtype=np.float32)
    scores = np.asarray(scores, dtype=np.float32)
    F, B, C = scores.shape
    tracks = np.full((C, max_tracks, F, 5), np.nan, np.float32)
    anchors = np.zeros((C, max_tracks, 3), np.float32)
    ntracks = np.zeros(C, np.int32)
    bad = False
    for c in range(C):
        tracks[c], anchors[c], ntracks[c], b = greedy_track_pixels_class(
            planes, boxes, np.ascontiguousarray(scores[:, :, c]), nms_thres, thres, max_tracks, grid, radius, min_conf, max_frames,
            step, scales, scale_step, scale_penalty, sampling)
        bad = bad or b
    return tracks, anchors, ntracks, bad
