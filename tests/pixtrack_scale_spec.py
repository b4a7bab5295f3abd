"""The pixel tracker with a scale search in numpy: the specification of vdet_track_pixels_scaled and
vdet_track_volume_pixels_scaled (include/vdet_hip.h, csrc/pixtrack_kernels.hpp).  Integers only, except the confidence.  The
device must match it bit for bit.  Luma, the grid, the template, the confidence, the anchor checks, ``reach`` and the rows are
tests/pixtrack_spec.py's; boxes are 0-based inclusive inside the rule, ``//`` is floor division.

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

With ns = 0 this is pixtrack_spec's rule exactly.  The greedy form is greedy_pixel_spec's loop, line for line, with this
module's ``track_slot`` as the tracker.
"""
import numpy as np

import pixtrack_spec as px
from oracle import oracle

SIDE_MAX = 1 << 21


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


def step_once(Tm, L, box, S, R, ns, p, q):
    """one step onto the luma plane L: (moved box, conf, (level, dy, dx), raw SAD)"""
    tables = {}
    for l in range(-ns, ns + 1):
        bl = level_box(box, l, p)
        if bl is not None:
            tables[l] = sad_table(Tm, px.sample(L, bl, S, -R, S + R), R)
    sad, l, dy, dx = pick(tables, R, q)
    x1, y1, x2, y2 = level_box(box, l, p)
    wl, hl = x2 - x1 + 1, y2 - y1 + 1
    sx = (2 * dx * wl + S) // (2 * S)
    sy = (2 * dy * hl + S) // (2 * S)
    return (x1 + sx, y1 + sy, x2 + sx, y2 + sy), px.confidence(sad, S), (l, dy, dx), sad


def track_slot(lumas, frame, box, S, R, min_conf=0.5, max_frames=0, step=1, scales=1, scale_step=5, scale_penalty=0, trace=None):
    """rows [F,5] f32 of one live slot (``frame`` 1-based, ``box`` the 0-based integer anchor box).  ``trace``: a dict that
    receives {frame: (level, dy, dx)} of the steps taken"""
    check_settings(scales, scale_step, scale_penalty)
    F, H, W = lumas.shape
    rows = np.full((F, 5), np.nan, np.float32)
    af = frame - 1
    rows[af] = px.row_of(box, np.float32(1.0))
    Tm = px.sample(lumas[af], box, S, 0, S)
    thr = np.float32(min_conf)
    for d in (1, -1):
        cur = tuple(box)
        for n in range(1, px.reach_of(max_frames, F) + 1):
            g = af + d * n * step
            if g < 0 or g >= F:
                break
            cur, conf, won, _ = step_once(Tm, lumas[g], cur, S, R, scales, scale_step, scale_penalty)
            if conf < thr or px.outside(cur, H, W):
                break
            rows[g] = px.row_of(cur, conf)
            if trace is not None:
                trace[g] = won
    return rows


def track_pixels(images, anchor_frames, anchor_boxes, anchor_scores=None, grid=32, radius=8, min_conf=0.5, max_frames=0, step=1,
                 scales=1, scale_step=5, scale_penalty=0):
    """pixtrack_spec.track_pixels with the scaled chain: -> (tracks [C,T,F,5] f32, anchors [C,T,3] f32, ntracks [C] int32, bad)"""
    images = np.asarray(images)
    F, H, W = images.shape[:3]
    lumas = px.luma(images)
    C, T = anchor_frames.shape
    tracks = np.full((C, T, F, 5), np.nan, np.float32)
    anchors = np.zeros((C, T, 3), np.float32)
    ntracks = np.zeros(C, np.int32)
    bad = False
    for c in range(C):
        for t in range(T):
            anchors[c, t] = (np.float32(anchor_frames[c, t]), -1.0, 0.0 if anchor_scores is None else anchor_scores[c, t])
            st, ib = px.anchor_state(anchor_frames[c, t], anchor_boxes[c, t], F, H, W)
            if st < 0:
                bad = True
            if st == 1:
                tracks[c, t] = track_slot(lumas, int(anchor_frames[c, t]), ib, grid, radius, min_conf, max_frames, step, scales,
                                          scale_step, scale_penalty)
                ntracks[c] = t + 1
    return tracks, anchors, ntracks, bad


def greedy_track_pixels_class(lumas, boxes, scores_c, nms_thres=0.3, thres=0.0, max_tracks=10, grid=32, radius=8, min_conf=0.5,
                              max_frames=0, step=1, scales=1, scale_step=5, scale_penalty=0):
    """ONE class: greedy_pixel_spec.greedy_track_pixels_class with the scaled ``track_slot`` ->
    (tracks [max_tracks,F,5], anchors [max_tracks,3], ntracks, bad)"""
    F, B = scores_c.shape
    H, W = lumas.shape[1:]
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
        state, ib = px.anchor_state(af0 + 1, boxes[af0, ab], F, H, W)
        if state == 1:
            rows = track_slot(lumas, af0 + 1, ib, grid, radius, min_conf, max_frames, step, scales, scale_step, scale_penalty)
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
                        max_frames=0, step=1, scales=1, scale_step=5, scale_penalty=0):
    """images uint8 [F,H,W,3], boxes [F,B,4] f32, scores [F,B,C] f32 -> (tracks [C,max_tracks,F,5] f32, anchors
    [C,max_tracks,3] f32, ntracks [C] int32, bad: True where the device latches VDET_EINVAL)"""
    lumas = px.luma(np.asarray(images))
    boxes = np.asarray(boxes, dtype=np.float32)
    scores = np.asarray(scores, dtype=np.float32)
    F, B, C = scores.shape
    tracks = np.full((C, max_tracks, F, 5), np.nan, np.float32)
    anchors = np.zeros((C, max_tracks, 3), np.float32)
    ntracks = np.zeros(C, np.int32)
    bad = False
    for c in range(C):
        tracks[c], anchors[c], ntracks[c], b = greedy_track_pixels_class(
            lumas, boxes, np.ascontiguousarray(scores[:, :, c]), nms_thres, thres, max_tracks, grid, radius, min_conf, max_frames,
            step, scales, scale_step, scale_penalty)
        bad = bad or b
    return tracks, anchors, ntracks, bad
