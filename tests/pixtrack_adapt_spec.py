"""The pixel tracker's template update with an anchor guard, in numpy: the specification of vdet_track_pixels_adaptive and
vdet_track_volume_pixels_adaptive (include/vdet_hip.h, csrc/pixtrack_kernels.hpp; the ``update`` / ``update_conf`` /
``drift_conf`` keywords of ops.track_pixels, track_pixels_scaled, track_volume_pixels, track_volume_pixels_scaled).  Integers
except the confidences.  The device must match it bit for bit.

Everything not restated here is tests/pixtrack_spec.py's: luma, grid, box cells, levels, key, tie order, confidence, move,
outside test, bad anchors, ``step``, ``max_frames``, the greedy loop.  This module is built from that one's ``SAMPLERS``,
``level_box``, ``sad_table``, ``pick``, ``confidence``, ``outside``, ``anchor_state``, ``reach_of`` and ``row_of``.

  settings  update = a, an integer in 0 .. 256: the weight of the new patch in 1/256;  update_conf, drift_conf: finite
  state     per chain -- per slot AND direction -- A[S,S], 8.8 fixed-point integers in 0 .. 65280, initialised to Tm0 << 8.
            Tm0 is the anchor's template: cells 0..S-1 of the truncated anchor box on the anchor frame, point or box sampled.
            The backward chain starts from Tm0 again, never from what the forward chain made of it
  match     a step matches against Tm = (A + 128) >> 8 (uint8) in the place of the fixed template; nothing else changes
  patch     after a step the chain keeps (conf >= min_conf and the moved box not wholly outside), with winner (l, dy, dx):
            P[S,S] = cells dx .. dx+S-1 (columns) by dy .. dy+S-1 (rows) of the winner's level box b_l on frame g, before the
            move: the window that won, Rg_l[R+dy : R+dy+S, R+dx : R+dx+S]
  guard     SAD0 = sum |Tm0 - P|;  c0 = 1.0f - float(SAD0) / float(255*S*S), in f32 like conf
  accept    a > 0 and conf >= (float)update_conf and c0 >= (float)drift_conf: f32 compares
  update    on accept, element by element: A = ((256 - a) * A + a * (P << 8) + 128) >> 8.  The largest intermediate is
            256 * 65280 + 128; A stays within 0 .. 65280; a = 256 makes A = P << 8, the replace-every-frame tracker.  The 8.8
            state is the point: a uint8 state stalls as soon as a * |P - Tm| < 128

The rows, the confidence in column 4 (the step's conf, against the CURRENT template), the NaN pattern, anchors and ntracks are
pixtrack_spec's.  With a = 0, or an update_conf or drift_conf no step can reach (2.0), the bits are the fixed-template rule's.

``track_slot`` restates pixtrack_spec.track_slot's walk and ``step_regions`` its ``step_once`` (they keep the regions, which
that one drops), ``greedy_track_pixels_class`` its greedy loop with this walk as the tracker; test_pixel_track_adapt_cpu.py
pins each restatement against the original on bits at update = 0.
"""
import numpy as np

from oracle import oracle

import pixtrack_spec as px


def check_update(update, update_conf, drift_conf):
    assert int(update) == update and 0 <= update <= 256 and np.isfinite(update_conf) and np.isfinite(drift_conf)


def template_of(A):
    """the uint8 template a step matches against"""
    return ((np.asarray(A, dtype=np.int64) + 128) >> 8).astype(np.uint8)


def initial_state(Tm0):
    return np.asarray(Tm0).astype(np.int64) << 8


def updated(A, P, a):
    """the state after an accepted step"""
    A = np.asarray(A, dtype=np.int64)
    out = ((256 - a) * A + a * (np.asarray(P).astype(np.int64) << 8) + 128) >> 8
    assert out.min() >= 0 and out.max() <= 65280
    return out


def step_regions(Tm, plane, box, S, R, scales, scale_step, scale_penalty, sampling):
    """pixtrack_spec.step_once that also returns the winning window: (moved box, conf, (level, dy, dx), P)"""
    cells = px.SAMPLERS[sampling]
    tables, regions = {}, {}
    for l in range(-scales, scales + 1):
        bl = px.level_box(box, l, scale_step)
        if bl is not None:
            regions[l] = cells(plane, bl, S, -R, S + R)
            tables[l] = px.sad_table(Tm, regions[l], R)
    sad, l, dy, dx = px.pick(tables, R, scale_penalty)
    x1, y1, x2, y2 = px.level_box(box, l, scale_step)
    wl, hl = x2 - x1 + 1, y2 - y1 + 1
    sx = (2 * dx * wl + S) // (2 * S)
    sy = (2 * dy * hl + S) // (2 * S)
    P = regions[l][R + dy:R + dy + S, R + dx:R + dx + S]
    return (x1 + sx, y1 + sy, x2 + sx, y2 + sy), px.confidence(sad, S), (l, dy, dx), P


def track_slot(planes, frame, box, S, R, min_conf=0.5, max_frames=0, step=1, scales=0, scale_step=5, scale_penalty=0,
               sampling='point', update=0, update_conf=0.8, drift_conf=0.7, trace=None):
    """rows [F,5] f32 of one live slot (``frame`` 1-based, ``box`` the 0-based integer anchor box) on ``px.planes_of(images,
    sampling)``.  ``trace``: a dict that receives {frame: (level, dy, dx, conf, c0, accepted)} of the steps the chains keep"""
    px.check_settings(scales, scale_step, scale_penalty)
    check_update(update, update_conf, drift_conf)
    F = planes.shape[0]
    H, W = px.image_size(planes, sampling)
    rows = np.full((F, 5), np.nan, np.float32)
    af = frame - 1
    rows[af] = px.row_of(box, np.float32(1.0))
    Tm0 = px.SAMPLERS[sampling](planes[af], box, S, 0, S)
    thr, uthr, dthr = np.float32(min_conf), np.float32(update_conf), np.float32(drift_conf)
    for d in (1, -1):
        cur = tuple(box)
        A = initial_state(Tm0)
        for n in range(1, px.reach_of(max_frames, F) + 1):
            g = af + d * n * step
            if g < 0 or g >= F:
                break
            cur, conf, won, P = step_regions(template_of(A), planes[g], cur, S, R, scales, scale_step, scale_penalty, sampling)
            if conf < thr or px.outside(cur, H, W):
                break
            rows[g] = px.row_of(cur, conf)
            sad0 = int(np.abs(Tm0.astype(np.int64) - P.astype(np.int64)).sum())
            c0 = px.confidence(sad0, S)
            accepted = bool(update > 0 and conf >= uthr and c0 >= dthr)
            if accepted:
                A = updated(A, P, update)
            if trace is not None:
                trace[g] = won + (conf, c0, accepted)
    return rows


def track_pixels(images, anchor_frames, anchor_boxes, anchor_scores=None, grid=32, radius=8, min_conf=0.5, max_frames=0, step=1,
                 scales=0, scale_step=5, scale_penalty=0, sampling='point', update=0, update_conf=0.8, drift_conf=0.7, traces=None):
    """pixtrack_spec.track_pixels with the three new keywords.  ``traces``: a dict that receives {(c, t): trace} of the live slots"""
    images = np.asarray(images)
    F, H, W = images.shape[:3]
    planes = px.planes_of(images, sampling)
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
                tr = None if traces is None else traces.setdefault((c, t), {})
                tracks[c, t] = track_slot(planes, int(anchor_frames[c, t]), ib, grid, radius, min_conf, max_frames, step, scales,
                                          scale_step, scale_penalty, sampling, update, update_conf, drift_conf, tr)
                ntracks[c] = t + 1
    return tracks, anchors, ntracks, bad


def greedy_track_pixels_class(planes, boxes, scores_c, nms_thres=0.3, thres=0.0, max_tracks=10, grid=32, radius=8, min_conf=0.5,
                              max_frames=0, step=1, scales=0, scale_step=5, scale_penalty=0, sampling='point', update=0,
                              update_conf=0.8, drift_conf=0.7):
    """pixtrack_spec.greedy_track_pixels_class, line for line, with this module's ``track_slot`` as the tracker"""
    F, B = scores_c.shape
    H, W = px.image_size(planes, sampling)
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
            rows = track_slot(planes, af0 + 1, ib, grid, radius, min_conf, max_frames, step, scales, scale_step, scale_penalty,
                              sampling, update, update_conf, drift_conf)
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
                        max_frames=0, step=1, scales=0, scale_step=5, scale_penalty=0, sampling='point', update=0, update_conf=0.8,
                        drift_conf=0.7):
    """pixtrack_spec.track_volume_pixels with the three new keywords"""
    planes = px.planes_of(images, sampling)
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
            step, scales, scale_step, scale_penalty, sampling, update, update_conf, drift_conf)
        bad = bad or b
    return tracks, anchors, ntracks, bad
