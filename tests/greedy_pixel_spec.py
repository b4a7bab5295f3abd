"""Greedy tubelet generation with the pixel tracker in numpy: the specification of vdet_track_volume_pixels
(include/vdet_hip.h; ops.track_volume_pixels).  The device must match it bit for bit.

It is ``oracle.greedy_track_volume``'s loop (vdet/track.py:189-252 for one class on arrays), line for line, with
``pixtrack_spec.anchor_state`` + ``pixtrack_spec.track_slot`` in the place of ``iou_link_rows``:

  order     a stable descending sort of the float64 scores over the flat (frame, box) index
  cursor    monotone: a detection passed over is never an anchor again; the next anchor is the first kept one at or after it
  stop      no kept detection at or after the cursor, ``max_tracks`` tubelets, or an anchor scoring below ``thres``
  tracker   the anchor's box, truncated toward zero (vdet/track.py:224, map(int, bbox)), on its frame: pixtrack_spec's chain
  suppress  ``oracle.track_det_nms`` on every frame the new tubelet has a row on, against that row, over the kept
            detections of the frame; frames ``step`` skips have no row, so their detections stay
  bad data  an anchor whose box pixtrack_spec.anchor_state refuses takes its slot (anchors written, all rows NaN),
            suppresses nothing, and makes the call bad; the loop goes on
"""
import numpy as np

import pixtrack_spec as px
from oracle import oracle


def greedy_track_pixels_class(lumas, boxes, scores_c, nms_thres=0.3, thres=0.0, max_tracks=10, grid=32, radius=8, min_conf=0.5,
                              max_frames=0, step=1):
    """ONE class: lumas uint8 [F,H,W], boxes [F,B,4] f32, scores_c [F,B] f32 ->
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
            rows = px.track_slot(lumas, af0 + 1, ib, grid, radius, min_conf, max_frames, step)
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
                        max_frames=0, step=1):
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
            step)
        bad = bad or b
    return tracks, anchors, ntracks, bad
