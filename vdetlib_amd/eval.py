"""VOC-style average precision for video object detection (the reference has no
evaluator; BASELINE config 5 asks for mAP on VID-shaped data).  The host evaluator: it is the
specification of the device evaluator ``ops.DetEvaluator`` (eval_kernels.hpp), which returns the same
per-class AP and mAP from the device outputs without bringing detections to the host.

Detections are scored boxes per (video, frame, class); ground truth comes from .annot protocol
dicts (tools/imagenet_annotation_processor).  A detection is a true positive when it overlaps a
not-yet-matched ground-truth box of its video/frame/class with IoU >= iou_thr (+1 pixel
convention, the reference's utils/common.py:451-468); AP is the area under the monotone
precision envelope (VOC2010+ / ILSVRC all-point interpolation).  ``rule='ilsvrc'`` swaps the fixed
threshold for the ILSVRC VID devkit's per-box one (small objects, see ``evaluate``)."""
from collections import defaultdict

import numpy as np


def _iou_1n(box, boxes):
    ix1 = np.maximum(box[0], boxes[:, 0]); iy1 = np.maximum(box[1], boxes[:, 1])
    ix2 = np.minimum(box[2], boxes[:, 2]); iy2 = np.minimum(box[3], boxes[:, 3])
    iw = np.maximum(0.0, ix2 - ix1 + 1); ih = np.maximum(0.0, iy2 - iy1 + 1)
    inter = iw * ih
    a = (box[2] - box[0] + 1) * (box[3] - box[1] + 1)
    b = (boxes[:, 2] - boxes[:, 0] + 1) * (boxes[:, 3] - boxes[:, 1] + 1)
    return inter / (a + b - inter)


def ground_truth_from_annots(annot_protos):
    """{(video, frame, class_index): float64 [n,4]}"""
    gt = defaultdict(list)
    for annot in annot_protos:
        for track in annot['annotations']:
            for box in track['track']:
                gt[(annot['video'], box['frame'], box['class_index'])].append(box['bbox'])
    return {k: np.asarray(v, dtype=np.float64).reshape(-1, 4) for k, v in gt.items()}


def detections_from_score_protos(score_protos, key='det_score'):
    """Tubelet boxes of .score protocol dicts -> list of (video, frame, class_index, bbox, score)."""
    dets = []
    for sp in score_protos:
        for tubelet in sp['tubelets']:
            for box in tubelet['boxes']:
                dets.append((sp['video'], box['frame'], tubelet['class_index'], box['bbox'], float(box[key])))
    return dets


def detections_from_tracks(video, tracks, ntracks, scores, boxes=None):
    """Device tubelets (ops.track_volume / ops.rescore_tracks arrays, already on the host) -> the same
    list.  tracks [C,T,F,5]; scores [C,T,F] (NaN = no box); boxes [C,T,F,4] (default: the track boxes).
    class_index = c + 1 (column c of the score volume is class c + 1, vdet/tubelet_cls.py:514)."""
    dets = []
    C, T, F = scores.shape
    bx = tracks[..., :4] if boxes is None else boxes
    for c in range(C):
        for t in range(int(ntracks[c])):
            for f in range(F):
                if not np.isnan(scores[c, t, f]):
                    dets.append((video, f + 1, c + 1, [float(v) for v in bx[c, t, f]], float(scores[c, t, f])))
    return dets


def detections_from_keep_lists(video, boxes, scores, keep_idx, keep_cnt, layout='FBC', class_base=1):
    """NMS survivors (ops.nms_volume[_topk] / nms_track_volume / video_batch arrays, already on the host) -> the
    (video, frame, class_index, bbox, score) list, nesting frame, class, k < keep_cnt: frame = f + 1, class = c +
    class_base.  boxes [F,B,4] f32, scores [F,B,C] ('FBC') or [F,C,B] ('FCB') f32, keep_idx [F,C,cap], keep_cnt [F,C]."""
    if layout not in ('FBC', 'FCB'):
        raise ValueError("layout must be 'FBC' or 'FCB'")
    dets = []
    F, C = keep_cnt.shape
    for f in range(F):
        for c in range(C):
            for k in range(int(keep_cnt[f, c])):
                b = int(keep_idx[f, c, k])
                s = scores[f, b, c] if layout == 'FBC' else scores[f, c, b]
                dets.append((video, f + 1, c + class_base, [float(v) for v in boxes[f, b]], float(s)))
    return dets


def gt_table_from_annots(annot_protos):
    """What ground_truth_from_annots reads, as flat arrays that can be uploaded:
    {'videos': [name, ...] (first-seen order), 'video': int32 [G] (index into videos), 'frame': int64 [G],
     'class_index': int64 [G], 'bbox': float64 [G,4]} -- boxes in annotation order (within every
    (video, frame, class) the order of ground_truth_from_annots, which decides ties of equal IoU)."""
    videos, vidx, vid, frame, cls, bbox = [], {}, [], [], [], []
    for annot in annot_protos:
        v = vidx.setdefault(annot['video'], len(videos))
        if v == len(videos):
            videos.append(annot['video'])
        for track in annot['annotations']:
            for box in track['track']:
                vid.append(v); frame.append(box['frame']); cls.append(box['class_index']); bbox.append(box['bbox'])
    return {'videos': videos, 'video': np.asarray(vid, dtype=np.int32), 'frame': np.asarray(frame, dtype=np.int64),
            'class_index': np.asarray(cls, dtype=np.int64), 'bbox': np.asarray(bbox, dtype=np.float64).reshape(-1, 4)}


def gt_from_table(table):
    """gt_table_from_annots -> the dict of ground_truth_from_annots."""
    gt = defaultdict(list)
    for i in range(len(table['video'])):
        gt[(table['videos'][int(table['video'][i])], int(table['frame'][i]), int(table['class_index'][i]))].append(table['bbox'][i])
    return {k: np.asarray(v, dtype=np.float64).reshape(-1, 4) for k, v in gt.items()}


def _ilsvrc_pick(box, g, used, iou_thr):
    """The ILSVRC VID rule for one detection: the unmatched ground truth with iw > 0, ih > 0 and IoU >= its own
    threshold min(iou_thr, w*h / ((w+10)*(h+10))) that has the largest IoU (the first of equal ones); -1 if none.
    IoU in _iou_1n's operation order (f64)."""
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        ix1 = np.maximum(box[0], g[:, 0]); iy1 = np.maximum(box[1], g[:, 1])
        ix2 = np.minimum(box[2], g[:, 2]); iy2 = np.minimum(box[3], g[:, 3])
        iw = np.maximum(0.0, ix2 - ix1 + 1); ih = np.maximum(0.0, iy2 - iy1 + 1)
        inter = iw * ih
        a = (box[2] - box[0] + 1) * (box[3] - box[1] + 1)
        b = (g[:, 2] - g[:, 0] + 1) * (g[:, 3] - g[:, 1] + 1)
        ov = inter / (a + b - inter)
        w = g[:, 2] - g[:, 0] + 1; h = g[:, 3] - g[:, 1] + 1
        thr = np.minimum(iou_thr, (w * h) / ((w + 10) * (h + 10)))
        ok = (~used) & (iw > 0) & (ih > 0) & (ov >= thr) & (ov > -np.inf)
    if not ok.any():
        return -1
    return int(np.argmax(np.where(ok, ov, -np.inf)))


def average_precision(tp, n_gt):
    """tp: bool array in descending-score order."""
    if n_gt == 0:
        return float('nan')
    tp = np.asarray(tp, dtype=bool)
    ctp = np.cumsum(tp); cfp = np.cumsum(~tp)
    rec = ctp / float(n_gt)
    prec = ctp / np.maximum(ctp + cfp, 1)
    mrec = np.concatenate([[0.0], rec, [1.0]])
    mpre = np.concatenate([[0.0], prec, [0.0]])
    for i in range(len(mpre) - 2, -1, -1):
        mpre[i] = max(mpre[i], mpre[i + 1])
    idx = np.where(mrec[1:] != mrec[:-1])[0]
    return float(np.sum((mrec[idx + 1] - mrec[idx]) * mpre[idx + 1]))


def evaluate(dets, gt, iou_thr=0.5, classes=None, rule='voc'):
    """dets: list of (video, frame, class_index, bbox, score); gt from ground_truth_from_annots.
    Returns ({class_index: AP}, mAP over the classes that have ground truth).

    rule='voc': IoU >= iou_thr against the arg-max IoU ground truth (already matched ones count -1).
    rule='ilsvrc': the ILSVRC VID devkit's matching loop as restated from its published description: every ground
    truth has its own threshold min(iou_thr, w*h / ((w+10)*(h+10))) (w, h: +1 convention), and the detection takes
    the unmatched ground truth with iw > 0, ih > 0, IoU >= that threshold and the largest IoU (the first of equal
    ones).  NOT pinned against the devkit (it is not part of this project); the devkit's blacklist and
    motion-speed splits are not implemented."""
    if rule not in ('voc', 'ilsvrc'):
        raise ValueError("rule must be 'voc' or 'ilsvrc'")
    by_class = defaultdict(list)
    for d in dets:
        by_class[d[2]].append(d)
    gt_classes = sorted(set(k[2] for k in gt)) if classes is None else list(classes)
    aps = {}
    for c in gt_classes:
        n_gt = sum(len(v) for k, v in gt.items() if k[2] == c)
        _, tp = match_class(by_class.get(c, []), gt, c, iou_thr, rule)
        aps[c] = average_precision(tp, n_gt)
    valid = [v for v in aps.values() if not np.isnan(v)]
    return aps, (float(np.mean(valid)) if valid else float('nan'))


def match_class(class_dets, gt, c, iou_thr=0.5, rule='voc'):
    """evaluate()'s greedy matching of one class: (its detections in descending score order -- Python's stable
    sorted(), ties keep input order --, the bool tp array in that order)."""
    cd = sorted(class_dets, key=lambda d: -d[4])      # stable: ties keep input order
    matched = {}
    tp = np.zeros(len(cd), dtype=bool)
    for i, (video, frame, _, bbox, _) in enumerate(cd):
        g = gt.get((video, frame, c))
        if g is None or len(g) == 0:
            continue
        used = matched.setdefault((video, frame), np.zeros(len(g), dtype=bool))
        if rule == 'ilsvrc':
            j = _ilsvrc_pick(np.asarray(bbox, dtype=np.float64), g, used, iou_thr)
            if j >= 0:
                tp[i] = True
                used[j] = True
            continue
        ious = _iou_1n(np.asarray(bbox, dtype=np.float64), g)
        ious = np.where(used, -1.0, ious)
        j = int(np.argmax(ious))
        if ious[j] >= iou_thr:
            tp[i] = True
            used[j] = True
    return cd, tp
