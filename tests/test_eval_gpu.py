"""-m gpu: the device evaluator (ops.DetEvaluator, eval_kernels.hpp) against the host evaluator (vdetlib_amd/eval.py)
on the same detections, which reach the host through eval.py's adapters: AP per class and mAP within 1e-12 (the AP
sum's order differs from numpy's pairwise sum), the per-class tp sequence in sorted order identical, both rules."""
import math

import numpy as np
import pytest

import synth

pytestmark = pytest.mark.gpu

RULES = ('voc', 'ilsvrc')


def _host_tp(dets, gt, classes, rule, iou_thr=0.5):
    from vdetlib_amd import eval as vev
    out = {}
    for c in classes:
        cd, tp = vev.match_class([d for d in dets if d[2] == c], gt, c, iou_thr, rule)
        out[c] = (np.array([d[4] for d in cd], dtype=np.float64), tp)
    return out


def _check(ev, dets, annots, rule, classes=None, iou_thr=0.5):
    """device == host on the same detections: APs, mAP, and the sorted (score, tp) sequence of every class."""
    from vdetlib_amd import eval as vev
    gt = vev.ground_truth_from_annots(annots)
    aps_h, map_h = vev.evaluate(dets, gt, iou_thr, classes=classes, rule=rule)
    aps_d, map_d, (cls, sc, tp, perm) = ev.compute(return_order=True)
    assert sorted(aps_d) == sorted(aps_h)
    for c in aps_h:
        if math.isnan(aps_h[c]):
            assert math.isnan(aps_d[c]), c
        else:
            assert abs(aps_d[c] - aps_h[c]) <= 1e-12, (c, aps_d[c], aps_h[c])
    assert (math.isnan(map_h) and math.isnan(map_d)) or abs(map_d - map_h) <= 1e-12
    cls, sc, tp, perm = (t.cpu().numpy() for t in (cls, sc, tp, perm))
    cls, sc, tp = cls[perm], sc[perm], tp[perm]
    host = _host_tp(dets, gt, aps_h.keys(), rule, iou_thr)
    for c, (hs, htp) in host.items():
        m = cls == c
        assert np.array_equal(sc[m], hs), c
        assert np.array_equal(tp[m], htp), c
    return aps_d, map_d


def test_hand_built_known_ap():
    import torch
    from vdetlib_amd import eval as vev, ops
    annots = [{'video': 'v', 'annotations': [
        {'id': '0', 'track': [{'frame': 1, 'bbox': [10, 10, 59, 59], 'class_index': 1}]},
        {'id': '1', 'track': [{'frame': 2, 'bbox': [100, 100, 149, 149], 'class_index': 1}]}]}]
    nan = float('nan')
    tracks = np.full((1, 3, 2, 5), nan, np.float32)
    scores = np.full((1, 3, 2), nan, np.float64)
    tracks[0, 0, 0, :4] = [10, 10, 59, 59]; scores[0, 0, 0] = 0.9        # tp
    tracks[0, 1, 1, :4] = [300, 300, 349, 349]; scores[0, 1, 1] = 0.8    # fp
    tracks[0, 2, 1, :4] = [102, 101, 150, 149]; scores[0, 2, 1] = 0.7    # tp
    ev = ops.DetEvaluator(vev.gt_table_from_annots(annots))
    n = ev.add_tracks('v', torch.from_numpy(tracks).cuda(), torch.tensor([3], dtype=torch.int32).cuda(),
                      torch.from_numpy(scores).cuda())
    assert n == 3
    aps, m = ev.compute()
    assert abs(aps[1] - (0.5 + 0.5 * 2 / 3)) <= 1e-15 and m == aps[1]
    cls, sc, tp = (t.cpu().numpy() for t in ev.stream())
    assert cls.tolist() == [1, 1, 1] and sc.tolist() == [0.9, 0.8, 0.7] and tp.tolist() == [True, False, True]


def _tubelet_videos(seeds=(61, 62, 63), F=24, B=120, C=5, T=4):
    import torch
    from vdetlib_amd import ops
    vids = []
    for seed in seeds:
        boxes, scores, annot = synth.vid_with_objects(seed, F, B, C)
        tb, ts = torch.from_numpy(boxes).cuda(), torch.from_numpy(scores).cuda()
        tr, an, nt = ops.track_volume(tb, ts, nms_thres=0.3, thres=0.5, max_tracks=T, link_thres=0.4)
        det, pooled, ob = ops.rescore_tracks(tr, nt, tb, ts, overlap_thres=0.5, window=3)
        vids.append((annot, boxes, scores, tr, nt, pooled, ob))
    return vids


@pytest.mark.parametrize("rule", RULES)
def test_tubelets_match_host(rule):
    from vdetlib_amd import eval as vev, ops
    vids = _tubelet_videos()
    annots = [v[0] for v in vids]
    ev = ops.DetEvaluator(vev.gt_table_from_annots(annots), rule=rule)
    dets = []
    for annot, _, _, tr, nt, pooled, ob in vids:
        ev.add_tracks(annot['video'], tr, nt, pooled, ob)
        dets += vev.detections_from_tracks(annot['video'], tr.cpu().numpy(), nt.cpu().numpy(), pooled.cpu().numpy(),
                                           ob.cpu().numpy())
    assert ev.stream()[0].numel() == len(dets)
    aps, m = _check(ev, dets, annots, rule)
    assert m > 0.5
    # the track rows as boxes, f32 scores (the track's own score column)
    ev2 = ops.DetEvaluator(vev.gt_table_from_annots(annots), rule=rule)
    dets2 = []
    for annot, _, _, tr, nt, _, _ in vids:
        sc = tr[..., 4].contiguous()
        ev2.add_tracks(annot['video'], tr, nt, sc)
        dets2 += vev.detections_from_tracks(annot['video'], tr.cpu().numpy(), nt.cpu().numpy(), sc.cpu().numpy())
    _check(ev2, dets2, annots, rule)


def _planted_video(seed, F, B, C, n_obj=6):
    """VID-shaped frames (F x <= B boxes x C classes) with planted ground truth: synth.vid_with_objects."""
    return synth.vid_with_objects(seed, F, B, C, n_obj=n_obj)


@pytest.mark.parametrize("rule", RULES)
def test_keep_lists_vid_shape(rule):
    import torch
    from vdetlib_amd import eval as vev, ops
    F, B, C = 200, 300, 30
    annots, dets = [], []
    per_video = []
    for seed in (71, 72):
        boxes, scores, annot = _planted_video(seed, F, B, C)
        annots.append(annot)
        tb, ts = torch.from_numpy(boxes).cuda(), torch.from_numpy(scores).cuda()
        ki, kc = ops.nms_volume(tb, ts, 0.5, topk=100, cap=100)
        per_video.append((annot['video'], tb, ts, ki, kc))
        dets += vev.detections_from_keep_lists(annot['video'], boxes, scores, ki.cpu().numpy(), kc.cpu().numpy())
    assert len(dets) > 500000
    ev = ops.DetEvaluator(vev.gt_table_from_annots(annots), rule=rule)
    for name, tb, ts, ki, kc in per_video:
        ev.add_keep_lists(name, tb, ts, ki, kc)
    _check(ev, dets, annots, rule)


def _edge_case(seed):
    """Tubelet arrays built by hand: scores quantised to 0.25 (ties across frames, tracks and videos), +-0.0, NaN gaps,
    degenerate boxes (zero unions: NaN / inf IoUs), ground truths smaller than 10 px, a class without detections, a class
    without ground truth, a video missing from the table."""
    rng = np.random.RandomState(seed)
    C, T, F = 5, 6, 7
    names = ['e0', 'e1', 'e2']                     # e2 is not in the table
    annots, vids = [], []
    for vi, name in enumerate(names):
        objs = []
        for k in range(4):
            cls = [1, 2, 4][k % 3]                 # class 3: no ground truth; class 4 gets ground truth, no detections
            small = k == 1
            x, y = rng.randint(0, 100), rng.randint(0, 100)
            w, h = (rng.randint(2, 9), rng.randint(2, 9)) if small else (rng.randint(20, 60), rng.randint(20, 60))
            objs.append((cls, x, y, w, h))
        if vi < 2:
            tr = []
            for k, (cls, x, y, w, h) in enumerate(objs):
                tr.append({'id': str(k), 'track': [{'frame': f + 1, 'bbox': [x + f, y, x + f + w - 1, y + h - 1], 'class_index': cls}
                                                   for f in range(F)]})
            # a degenerate ground truth (zero width and height with the +1 convention) in frame 1 of class 1
            tr.append({'id': 'z', 'track': [{'frame': 1, 'bbox': [5, 5, 4, 4], 'class_index': 1}]})
            annots.append({'video': name, 'annotations': tr})
        tracks = np.full((C, T, F, 5), np.nan, np.float32)
        scores = np.full((C, T, F), np.nan, np.float64)
        for c in range(C):
            if c + 1 == 4:
                continue
            for t in range(T):
                cls, x, y, w, h = objs[t % len(objs)]
                for f in range(F):
                    if rng.rand() < 0.2:
                        continue
                    j = rng.randint(-3, 4, 4)
                    b = [x + f + j[0], y + j[1], x + f + w - 1 + j[2], y + h - 1 + j[3]]
                    if rng.rand() < 0.1:
                        b = [5, 5, 4, 4]                       # zero area: a zero union with the degenerate ground truth
                    if rng.rand() < 0.05:
                        b = [5, 5, 3, 4]                       # negative width
                    tracks[c, t, f, :4] = b
                    s = np.round(rng.rand() * 4) / 4
                    scores[c, t, f] = -0.0 if s == 0 and rng.rand() < 0.5 else s
        vids.append((name, tracks, scores))
    return annots, vids


@pytest.mark.parametrize("rule", RULES)
def test_ties_and_edges(rule):
    import torch
    from vdetlib_amd import eval as vev, ops
    annots, vids = _edge_case(5)
    table = vev.gt_table_from_annots(annots)
    for classes in (None, [2, 1, 3], [1]):
        ev = ops.DetEvaluator(table, classes=classes, rule=rule)
        dets = []
        for name, tracks, scores in vids:
            C, T = scores.shape[:2]
            nt = np.array([T, T - 1, T, T, 2], np.int32)[:C]
            ev.add_tracks(name, torch.from_numpy(tracks).cuda(), torch.from_numpy(nt).cuda(), torch.from_numpy(scores).cuda())
            dets += vev.detections_from_tracks(name, tracks, nt, scores)
        aps, m = _check(ev, dets, annots, rule, classes=classes)
        if classes is None:
            assert aps[4] == 0.0 and 3 not in aps                 # ground truth but no detections / vice versa
        if classes == [2, 1, 3]:
            assert math.isnan(aps[3])


def test_keep_list_errors():
    import torch
    from vdetlib_amd import eval as vev, ops
    annots = [{'video': 'v', 'annotations': [{'id': '0', 'track': [{'frame': 1, 'bbox': [0, 0, 9, 9], 'class_index': 1}]}]}]
    ev = ops.DetEvaluator(vev.gt_table_from_annots(annots))
    boxes = torch.zeros((1, 3, 4), dtype=torch.float32).cuda()
    boxes[0, :, 2:] = 9
    good = torch.tensor([[[0.9], [0.5], [0.7]]], dtype=torch.float32).cuda()     # [F,B,C]
    kc = torch.tensor([[3]], dtype=torch.int32).cuda()
    assert ev.add_keep_lists('v', boxes, good, torch.tensor([[[0, 2, 1]]], dtype=torch.int32).cuda(), kc) == 3
    with pytest.raises(ValueError):                                                # increasing score
        ev.add_keep_lists('v', boxes, good, torch.tensor([[[0, 1, 2]]], dtype=torch.int32).cuda(), kc)
    bad = good.clone()
    bad[0, 2, 0] = float('nan')
    with pytest.raises(ValueError):                                                # kept NaN
        ev.add_keep_lists('v', boxes, bad, torch.tensor([[[0, 2, 1]]], dtype=torch.int32).cuda(), kc)
    assert ev.stream()[0].numel() == 3                                             # failed adds left the stream alone
    with pytest.raises(ValueError):
        ev.add_keep_lists('v', boxes, good.double(), torch.tensor([[[0, 2, 1]]], dtype=torch.int32).cuda(), kc)
    aps, _ = ev.compute()
    assert aps[1] == 1.0


def test_forms_agree():
    import torch
    from vdetlib_amd import eval as vev, ops
    F, B, C, T = 16, 120, 5, 4
    vids = [synth.vid_with_objects(s, F + 4 * i, B, C) for i, s in enumerate((81, 82, 83, 84))]
    annots = [v[2] for v in vids]
    names = [a['video'] for a in annots]
    boxes = torch.from_numpy(np.concatenate([v[0] for v in vids])).cuda()
    scores = torch.from_numpy(np.concatenate([v[1] for v in vids])).cuda()
    off = np.cumsum([0] + [v[0].shape[0] for v in vids])
    out = ops.video_batch(boxes, scores, off, nms_thres=0.3, thres=0.5, max_tracks=T, link_thres=0.4, overlap_thres=0.5, window=3)
    table = vev.gt_table_from_annots(annots)
    for rule in RULES:
        eb = ops.DetEvaluator(table, rule=rule)
        eb.add_batch(names, out)
        et = ops.DetEvaluator(table, rule=rule)
        dets = []
        for v, name in enumerate(names):
            et.add_tracks(name, out['tracks'][v], out['ntracks'][v].contiguous(), out['pooled'][v], out['tboxes'][v])
            dets += vev.detections_from_tracks(name, out['tracks'][v].cpu().numpy(), out['ntracks'][v].cpu().numpy(),
                                               out['pooled'][v].cpu().numpy(), out['tboxes'][v].cpu().numpy())
        for a, b in zip(eb.stream(), et.stream()):
            assert torch.equal(a, b)
        assert eb.compute() == et.compute()
        _check(eb, dets, annots, rule)
        # two evaluators on disjoint halves, streams concatenated in order == one evaluator on all videos
        h1, h2 = ops.DetEvaluator(table, rule=rule), ops.DetEvaluator(table, rule=rule)
        for v, name in enumerate(names):
            (h1 if v < 2 else h2).add_tracks(name, out['tracks'][v], out['ntracks'][v].contiguous(), out['pooled'][v],
                                             out['tboxes'][v])
        for a, b, c in zip(h1.stream(raw=True), h2.stream(raw=True), et.stream(raw=True)):
            assert torch.equal(torch.cat([a, b]), c)
