"""CPU-only: the host evaluator's additions (vdetlib_amd/eval.py) -- the ILSVRC VID rule, the keep-list adapter, the
flat ground-truth table -- and the rank-major gather of the device evaluator's streams (gloo, two ranks)."""
import os
import socket
from collections import defaultdict

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from vdetlib_amd import dist as vd
from vdetlib_amd import eval as vev


def _evaluate_before(dets, gt, iou_thr=0.5, classes=None):
    """evaluate() as it was before the ILSVRC rule was added (verbatim)."""
    by_class = defaultdict(list)
    for d in dets:
        by_class[d[2]].append(d)
    gt_classes = sorted(set(k[2] for k in gt)) if classes is None else list(classes)
    aps = {}
    for c in gt_classes:
        n_gt = sum(len(v) for k, v in gt.items() if k[2] == c)
        cd = sorted(by_class.get(c, []), key=lambda d: -d[4])
        matched = {}
        tp = np.zeros(len(cd), dtype=bool)
        for i, (video, frame, _, bbox, _) in enumerate(cd):
            g = gt.get((video, frame, c))
            if g is None or len(g) == 0:
                continue
            ious = vev._iou_1n(np.asarray(bbox, dtype=np.float64), g)
            used = matched.setdefault((video, frame), np.zeros(len(g), dtype=bool))
            ious = np.where(used, -1.0, ious)
            j = int(np.argmax(ious))
            if ious[j] >= iou_thr:
                tp[i] = True
                used[j] = True
        aps[c] = vev.average_precision(tp, n_gt)
    valid = [v for v in aps.values() if not np.isnan(v)]
    return aps, (float(np.mean(valid)) if valid else float('nan'))


def _random_case(seed, n_vid=3, F=6, C=4, per=12):
    rng = np.random.RandomState(seed)
    annots, dets = [], []
    for v in range(n_vid):
        name = 'v%d' % v
        tracks = []
        for k in range(3):
            x, y, w, h = rng.randint(0, 200), rng.randint(0, 200), rng.randint(4, 80), rng.randint(4, 80)
            cls = int(rng.randint(1, C + 1))
            tracks.append({'id': str(k), 'track': [{'frame': f + 1, 'bbox': [x + f, y, x + f + w, y + h], 'class_index': cls}
                                                   for f in range(F) if rng.rand() < 0.8]})
            for f in range(F):
                for _ in range(per // 3):
                    j = rng.randint(-8, 9, 4)
                    dets.append((name, f + 1, cls if rng.rand() < 0.8 else int(rng.randint(1, C + 2)),
                                 [float(x + f + j[0]), float(y + j[1]), float(x + f + w + j[2]), float(y + h + j[3])],
                                 float(np.round(rng.rand() * 4) / 4)))
        annots.append({'video': name, 'annotations': tracks})
    return annots, dets


def test_default_rule_unchanged():
    for seed in range(4):
        annots, dets = _random_case(seed)
        gt = vev.ground_truth_from_annots(annots)
        want = _evaluate_before(dets, gt)
        assert vev.evaluate(dets, gt) == want
        assert vev.evaluate(dets, gt, rule='voc') == want
        # (class 9 has no ground truth: NaN, compared through repr)
        assert repr(vev.evaluate(dets, gt, 0.3, classes=[1, 2, 9])) == repr(_evaluate_before(dets, gt, 0.3, classes=[1, 2, 9]))
    with pytest.raises(ValueError):
        vev.evaluate(dets, gt, rule='coco')


def test_ilsvrc_rule_small_box_threshold():
    # ground truth 20x20 (+1 convention: x2 - x1 + 1 = 20): thr = min(0.5, 400 / 900) = 0.444...
    gt = {('v', 1, 1): np.array([[0.0, 0.0, 19.0, 19.0]])}
    # detection 20 x 17 inside it: IoU = 340 / 400 = 0.85 -> tp either way
    # detection 20 x 9: IoU = 180 / 400 = 0.45 -> tp for ILSVRC only
    d_small = [('v', 1, 1, [0.0, 0.0, 19.0, 8.0], 0.9)]
    assert vev.evaluate(d_small, gt)[0][1] == 0.0
    assert vev.evaluate(d_small, gt, rule='ilsvrc')[0][1] == 1.0
    # a large ground truth keeps the 0.5 threshold: 200x200, thr = min(0.5, 40000/44100) = 0.5
    gt2 = {('v', 1, 1): np.array([[0.0, 0.0, 199.0, 199.0]])}
    d45 = [('v', 1, 1, [0.0, 0.0, 199.0, 89.0], 0.9)]            # IoU 0.45
    assert vev.evaluate(d45, gt2, rule='ilsvrc')[0][1] == 0.0


def test_ilsvrc_rule_largest_overlap_and_ties():
    # two ground truths; the detection overlaps the SECOND one more: VOC's arg-max and ILSVRC agree on it
    gt = {('v', 1, 1): np.array([[0.0, 0.0, 99.0, 99.0], [10.0, 0.0, 109.0, 99.0]])}
    d = [('v', 1, 1, [10.0, 0.0, 109.0, 99.0], 0.9), ('v', 1, 1, [10.0, 0.0, 109.0, 99.0], 0.8)]
    _, tp = vev.match_class(d, gt, 1, 0.5, 'ilsvrc')
    assert tp.tolist() == [True, True]                  # second detection takes the other ground truth (IoU 0.82)
    # equal IoU with two ground truths: the first wins
    gt = {('v', 1, 1): np.array([[0.0, 0.0, 99.0, 99.0], [0.0, 0.0, 99.0, 99.0]])}
    g = gt[('v', 1, 1)]
    assert vev._ilsvrc_pick(np.array([0.0, 0.0, 99.0, 99.0]), g, np.zeros(2, bool), 0.5) == 0
    assert vev._ilsvrc_pick(np.array([0.0, 0.0, 99.0, 99.0]), g, np.array([True, False]), 0.5) == 1
    # zero-width overlap never qualifies (iw > 0), nor does a NaN IoU
    assert vev._ilsvrc_pick(np.array([200.0, 0.0, 250.0, 99.0]), g, np.zeros(2, bool), 0.0) == -1
    assert vev._ilsvrc_pick(np.array([0.0, 0.0, -1.0, -1.0]), np.array([[0.0, 0.0, -1.0, -1.0]]), np.zeros(1, bool), 0.0) == -1


def test_ilsvrc_rule_hand_ap():
    gt = {('v', 1, 1): np.array([[0.0, 0.0, 9.0, 9.0]]), ('v', 2, 1): np.array([[50.0, 50.0, 59.0, 59.0]])}
    # 10x10 ground truths: thr = 100 / 400 = 0.25; IoU of a 10 x 3 box inside = 0.3
    dets = [('v', 1, 1, [0.0, 0.0, 9.0, 2.0], 0.9), ('v', 2, 1, [0.0, 0.0, 9.0, 9.0], 0.8),
            ('v', 2, 1, [50.0, 50.0, 59.0, 52.0], 0.7)]
    aps, m = vev.evaluate(dets, gt, rule='ilsvrc')
    assert aps[1] == pytest.approx(0.5 + 0.5 * 2 / 3, abs=1e-15) and m == aps[1]
    assert vev.evaluate(dets, gt)[0][1] == 0.0


def test_detections_from_keep_lists_order():
    F, B, C, cap = 2, 4, 3, 3
    rng = np.random.RandomState(0)
    boxes = rng.rand(F, B, 4).astype(np.float32)
    scores = rng.rand(F, B, C).astype(np.float32)
    keep_idx = np.full((F, C, cap), -1, np.int32)
    keep_cnt = np.array([[2, 0, 1], [3, 1, 0]], np.int32)
    keep_idx[0, 0, :2] = [3, 1]; keep_idx[0, 2, 0] = 2; keep_idx[1, 0] = [0, 2, 1]; keep_idx[1, 1, 0] = 3
    d = vev.detections_from_keep_lists('x', boxes, scores, keep_idx, keep_cnt)
    want = [(0, 0, 3), (0, 0, 1), (0, 2, 2), (1, 0, 0), (1, 0, 2), (1, 0, 1), (1, 1, 3)]
    assert [(t[1], t[2], t[3], t[4]) for t in d] == [
        (f + 1, c + 1, [float(v) for v in boxes[f, b]], float(scores[f, b, c])) for f, c, b in want]
    d2 = vev.detections_from_keep_lists('x', boxes, np.ascontiguousarray(scores.transpose(0, 2, 1)), keep_idx, keep_cnt,
                                        layout='FCB', class_base=0)
    assert [(t[1], t[2] + 1, t[3], t[4]) for t in d2] == [(t[1], t[2], t[3], t[4]) for t in d]


def test_gt_table_round_trip():
    annots, _ = _random_case(7)
    annots.append({'video': 'v1', 'annotations': [{'id': '9', 'track': [{'frame': 2, 'bbox': [1, 2, 3, 4], 'class_index': 2}]}]})
    tab = vev.gt_table_from_annots(annots)
    assert tab['videos'] == ['v0', 'v1', 'v2']
    assert tab['bbox'].dtype == np.float64 and tab['bbox'].shape == (len(tab['video']), 4)
    want = vev.ground_truth_from_annots(annots)
    got = vev.gt_from_table(tab)
    assert sorted(got) == sorted(want)
    for k in want:
        assert np.array_equal(got[k], want[k])


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _stream_of(rank):
    n = 5 + 3 * rank
    g = torch.Generator().manual_seed(rank)
    return (torch.randint(0, 4, (n,), dtype=torch.int32, generator=g),
            torch.round(torch.rand(n, dtype=torch.float64, generator=g) * 4) / 4,
            torch.randint(0, 2, (n,), dtype=torch.uint8, generator=g))


def _rank_worker(rank, world, port, ret):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), WORLD_SIZE=str(world), RANK=str(rank),
                      LOCAL_RANK=str(rank))
    vd.init(backend="gloo")
    s, sc, tp = vd.gather_eval_stream(*_stream_of(rank), group=dist.group.WORLD)
    parts = [_stream_of(r) for r in range(world)]
    ok = (torch.equal(s, torch.cat([p[0] for p in parts])) and torch.equal(sc, torch.cat([p[1] for p in parts]))
          and torch.equal(tp, torch.cat([p[2] for p in parts])))
    ok = ok and s.dtype == torch.int32 and sc.dtype == torch.float64 and tp.dtype == torch.uint8
    ret[rank] = bool(ok)
    dist.barrier()
    dist.destroy_process_group()


def test_world2_gloo_eval_stream_rank_major():
    world = 2
    ret = mp.Manager().dict()
    mp.spawn(_rank_worker, args=(world, _free_port(), ret), nprocs=world, join=True)
    assert dict(ret) == {0: True, 1: True}


def test_single_process_stream_passes_through():
    st = _stream_of(0)
    out = vd.gather_eval_stream(*st)
    assert all(a is b for a, b in zip(out, st))
