"""-m gpu: ops.tubelets_overlap (csrc/tcn_kernels.hpp: tubelets_overlap_kernel over the evaluator's ground-truth table)
against the mirrored utils.protocol.tubelets_overlap on protocol dicts built from the same tensors: gt_overlap equal as
f64 bits, mean_iou equal to the sequential f64 mean, gt flags equal.  Boxes are integer-valued (tracks_to_proto's int()
truncation then changes nothing) except in the one fractional case, which follows the rule of include/vdet_hip.h: the
device measures the UNtruncated f32 box."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NAN = float('nan')
C, T, F = 4, 3, 6


def _annot(name='ov_vid'):
    """class 1: one object on frames 1..6 except frame 3; a second class-1 object on frames 4..5 (two boxes of the class
    on one frame); class 3: one object on every frame (a tubelet of class 2 on the same place sees only another class);
    class 4: an object on every frame (a tubelet lies exactly on it)."""
    a1 = [{'frame': f, 'bbox': [100 + 2 * f, 100, 199 + 2 * f, 179], 'class_index': 1, 'class': 'c1'} for f in (1, 2, 4, 5, 6)]
    a2 = [{'frame': f, 'bbox': [120 + 2 * f, 90, 215 + 2 * f, 185], 'class_index': 1, 'class': 'c1'} for f in (4, 5)]
    a3 = [{'frame': f, 'bbox': [400, 200 + f, 520, 330 + f], 'class_index': 3, 'class': 'c3'} for f in range(1, F + 1)]
    a4 = [{'frame': f, 'bbox': [600 + 3 * f, 50, 700 + 3 * f, 140], 'class_index': 4, 'class': 'c4'} for f in range(1, F + 1)]
    return {'video': name, 'annotations': [{'id': str(i), 'track': t} for i, t in enumerate((a1, a2, a3, a4))]}


def _tracks(frac=False):
    tr = np.full((C, T, F, 5), NAN, np.float32)
    nt = np.array([2, 1, 1, 2], np.int32)
    rng = np.random.RandomState(3)
    for f in range(F):                                  # class 1, tubelet 0: near object 1 on every frame (frame 3: no gt)
        tr[0, 0, f] = [103 + 2 * (f + 1), 97, 196 + 2 * (f + 1), 183, 0.9]
    for f in (2, 3, 4):                                 # class 1, tubelet 1: frames 3..5 between the two objects, with a gap
        tr[0, 1, f] = [112 + 2 * (f + 1), 95, 207 + 2 * (f + 1), 181, 0.8]
    tr[0, 1, 3] = NAN
    tr[0, 2, 0] = [100, 100, 199, 179, 0.7]             # t >= ntracks: must be ignored
    for f in range(1, F):                               # class 2: on the class-3 object -> 0 everywhere
        tr[1, 0, f] = [400, 200 + f + 1, 520, 330 + f + 1, 0.6]
    for f in range(F):                                  # class 3: shifted copies
        tr[2, 0, f] = [400 + rng.randint(-9, 10), 200 + f + 1, 520, 330 + f + 1 + rng.randint(-9, 10), 0.5]
    for f in range(F):                                  # class 4, tubelet 0: exactly the ground truth -> gt == 1
        tr[3, 0, f] = [600 + 3 * (f + 1), 50, 700 + 3 * (f + 1), 140, 0.4]
    tr[3, 1, 2] = [5, 5, 50, 50, 0.3]                   # class 4, tubelet 1: one box, far away
    if frac:
        tr[..., :4] += rng.uniform(0.05, 0.95, tr[..., :4].shape).astype(np.float32)
    return tr, nt


def _host(tr, nt, annot, truncate=True):
    """The mirrored tubelets_overlap on protos of the same tensors -> (gt_overlap, mean_iou, gt) arrays."""
    from vdetlib_amd import ops
    from vdetlib_amd.utils.protocol import tubelets_overlap, tubelets_proto_from_tracks_proto
    an = np.ones((C, T, 3), np.float32)
    ov = np.full((C, T, F), NAN, np.float64)
    mean = np.full((C, T), NAN, np.float64)
    flag = np.zeros((C, T), np.int32)
    for c in range(C):
        tp = ops.tracks_to_proto(annot['video'], tr[c], an[c], int(nt[c]))
        if not truncate:                                 # the un-truncated f32 coordinates, as python floats
            for t, track in enumerate(tp['tracks']):
                for box in track:
                    box['bbox'] = [float(v) for v in tr[c, t, box['frame'] - 1, :4]]
        tubs = tubelets_overlap(tubelets_proto_from_tracks_proto(tp['tracks'], c + 1), annot, c + 1)
        for t, tub in enumerate(tubs):
            s = 0.0
            for box in tub['boxes']:
                ov[c, t, box['frame'] - 1] = float(box['gt_overlap'])
                s = s + float(box['gt_overlap'])          # sequential, frame order
            mean[c, t] = s / len(tub['boxes'])
            flag[c, t] = tub['gt']
    return ov, mean, flag


def _same_f64(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a.view(np.uint64)[~na], b.view(np.uint64)[~nb])


def _device(ev, name, tr, nt, boxes=None):
    import torch
    from vdetlib_amd import ops
    bx = None if boxes is None else torch.from_numpy(boxes).cuda()
    got = ops.tubelets_overlap(ev, name, torch.from_numpy(tr).cuda(), torch.from_numpy(nt).cuda(), boxes=bx)
    return [g.cpu().numpy() for g in got]


def test_cases_against_the_mirrored_protocol_function():
    from vdetlib_amd import eval as vev, ops
    annot = _annot()
    tr, nt = _tracks()
    ev = ops.DetEvaluator(vev.gt_table_from_annots([annot]))
    ov, mean, flag = _device(ev, annot['video'], tr, nt)
    h_ov, h_mean, h_flag = _host(tr, nt, annot)
    assert ov.dtype == np.float64 and _same_f64(ov, h_ov)
    assert _same_f64(mean, h_mean)
    assert np.array_equal(flag, h_flag)
    # the cases are what they claim to be
    assert ov[0, 0, 2] == 0.0 and (ov[0, 0, [0, 1, 3, 4, 5]] > 0.5).all()          # a frame without ground truth
    two = [vev.ground_truth_from_annots([annot])[(annot['video'], 5, 1)]]
    assert len(two[0]) == 2 and ov[0, 1, 4] == max(float(ops.iou([g], [tr[0, 1, 4, :4]])[0, 0]) for g in two[0])   # the max of two
    assert np.isnan(ov[0, 1, 3]) and np.isnan(ov[0, 2]).all() and np.isnan(mean[0, 2]) and flag[0, 2] == 0
    assert (ov[1, 0, 1:] == 0.0).all() and np.isnan(ov[1, 0, 0]) and mean[1, 0] == 0.0     # only another class there
    assert flag[3, 0] == 1 and mean[3, 0] == 1.0 and (ov[3, 0] == 1.0).all()      # exactly on a ground-truth track
    assert flag.sum() == 1 and ov[3, 1, 2] == 0.0
    # the evaluator and the overlap share ONE uploaded table
    gtb, gto, gtm, K = ev.device_table()
    assert gtb.data_ptr() == ev._gt_boxes.data_ptr() and K == len(ev.classes)
    # a video the table does not know: nothing overlaps
    ov_u, mean_u, flag_u = _device(ev, 'no_such_video', tr, nt)
    assert np.array_equal(np.isnan(ov_u), np.isnan(ov)) and (ov_u[~np.isnan(ov_u)] == 0.0).all() and flag_u.sum() == 0
    assert (mean_u[~np.isnan(mean_u)] == 0.0).all()
    # a gt_table dict in place of the evaluator
    ov_t, _, _ = _device(vev.gt_table_from_annots([annot]), annot['video'], tr, nt)
    assert _same_f64(ov_t, ov)
    # boxes [C,T,F,4] measured instead of the track rows
    bx = np.ascontiguousarray(tr[..., :4]) + np.float32(2.0)
    tr2 = tr.copy()
    tr2[..., :4] = bx
    ov_b, mean_b, _ = _device(ev, annot['video'], tr, nt, boxes=bx)
    ov_r, mean_r, _ = _device(ev, annot['video'], tr2, nt)
    assert _same_f64(ov_b, ov_r) and _same_f64(mean_b, mean_r) and not _same_f64(ov_b, ov)


def test_fractional_boxes_follow_the_stated_rule():
    """include/vdet_hip.h: the device widens the f32 coordinates as they are; tracks_to_proto truncates them.  So the device
    equals the mirrored function on the UNtruncated boxes, and differs from it on the truncated ones."""
    from vdetlib_amd import eval as vev, ops
    annot = _annot()
    tr, nt = _tracks(frac=True)
    ev = ops.DetEvaluator(vev.gt_table_from_annots([annot]))
    ov, mean, flag = _device(ev, annot['video'], tr, nt)
    h_ov, h_mean, h_flag = _host(tr, nt, annot, truncate=False)
    assert _same_f64(ov, h_ov) and _same_f64(mean, h_mean) and np.array_equal(flag, h_flag)
    t_ov, _, _ = _host(tr, nt, annot, truncate=True)
    assert not _same_f64(ov, t_ov)


def test_tracker_tubelets_and_errors():
    """Tubelets of the tracker on a planted video (integer boxes), every (c, t < ntracks[c]); argument errors."""
    import torch
    import synth
    from vdetlib_amd import eval as vev, ops
    from vdetlib_amd.utils.protocol import tubelets_overlap, tubelets_proto_from_tracks_proto
    boxes, scores, annot = synth.vid_with_objects(91, 12, 100, 5)
    tb, ts = torch.from_numpy(boxes).cuda(), torch.from_numpy(scores).cuda()
    tr, an, nt = ops.track_volume(tb, ts, nms_thres=0.3, thres=0.5, max_tracks=4, link_thres=0.4)
    ev = ops.DetEvaluator(vev.gt_table_from_annots([annot]))
    ov, mean, flag = (g.cpu().numpy() for g in ops.tubelets_overlap(ev, annot['video'], tr, nt))
    trh, anh, nth = tr.cpu().numpy(), an.cpu().numpy(), nt.cpu().numpy()
    assert nth.sum() >= 3
    n_pos = 0
    for c in range(5):
        tp = ops.tracks_to_proto(annot['video'], trh[c], anh[c], int(nth[c]))
        tubs = tubelets_overlap(tubelets_proto_from_tracks_proto(tp['tracks'], c + 1), annot, c + 1)
        for t, tub in enumerate(tubs):
            want = np.full(12, NAN)
            for box in tub['boxes']:
                want[box['frame'] - 1] = float(box['gt_overlap'])
            assert _same_f64(ov[c, t], want), (c, t)
            assert flag[c, t] == tub['gt']
            n_pos += int(np.nansum(want) > 0)
        assert np.isnan(ov[c, int(nth[c]):]).all()
    assert n_pos >= 3
    with pytest.raises(ValueError):
        ops.tubelets_overlap(ev, annot['video'], tr.double(), nt)
    with pytest.raises(ValueError):
        ops.tubelets_overlap(ev, annot['video'], tr, nt.long())
    with pytest.raises(ValueError):
        ops.tubelets_overlap(ev, annot['video'], tr, nt[:-1])
    with pytest.raises(ValueError):
        ops.tubelets_overlap(ev, annot['video'], tr.cpu(), nt)
    with pytest.raises(ValueError):
        ops.tubelets_overlap(ev, annot['video'], tr, nt, boxes=tr[..., :3].contiguous())
    again = ops.tubelets_overlap(ev, annot['video'], tr, nt)[0].cpu().numpy()
    assert _same_f64(again, ov)
