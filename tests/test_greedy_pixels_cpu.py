"""No GPU: the greedy loop of tests/pixtrack_spec.py, the rule of ops.track_volume_pixels, against the design of the seeded case -- so that
the device's comparison with the spec (test_greedy_pixels_gpu.py) cannot be vacuous -- and the symbol's declaration."""
import numpy as np

import greedy_pixel_cases as gc
import pixtrack_cases as pc


def test_symbol_is_declared():
    from vdetlib_amd import _lib
    res, args = _lib.SYMBOLS['vdet_track_volume_pixels']
    assert len(args) == 20


def test_case_is_what_it_says():
    (images, boxes, scores, posa, posb), _ = gc.main_case()
    assert images.shape == (gc.F, gc.H, gc.W, 3) and boxes.shape == (gc.F, gc.B, 4) and scores.shape == (gc.F, gc.B, gc.C)
    for f in range(gc.F):
        ta, tb = boxes[f, gc.IA], boxes[f, gc.IB]
        assert gc.iou(ta, tb) == 0.0                                              # non-overlapping walks
        assert ta.tolist() == gc.box_of(posa[f], gc.WA, gc.HA) and tb.tolist() == gc.box_of(posb[f], gc.WB, gc.HB)
        for i in gc.IJA:
            assert 0.3 <= gc.iou(boxes[f, i], ta) < 1.0
        for i in gc.IJB:
            assert 0.3 <= gc.iou(boxes[f, i], tb) < 1.0
        for i in gc.IDIS:
            assert gc.iou(boxes[f, i], ta) < 0.3 and gc.iou(boxes[f, i], tb) < 0.3
    order = np.argsort(-scores[:, :, 0].reshape(-1).astype(np.float64), kind='stable')
    assert order[0] == gc.FA * gc.B + gc.IA and order[1] == (gc.FA + 1) * gc.B + gc.IJA[0] and order[2] == gc.FB * gc.B + gc.IB


def test_spec_on_the_main_case():
    (images, boxes, scores, posa, posb), (tracks, anchors, ntracks, bad) = gc.main_case()
    assert not bad
    assert tracks.shape == (gc.C, 3, gc.F, 5) and anchors.shape == (gc.C, 3, 3) and ntracks.dtype == np.int32
    # track 0 and track 1 of class 0 follow the two planted position tables exactly (confidence 1.0 everywhere: SAD 0)
    assert np.array_equal(tracks[0, 0], pc.rows_from_positions(posa, gc.WA, gc.HA, range(gc.F)))
    assert np.array_equal(tracks[0, 1], pc.rows_from_positions(posb, gc.WB, gc.HB, range(gc.F)))
    assert anchors[0, 0].tolist() == [gc.FA + 1, gc.IA, np.float32(0.99)]
    assert anchors[0, 1].tolist() == [gc.FB + 1, gc.IB, np.float32(0.95)]
    # the detection that is second in score order -- A's jittered copy on the next frame -- is explained by track 0: no anchor
    dup = [gc.FA + 2, gc.IJA[0]]
    assert all(anchors[0, t, :2].tolist() != dup for t in range(3))
    # as designed per class: class 0 fills its slots, its third anchor is a distractor; class 1 stops early by thres
    assert ntracks.tolist() == [3, 1]
    assert int(anchors[0, 2, 1]) in gc.IDIS and gc.THRES <= anchors[0, 2, 2] < 0.5
    assert anchors[1, 0].tolist() == [3, gc.IB, np.float32(0.9)]
    assert np.array_equal(tracks[1, 0], pc.rows_from_positions(posb, gc.WB, gc.HB, range(gc.F)))
    assert np.isnan(tracks[1, 1:]).all() and (anchors[1, 1:] == 0).all()
    # ... by thres: detections of class 1 are left, all below it
    assert (scores[:, [gc.IA] + list(gc.IJA) + list(gc.IDIS), 1] < gc.THRES).all()


def test_spec_takes_a_slot_for_an_untrackable_anchor():
    import pixtrack_spec as px
    (images, boxes, scores, posa, posb), want = gc.main_case()
    boxes, scores = boxes.copy(), scores.copy()
    boxes[7, gc.IDIS[0]] = [10, 10, 9.5, 30]                   # empty after truncation
    scores[7, gc.IDIS[0], 0] = 2.0
    tracks, anchors, ntracks, bad = px.track_volume_pixels(images, boxes, scores, **gc.MAIN)
    assert bad and ntracks.tolist() == [3, 1]
    assert np.isnan(tracks[0, 0]).all() and anchors[0, 0].tolist() == [8, gc.IDIS[0], 2.0]
    # it suppresses nothing: the next two slots are the main case's first two
    assert np.array_equal(tracks[0, 1:], want[0][0, :2]) and np.array_equal(anchors[0, 1:], want[1][0, :2])
