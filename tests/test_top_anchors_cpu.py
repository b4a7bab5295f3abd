"""CPU: what the device anchor selection and the anchor route's batch forms do above the kernels -- the built library
exports the new entry points with the declared prototypes, and the ops wrappers check their arguments and refuse host
tensors (there is no CPU path to fall back to)."""
import ctypes
import inspect

import pytest


def test_library_exports_the_new_entry_points():
    from vdetlib_amd import _lib
    lib = _lib.load_library()
    vp, i64, ci, f64 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_double
    want = {
        "vdet_top_anchors": [vp, vp, vp, i64, i64, i64, ci, ci, ci, f64, vp, i64, vp, vp, vp, vp],
        "vdet_track_from_anchors_batch": [vp, vp, vp, i64, i64, vp, vp, vp, i64, ci, f64, ci, vp, vp, vp],
        "vdet_anchor_propagate_tracks_batch": [vp, vp, vp, vp, vp, vp, vp, i64, i64, i64, ci, vp, vp],
    }
    for name, args in want.items():
        fn = getattr(lib, name)
        assert fn.restype is ci and list(fn.argtypes) == args, name
        assert list(_lib.SYMBOLS[name][1]) == args
    # a NULL context is refused by every one of them, without a device
    assert lib.vdet_top_anchors(None, None, None, 1, 1, 1, 1, 0, 0, 0.0, None, 0, None, None, None, None) == _lib.VDET_EINVAL
    assert lib.vdet_track_from_anchors_batch(None, None, None, 1, 1, None, None, None, 1, 1, 0.5, 0, None, None, None) == _lib.VDET_EINVAL
    assert lib.vdet_anchor_propagate_tracks_batch(None, None, None, None, None, None, None, 1, 1, 1, 1, None, None) == _lib.VDET_EINVAL


def test_signatures():
    from vdetlib_amd import ops
    assert list(inspect.signature(ops.top_anchors).parameters) == [
        'boxes', 'scores', 'top_num', 'mode', 'score_thresh', 'frame_off', 'sync', 'ctx']
    assert list(inspect.signature(ops.track_from_anchors_batch).parameters) == [
        'boxes', 'frame_off', 'anchor_frames', 'anchor_boxes', 'anchor_scores', 'link_thres', 'max_frames', 'sync', 'ctx']
    assert list(inspect.signature(ops.anchor_propagate_tracks_batch).parameters) == ['batch_out', 'boxes', 'scores', 'sync', 'ctx']


def test_argument_checks_without_a_device():
    import torch
    from vdetlib_amd import ops
    boxes, scores = torch.zeros((5, 8, 4)), torch.zeros((5, 8, 2))
    for fn in (lambda: ops.top_anchors(boxes.double(), scores, 2),
               lambda: ops.top_anchors(boxes, scores.double(), 2),
               lambda: ops.top_anchors(boxes, scores, 0),
               lambda: ops.top_anchors(boxes, scores, 1025),
               lambda: ops.top_anchors(boxes, scores, 129, mode='frame'),
               lambda: ops.top_anchors(boxes, scores, 2, mode='clip'),
               lambda: ops.top_anchors(boxes, scores, 2, mode='frame', frame_off=[0, 2, 5]),
               lambda: ops.top_anchors(boxes[..., :3], scores, 2),
               lambda: ops.top_anchors(boxes[:4], scores, 2),
               lambda: ops.top_anchors(boxes, scores[:, :7], 2),
               lambda: ops.top_anchors(boxes, scores, 2, frame_off=[0, 2, 4]),
               lambda: ops.top_anchors(boxes, scores, 2, frame_off=[0, 3, 3, 5]),
               lambda: ops.top_anchors(boxes, scores, 2),                       # host tensors: there is no CPU path
               lambda: ops.top_anchors(boxes, scores, 1024),
               lambda: ops.top_anchors(boxes, scores, 128, mode='frame')):
        with pytest.raises(ValueError):
            fn()
    off = [0, 2, 5]
    fr = torch.zeros((2, 2, 3), dtype=torch.int32)
    ab = torch.zeros((2, 2, 3, 4))
    for fn in (lambda: ops.track_from_anchors_batch(boxes.double(), off, fr, ab),
               lambda: ops.track_from_anchors_batch(boxes, off, fr.long(), ab),
               lambda: ops.track_from_anchors_batch(boxes, off, fr, ab.double()),
               lambda: ops.track_from_anchors_batch(boxes, off, fr, ab, torch.zeros((2, 2, 3), dtype=torch.float64)),
               lambda: ops.track_from_anchors_batch(boxes, [0, 2, 4], fr, ab),
               lambda: ops.track_from_anchors_batch(boxes, off, fr[:1], ab),
               lambda: ops.track_from_anchors_batch(boxes, off, fr, ab[:, :, :2]),
               lambda: ops.track_from_anchors_batch(boxes, off, fr, ab, torch.zeros((2, 2, 2))),
               lambda: ops.track_from_anchors_batch(boxes, off, fr, ab)):          # host tensors
        with pytest.raises(ValueError):
            fn()
    out = dict(tracks=[t.view(2, 3, n, 5) for t, n in zip(torch.zeros(2 * 3 * 5 * 5).split([60, 90]), (2, 3))],
               anchors=torch.zeros((2, 2, 3, 3)), ntracks=torch.zeros((2, 2), dtype=torch.int32), frame_off=off)
    for fn in (lambda: ops.anchor_propagate_tracks_batch(out, boxes.double(), scores),
               lambda: ops.anchor_propagate_tracks_batch(out, boxes[:4], scores),
               lambda: ops.anchor_propagate_tracks_batch(out, boxes, scores[..., :1]),
               lambda: ops.anchor_propagate_tracks_batch(dict(out, ntracks=out['ntracks'].long()), boxes, scores),
               lambda: ops.anchor_propagate_tracks_batch(dict(out, anchors=out['anchors'][:, :, :2]), boxes, scores),
               lambda: ops.anchor_propagate_tracks_batch(out, boxes, scores)):     # host tensors
        with pytest.raises(ValueError):
            fn()
    assert 'det' not in out
