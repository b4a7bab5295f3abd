"""CPU: what the anchor route does above the C-ABI.
 * the host logic of the dict-level `anchor_propagate` (vdetlib_amd/vdet/tubelet_cls.py) -- all tubelets of a call in ONE
   `hot.anchor_argmax`, each anchor frame's detections once, only the anchor frames read -- with the ORACLE standing in for
   the device call, against the reference's recorded output (proto_golden, G11);
 * the argument checks of ops.track_from_anchors / ops.anchor_propagate_tracks that need no device."""
import copy

import numpy as np
import pytest

import synth
from test_pipeline_gpu import _close, _py


def _oracle_argmax(oracle, calls):
    def anchor_argmax(anchor_boxes, anchor_group, det_boxes_list):
        calls.append((len(anchor_boxes), len(det_boxes_list)))
        return np.array([int(np.argmax(oracle.iou(np.asarray(b, dtype=np.float64)[None], det_boxes_list[g])[0]))
                         for b, g in zip(anchor_boxes, anchor_group)], dtype=np.int64)
    return anchor_argmax


def test_dict_anchor_propagate_batches_into_one_call(oracle, proto_golden, monkeypatch):
    from vdetlib_amd import hot
    from vdetlib_amd.vdet import tubelet_cls as T
    calls = []
    monkeypatch.setattr(hot, 'anchor_argmax', _oracle_argmax(oracle, calls))
    case = synth.proto_case()
    g = proto_golden['protocol_misc']
    track_proto = proto_golden['greedy_track']['plain_det_c1']
    n_tub = len(track_proto['tracks'])
    anchor_frames = {b['frame'] for t in track_proto['tracks'] for b in t if b['anchor'] == 0}
    assert n_tub > 1
    _close(_py(T.anchor_propagate(case['vid'], copy.deepcopy(track_proto), case['det'], 2)), g['anchor_propagate'])
    assert calls == [(n_tub, len(anchor_frames))]            # one call; a frame shared by two anchors travels once
    # only the anchor frames' detections are read
    short = copy.deepcopy(case['det'])
    for d in short['detections']:
        if d['frame'] not in anchor_frames:
            d['scores'] = d['scores'][:1]
    _close(_py(T.anchor_propagate(case['vid'], copy.deepcopy(track_proto), short, 2)), g['anchor_propagate'])
    assert len(calls) == 2
    # a tubelet needs exactly one anchor box, an anchor frame at least one detection: nothing reaches the device otherwise
    two = copy.deepcopy(track_proto)
    two['tracks'][0][0]['anchor'] = two['tracks'][0][1]['anchor'] = 0
    with pytest.raises(AssertionError):
        T.anchor_propagate(case['vid'], two, case['det'], 2)
    empty = {'video': case['det']['video'], 'detections': [d for d in case['det']['detections'] if d['frame'] not in anchor_frames]}
    with pytest.raises((IndexError, ValueError)):
        T.anchor_propagate(case['vid'], copy.deepcopy(track_proto), empty, 2)
    assert len(calls) == 2
    # no tubelets: no call, an empty result
    none = T.anchor_propagate(case['vid'], {'video': track_proto['video'], 'method': 'x', 'tracks': []}, case['det'], 2)
    assert none['tubelets'] == [] and len(calls) == 2


def test_argument_checks_without_a_device():
    import torch
    from vdetlib_amd import ops
    boxes = torch.zeros((5, 8, 4))
    frames = torch.zeros((2, 3), dtype=torch.int32)
    ab = torch.zeros((2, 3, 4))
    for fn in (lambda: ops.track_from_anchors(boxes.double(), frames, ab),
               lambda: ops.track_from_anchors(boxes, frames.long(), ab),
               lambda: ops.track_from_anchors(boxes, frames, ab.double()),
               lambda: ops.track_from_anchors(boxes, frames, ab, torch.zeros((2, 3), dtype=torch.float64)),
               lambda: ops.track_from_anchors(boxes[:, :0], frames, ab),
               lambda: ops.track_from_anchors(boxes[..., :3], frames, ab),
               lambda: ops.track_from_anchors(boxes, frames, ab[:, :2]),
               lambda: ops.track_from_anchors(boxes, frames, ab, torch.zeros((2, 2))),
               lambda: ops.track_from_anchors(boxes, frames, ab)):                    # host tensors: there is no CPU path
        with pytest.raises(ValueError):
            fn()
    tracks = torch.zeros((2, 3, 5, 5))
    nt = torch.zeros((2,), dtype=torch.int32)
    an = torch.zeros((2, 3, 3))
    scores = torch.zeros((5, 8, 2))
    for fn in (lambda: ops.anchor_propagate_tracks(tracks.double(), nt, an, boxes, scores),
               lambda: ops.anchor_propagate_tracks(tracks, nt.long(), an, boxes, scores),
               lambda: ops.anchor_propagate_tracks(tracks[..., :4], nt, an, boxes, scores),
               lambda: ops.anchor_propagate_tracks(tracks, nt, an, boxes[:4], scores),
               lambda: ops.anchor_propagate_tracks(tracks, nt, an, boxes, scores[..., :1]),
               lambda: ops.anchor_propagate_tracks(tracks, nt[:1], an, boxes, scores),
               lambda: ops.anchor_propagate_tracks(tracks, nt, an[:, :2], boxes, scores),
               lambda: ops.anchor_propagate_tracks(tracks, nt, an, boxes, scores)):
        with pytest.raises(ValueError):
            fn()
