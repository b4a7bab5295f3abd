"""Tubelet re-scoring of the reference's vdet/tubelet_cls.py: spatial max-pooling of detection
scores onto tubelet boxes, gap completion, temporal max-pooling, interpolation, the channel
assembly of the temporal-convolution scorer, and the CNN scorers ``rcnn_scoring`` /
``rcnn_sampling_scoring`` with ``sampling_boxes`` (:102-194).  Dict plumbing in python, every numeric
core on the GPU (vdetlib_amd.hot / vdetlib_amd.ops -> include/vdet_hip.h).

The CNN scorers: the net is the caller's (any pycaffe-like object, ``image_det.googlenet_features``);
its windows are warped on the GPU (``ops.rcnn_patches``) and everything after it -- the class column
of the SVM, the max over a box's sampled windows, the winning box -- is ``ops.svm_head`` (DESIGN.md
section 10k).

``fast_rcnn_cls`` (:53-76) follows the reference's frame loop around ``image_det.im_detect``: backbone and head are
the caller's torch callables, the pooling between them is ``ops.roi_pool``.

Out of scope: googlenet_cls (:79-100, the fixed-point uint8 crop of ``googlenet_det``).
``rcnn_sampling_dets_scoring`` (:196-260) has no dict-level form; its half after the CNN is
``ops.rescore_tubelets(floor=...)`` on the scores ``ops.svm_head`` writes.
"""
import copy
from collections import defaultdict

import numpy as np

from ..utils.protocol import bbox_hash, frame_path_at, track_box_at_frame, tubelet_box_at_frame, tubelets_overlap, \
    tubelets_proto_from_tracks_proto
from ..utils.common import imread, svm_from_rcnn_model
from ..utils.log import logger as logging
from .dataset import imagenet_vdet_classes, index_vdet_to_det
from .image_det import googlenet_features, im_detect
from .. import hot


# per-box fields that become channel sequences of the temporal-convolution scorer: blob name -> box key
_TCN_BOX_FIELDS = (('det_scores', 'det_score'), ('track_scores', 'track_score'), ('gt_overlaps', 'gt_overlap'))
_TCN_OPTIONAL_FIELDS = (('all_scores', 'all_score'), ('feats', 'feat'))       # memory-heavy: read only when the net has the blob


def _tcn_channels(tubelet, blob_names):
    """Everything the reference offers a net per tubelet (:19-37), keyed by blob name: the per-box fields, the anchor offset
    normalised by the tubelet length (float division) and its magnitude, the 0 / 1 labels (gt overlap >= 0.5), and the
    tubelet-level entries `length`, `gt`, `mean_iou` (a net with blobs of those names receives them too)."""
    boxes = tubelet['boxes']
    length = len(boxes)
    ch = {name: [box[key] for box in boxes] for name, key in _TCN_BOX_FIELDS}
    rel = np.asarray([box['anchor'] for box in boxes], dtype=np.float64) / length
    ch['anchors'] = rel
    ch['abs_anchors'] = np.abs(rel)
    ch['labels'] = (np.asarray(ch['gt_overlaps'], dtype=np.float64) >= 0.5).astype(np.int64)
    ch['length'], ch['gt'] = length, tubelet['gt']
    ch['mean_iou'] = np.mean([ch['gt_overlaps']])
    for name, key in _TCN_OPTIONAL_FIELDS:
        if name in blob_names:
            ch[name] = [box[key] for box in boxes]
    return ch, length


def score_conv_cls(score_proto, net):
    """Reference :15-51.  Contract: for every tubelet, each blob of ``net`` whose name is one of the channel names above is
    reshaped to (1, its channel count, 1, L) and filled with the float32 sequence; ``net.forward()['probs'][:, 1, :]``
    becomes ``box['conv_score']`` (python float) of the tubelet's boxes, in place; the returned proto is a shallow copy.
    ``net`` is any object with ``.blobs`` (name -> object with ``.shape``, ``.reshape(*dims)``, ``.data``) and
    ``.forward()`` -- pycaffe's interface; ``vdetlib_amd.vdet.tcn.TCNNet`` is a gfx950 implementation of it.
    A net with a wide blob (``all_scores`` / ``feats``, per-box lists) raises ValueError here exactly as in the reference:
    the [L, ch] array of the boxes' rows does not broadcast into the (1, ch, 1, L) blob.  ``score_conv_cls_batched`` and
    ``ops.tcn_tracks(wide=...)`` give such nets their intended input."""
    out = copy.copy(score_proto)
    print("{}: {} tubelet(s).".format(score_proto['video'], len(out['tubelets'])))
    blob_names = set(net.blobs.keys())
    for tubelet in out['tubelets']:
        channels, length = _tcn_channels(tubelet, blob_names)
        for name in blob_names.intersection(channels):
            blob = net.blobs[name]
            blob.reshape(1, blob.shape[1], 1, length)
            blob.data[...] = np.asarray(channels[name], dtype='float32')
        probs = np.asarray(net.forward()['probs'][:, 1, :]).ravel()
        for box, p in zip(tubelet['boxes'], probs):
            box['conv_score'] = float(p)
    return out


def score_conv_cls_batched(score_proto, net):
    """``score_conv_cls`` for a ``vdetlib_amd.vdet.tcn.TCNNet`` with ALL tubelets of the proto in one launch
    (``TCNNet.forward_series``): same channel assembly, same ``conv_score`` values bit for bit, same return value.  The
    net's blobs are not touched (``score_conv_cls`` itself keeps the per-tubelet pycaffe contract).

    Wide blobs (``all_scores``, ``feats``: per-box lists, :35-41) are laid out [ch, L] by TRANSPOSING the [L, ch] array of
    the boxes' rows: channel q at position j is entry q of box j.  ``score_conv_cls`` keeps the reference's behaviour for
    them, which is to raise: it assigns the [L, ch] array to the (1, ch, 1, L) blob, and numpy cannot broadcast that."""
    from .tcn import TCNNet
    if not isinstance(net, TCNNet):
        raise TypeError("score_conv_cls_batched needs a vdetlib_amd.vdet.tcn.TCNNet (any pycaffe-like net: score_conv_cls)")
    out = copy.copy(score_proto)
    print("{}: {} tubelet(s).".format(score_proto['video'], len(out['tubelets'])))
    blob_names = set(net.blobs.keys())
    series = []
    for tubelet in out['tubelets']:
        channels, length = _tcn_channels(tubelet, blob_names)
        rows = []
        for name, ch in net.inputs:
            if name not in channels:
                raise ValueError("the net reads a blob %r that score_conv_cls does not assemble" % name)
            arr = np.asarray(channels[name], dtype='float32')
            if arr.ndim == 2:       # a per-box field whose entries are lists ([L, ch]): channel q at position j = entry q of box j
                if arr.shape != (length, ch):
                    raise ValueError("blob %r has %d channels; its boxes carry rows of %d" % (name, ch, arr.shape[1]))
                arr = arr.T
            rows.append(np.ascontiguousarray(arr).reshape(ch, length))
        series.append(np.concatenate(rows, 0))
    for tubelet, probs in zip(out['tubelets'], net.forward_series(series)):
        for box, p in zip(tubelet['boxes'], probs):
            box['conv_score'] = float(p)
    return out


def fast_rcnn_cls(video_proto, track_proto, net, class_idx, images=None):
    """:53-76 -- per frame, the boxes of the tracks that have one there go through ``im_detect`` (one backbone pass, every box
    pooled on the device) and each track gets {frame, bbox: the decoded box row (all classes, as the reference's
    ``list(box)``), score: column ``class_idx``, hash}; a frame where a track has no box adds nothing to it.  ``net``: see
    ``image_det.im_detect``.  ``images``: {frame id: uint8 [H,W,3]} instead of reading the frames' files.  A frame without
    any box is skipped (the reference's ``im_detect`` has nothing to reshape there)."""
    new_tracks = [[] for _ in track_proto['tracks']]
    for frame in video_proto['frames']:
        frame_id = frame['frame']
        img = images[frame_id] if images is not None else imread(frame_path_at(video_proto, frame_id))
        boxes = [track_box_at_frame(tracklet, frame_id) for tracklet in track_proto['tracks']]
        valid_boxes = np.asarray([box for box in boxes if box is not None])
        valid_index = [i for i in range(len(boxes)) if boxes[i] is not None]
        if not valid_index:
            continue
        scores, pred_boxes = im_detect(net, img, valid_boxes)
        for score, box, track_id in zip(scores, pred_boxes, valid_index):
            new_tracks[track_id].append({"frame": frame_id, "bbox": list(box), "score": score[class_idx],
                                         "hash": bbox_hash(video_proto['video'], frame_id, box)})
    return new_tracks


def sampling_boxes(orig_box, num, ratio=0.05, return_orig=True):
    """:136-142, line for line: ``num`` boxes around ``orig_box``, every corner moved by a uniform draw of at most ``ratio``
    of the box's width / height (x2-x1, y2-y1) from numpy's GLOBAL generator."""
    h, w = orig_box[3] - orig_box[1], orig_box[2] - orig_box[0]
    offsets = np.random.uniform(-ratio, ratio, [num, 4]) * [w, h, w, h]
    if not return_orig:
        return orig_box + offsets
    else:
        return np.vstack((orig_box, orig_box + offsets))


def _frame_tubelet_boxes(tubelets_proto, frame_id):
    """The boxes of a frame as the reference's frame loop collects them (:111-114): (boxes [n,4], tubelet index of each)."""
    boxes = [tubelet_box_at_frame(tubelet, frame_id) for tubelet in tubelets_proto]
    valid_boxes = np.asarray([box for box in boxes if box is not None])
    valid_index = [i for i, box in enumerate(boxes) if box is not None]
    return valid_boxes, valid_index


def _svm_head_frame(features, svm_model, cache, class_idx, group, want_all):
    """One upload of a frame's features, then ``ops.svm_head``: per box the class score and the winning window (f64 numpy),
    the winners' feature rows, and their scores of ALL classes (``ops.svm_scores``) when asked for.  ``cache``: a dict of the
    calling scorer that keeps the model's device copy from frame to frame."""
    import torch
    from .. import _lib, ops
    _lib.get_context()        # no library or no GPU: RuntimeError
    features = np.asarray(features)
    if features.ndim == 4:
        features = np.squeeze(features, axis=(2, 3))
    W = np.asarray(svm_model['W'])
    if W.shape[1] != 200:
        raise RuntimeError("the SVM model must score the 200 DET classes")        # the reference's bare `raise` (:122-123)
    dev = torch.device('cuda', torch.cuda.current_device())
    model = cache.get('model')
    if model is None or model['W'].device != dev:
        model = {'W': torch.from_numpy(np.ascontiguousarray(W)).to(dev),
                 'B': torch.from_numpy(np.ascontiguousarray(np.asarray(svm_model['B']).reshape(-1))).to(dev),
                 'feat_norm_mean': svm_model['feat_norm_mean']}
        cache['model'] = model
    d_feat = torch.from_numpy(np.ascontiguousarray(features)).to(dev)
    cols = torch.tensor([index_vdet_to_det[class_idx] - 1], dtype=torch.int32, device=dev)
    out = ops.svm_head(d_feat, model, group=group, cols=cols)
    if int(out['nbad']):
        raise ValueError("a box without a window to score")
    arg = out['arg_flat'].cpu().numpy().astype(np.int64)
    rows = np.arange(len(arg)) * group + arg
    all_scores = None
    if want_all:
        all_scores = ops.svm_scores(d_feat[torch.from_numpy(rows).to(dev)], model).cpu().numpy()
    return out['score'].cpu().numpy(), arg, features[rows], all_scores


def rcnn_scoring(vid_proto, track_proto, net, class_idx, rcnn_model, save_feat=False, save_all_sc=False):
    """:102-134 -- every tubelet box of class ``class_idx`` gets ``det_score``: the R-CNN SVM score of its ``pool5`` features
    for the class (column ``index_vdet_to_det[class_idx] - 1`` of the 200).  ``save_feat`` / ``save_all_sc`` add ``feat`` and
    ``all_score`` (all 200 classes).  Per frame: ``googlenet_features`` (windows warped on the GPU, ``net`` the caller's), one
    upload of the features, ``ops.svm_head``."""
    svm_model = svm_from_rcnn_model(rcnn_model)
    tubelets_proto = tubelets_proto_from_tracks_proto(track_proto['tracks'], class_idx)
    cache = {}
    logging.info("Scoring {} for {}...".format(vid_proto['video'], imagenet_vdet_classes[class_idx]))
    for frame in vid_proto['frames']:
        frame_id = frame['frame']
        img = imread(frame_path_at(vid_proto, frame_id))
        valid_boxes, valid_index = _frame_tubelet_boxes(tubelets_proto, frame_id)
        logging.info("frame {}: {} boxes".format(frame_id, len(valid_index)))
        if len(valid_index) == 0:
            continue
        features = googlenet_features(img, valid_boxes, net, 'pool5')
        cls_scores, _, feats, all_scores = _svm_head_frame(features, svm_model, cache, class_idx, 1, save_all_sc)
        for k, tubelet_id in enumerate(valid_index):
            cur_box = [box for box in tubelets_proto[tubelet_id]['boxes'] if box['frame'] == frame_id]
            assert len(cur_box) == 1
            cur_box[0]['det_score'] = cls_scores[k]
            if save_feat:
                cur_box[0]['feat'] = feats[k].ravel().tolist()
            if save_all_sc:
                cur_box[0]['all_score'] = all_scores[k].ravel().tolist()
    return tubelets_proto


def rcnn_sampling_scoring(vid_proto, track_proto, net, class_idx, rcnn_model, samples_per_box=32, ratio=0.05,
                          save_feat=False, save_all_sc=False):
    """:144-194 -- ``rcnn_scoring`` over ``samples_per_box`` boxes sampled around every tubelet box (``sampling_boxes``, numpy's
    global generator, drawn in the reference's order) and the box itself: ``det_score`` is the best class score of the
    ``samples_per_box + 1`` windows and ``bbox`` becomes the winning window's box (the first one on ties, np.argmax);
    ``feat`` / ``all_score`` are the winner's.  The max, the argmax and the class column are one ``ops.svm_head`` call per
    frame."""
    svm_model = svm_from_rcnn_model(rcnn_model)
    tubelets_proto = tubelets_proto_from_tracks_proto(track_proto['tracks'], class_idx)
    cache = {}
    logging.info("Scoring {} for {}...".format(vid_proto['video'], imagenet_vdet_classes[class_idx]))
    for frame in vid_proto['frames']:
        frame_id = frame['frame']
        img = imread(frame_path_at(vid_proto, frame_id))
        valid_boxes, valid_index = _frame_tubelet_boxes(tubelets_proto, frame_id)
        logging.info("frame {}: {} boxes".format(frame_id, len(valid_index)))
        if len(valid_index) == 0:
            continue
        # sample nearby boxes to increase spatial robustness
        sampled_boxes = np.vstack([sampling_boxes(box, samples_per_box, ratio) for box in valid_boxes])
        features = googlenet_features(img, sampled_boxes, net, 'pool5')
        max_scores, max_idx, feats, all_scores = _svm_head_frame(features, svm_model, cache, class_idx, samples_per_box + 1,
                                                                 save_all_sc)
        sampled_boxes = sampled_boxes.reshape((len(valid_index), samples_per_box + 1, -1))
        boxes = sampled_boxes[range(len(valid_index)), max_idx, :]
        for k, tubelet_id in enumerate(valid_index):
            cur_box = [box for box in tubelets_proto[tubelet_id]['boxes'] if box['frame'] == frame_id]
            assert len(cur_box) == 1
            cur_box[0]['det_score'] = max_scores[k]
            cur_box[0]['bbox'] = boxes[k].tolist()
            if save_feat:
                cur_box[0]['feat'] = feats[k].ravel().tolist()
            if save_all_sc:
                cur_box[0]['all_score'] = all_scores[k].ravel().tolist()
    return tubelets_proto


def scoring_tracks(vid_proto, track_proto, annot_proto, sc_method, net, class_idx):
    """:263-273"""
    assert vid_proto['video'] == track_proto['video']
    tubelets_proto = sc_method(vid_proto, track_proto, net, class_idx)
    if annot_proto is not None:
        tubelets_proto = tubelets_overlap(tubelets_proto, annot_proto, class_idx)
    return {'video': vid_proto['video'], 'method': sc_method.__name__, 'tubelets': tubelets_proto}


def classify_tracks(video_proto, track_proto, cls_method, net, class_idx):
    """:276-282"""
    assert video_proto['video'] == track_proto['video']
    return {'video': video_proto['video'], 'method': cls_method.__name__,
            'tracks': cls_method(video_proto, track_proto, net, class_idx)}


def do_score_completion(score_proto):
    """:284-303 -- in place: runs of det_score <= -10 are filled (edge extension / linear
    interpolation).  IndexError, like the reference, for a tubelet with no valid score at all."""
    tubelets = score_proto['tubelets']
    series = [[box['det_score'] for box in tubelet['boxes']] for tubelet in tubelets]
    done = hot.series_completion(series)
    for tubelet, new in zip(tubelets, done):
        for box, old, v in zip(tubelet['boxes'], [b['det_score'] for b in tubelet['boxes']], new):
            if old <= -10:            # untouched entries keep their python object (int stays int)
                box['det_score'] = float(v)


def _spatial_max_pooling(vid_proto, tubelets_proto, frame_dets, overlap_thres):
    """Shared core of :316-347 / :504-532.  frame_dets: frame_id -> (det_boxes array, det_scores
    1-D array) for the frames that have detections."""
    frame_to_tubelets_idx = defaultdict(list)
    for i, tubelet in enumerate(tubelets_proto):
        for j, box in enumerate(tubelet['boxes']):
            frame_to_tubelets_idx[box['frame']].append((i, j))
    slots, det_boxes_list, det_scores_list = {}, [], []
    tub_boxes, tub_group, targets = [], [], []
    for frame in vid_proto['frames']:
        frame_id = frame['frame']
        if frame_id not in frame_dets:
            continue
        for i, j in frame_to_tubelets_idx[frame_id]:
            cur_box = tubelets_proto[i]['boxes'][j]
            if cur_box is None:
                continue
            if frame_id not in slots:
                slots[frame_id] = len(det_boxes_list)
                det_boxes_list.append(frame_dets[frame_id][0])
                det_scores_list.append(frame_dets[frame_id][1])
            tub_boxes.append(cur_box['bbox'])
            tub_group.append(slots[frame_id])
            targets.append((i, j, frame_id))
    idx, score = hot.spatial_maxpool(tub_boxes, tub_group, det_boxes_list, det_scores_list, overlap_thres)
    for (i, j, frame_id), k, s in zip(targets, idx, score):
        cur_box = tubelets_proto[i]['boxes'][j]
        if k >= 0:
            cur_box['det_score'] = float(s)
            cur_box['bbox'] = frame_dets[frame_id][0][int(k)].tolist()
        else:
            print("Warning: Tubelet {} has no overlapping dets (IOU > {}).".format(i, overlap_thres))
            cur_box['det_score'] = float(-1e5)


def dets_spatial_max_pooling(vid_proto, track_proto, det_proto, class_idx, overlap_thres=0.7):
    """:305-350 -- detections as protocol dicts; the class score is read BY POSITION
    ``det['scores'][class_idx - 1]['score']`` (:329)."""
    assert vid_proto['video'] == track_proto['video']
    score_proto = {'video': vid_proto['video'],
                   'method': "spatial_max_pooling_IOU_{}".format(overlap_thres)}
    tubelets_proto = tubelets_proto_from_tracks_proto(track_proto['tracks'], class_idx)
    logging.info("Sampling dets in {} for {}...".format(vid_proto['video'], imagenet_vdet_classes[class_idx]))
    frame_to_det_idx = defaultdict(list)
    for i, det in enumerate(det_proto['detections']):
        frame_to_det_idx[det['frame']].append(i)
    frame_dets = {}
    for frame_id, det_idx in frame_to_det_idx.items():
        frame_dets[frame_id] = (
            np.asarray([det_proto['detections'][i]['bbox'] for i in det_idx]),
            np.asarray([det_proto['detections'][i]['scores'][class_idx - 1]['score'] for i in det_idx]))
    _spatial_max_pooling(vid_proto, tubelets_proto, frame_dets, overlap_thres)
    score_proto['tubelets'] = tubelets_proto
    do_score_completion(score_proto)
    return score_proto


class _ClassDetsByFrame(object):
    """frame -> (bboxes [n,4], class scores [n]) of a det_proto, detections in protocol order.  Only the frames that are
    asked for are touched (and remembered): a det_proto whose detections of OTHER frames carry short score lists must not
    fail here -- the reference only reads the anchor frames' detections (:366-374)."""

    def __init__(self, det_proto, class_idx):
        self._dets = det_proto['detections']
        self._cls = class_idx - 1
        self._by_frame = defaultdict(list)
        for i, det in enumerate(self._dets):
            self._by_frame[det['frame']].append(i)
        self._memo = {}

    def __call__(self, frame):
        got = self._memo.get(frame)
        if got is None:
            idx = self._by_frame.get(frame, ())
            got = self._memo[frame] = (np.asarray([self._dets[i]['bbox'] for i in idx]),
                                       np.asarray([self._dets[i]['scores'][self._cls]['score'] for i in idx]))
        return got


def anchor_propagate(vid_proto, track_proto, det_proto, class_idx):
    """Contract of :353-383: a tubelet's anchor is its one box with ``anchor == 0``; the detection of that frame that
    overlaps the anchor box most (first one on ties) lends its ``class_idx`` score to EVERY box of the tubelet."""
    assert vid_proto['video'] == track_proto['video']
    tubelets_proto = tubelets_proto_from_tracks_proto(track_proto['tracks'], class_idx)
    logging.info("Propagating anchor scores in {} for {}...".format(vid_proto['video'],
                                                                     imagenet_vdet_classes[class_idx]))
    dets = _ClassDetsByFrame(det_proto, class_idx)
    # overlap + arg-max of ALL tubelets of the call in one device call: the anchor frames' detections, each frame once
    slots, det_boxes_list, anchor_boxes, anchor_group, det_scores_of = {}, [], [], [], []
    for tubelet in tubelets_proto:
        anchors = [box for box in tubelet['boxes'] if box['anchor'] == 0]
        assert len(anchors) == 1
        frame_id = anchors[0]['frame']
        det_boxes, det_scores = dets(frame_id)
        abox = np.asarray([anchors[0]['bbox']]).astype('float')
        det_boxes = np.asarray(det_boxes).astype('float')
        if abox.ndim != 2 or det_boxes.ndim != 2 or abox.shape[1] < 4 or det_boxes.shape[1] < 4:
            raise IndexError("boxes must be [n,4]")              # what iou([bbox], det_boxes) raises
        if det_boxes.shape[0] == 0:
            raise ValueError("attempt to get argmax of an empty sequence")
        if frame_id not in slots:
            slots[frame_id] = len(det_boxes_list)
            det_boxes_list.append(det_boxes[:, :4])
        anchor_boxes.append(abox[0, :4])
        anchor_group.append(slots[frame_id])
        det_scores_of.append(det_scores)
    best = hot.anchor_argmax(anchor_boxes, anchor_group, det_boxes_list) if anchor_boxes else []
    for tubelet, det_scores, k in zip(tubelets_proto, det_scores_of, best):
        for box in tubelet['boxes']:
            box['det_score'] = det_scores[int(k)]
    return {'video': vid_proto['video'], 'method': "anchor_propagate", 'tubelets': tubelets_proto}


def score_proto_temporal_maxpool(score_proto, window_size):
    """:386-414 -- centred sliding max of det_score per tubelet (out-of-range = -1e5), written back
    into the SAME box dicts; the returned proto is a shallow copy whose method gets the suffix
    '_temporal_maxpool_{w}'.  Raises on an even window and on ground-truth tubelets (after having
    processed the tubelets before it, like the reference)."""
    if window_size == 1:
        return score_proto
    if window_size % 2 != 1:
        raise ValueError('Window size must be odd!')
    new_score_proto = copy.copy(score_proto)
    new_score_proto['method'] += '_temporal_maxpool_{}'.format(window_size)
    tubelets = new_score_proto['tubelets']
    n_ok = len(tubelets)
    for t, tubelet in enumerate(tubelets):
        if tubelet['gt'] == 1:
            n_ok = t
            break
    series = [[box['det_score'] for box in tubelet['boxes']] for tubelet in tubelets[:n_ok]]
    pooled = hot.series_maxpool(series, window_size, -1e+5)
    for tubelet, new in zip(tubelets[:n_ok], pooled):
        for box, v in zip(tubelet['boxes'], new):
            box['det_score'] = float(v)
    if n_ok < len(tubelets):
        raise ValueError('Dangerous: Score file contains gt tracks!')
    return new_score_proto


def extrap1d(interpolator):
    """:416-428 -- point-wise linear extrapolation wrapper around a scipy interp1d-like object
    (kept for API compatibility; score_proto_interpolation does not need it here)."""
    xs, ys = interpolator.x, interpolator.y

    def pointwise(x):
        if x < xs[0]:
            return ys[0] + (x - xs[0]) * (ys[1] - ys[0]) / (xs[1] - xs[0])
        elif x > xs[-1]:
            return ys[-1] + (x - xs[-1]) * (ys[-1] - ys[-2]) / (xs[-1] - xs[-2])
        return interpolator(x)
    return pointwise


def score_proto_interpolation(score_proto, vid_proto):
    """:430-490 -- per tubelet with >= 2 boxes: linear interpolation of x1,y1,x2,y2,det_score,
    anchor to every integer frame of [min, max] (min 2 -> 1 and max F-1 -> F by one-step
    extrapolation, :472-475).  Output boxes carry only frame, det_score, anchor, bbox."""
    new_score_proto = {'video': score_proto['video'], 'method': score_proto['method'] + '_interpolation'}
    max_frames = len(vid_proto['frames'])
    out = []
    jobs = []
    for tubelet in score_proto['tubelets']:
        if tubelet['gt'] == 1:
            raise ValueError('Dangerous: Score file contains gt tracks!')
        if len(tubelet['boxes']) < 2:
            out.append(copy.copy(tubelet))
            continue
        truth_idx = [box['frame'] for box in tubelet['boxes']]
        fields = np.asarray([[box['bbox'][0], box['bbox'][1], box['bbox'][2], box['bbox'][3],
                              box['det_score'], box['anchor']] for box in tubelet['boxes']], dtype=np.float64)
        order = np.argsort(np.asarray(truth_idx), kind='stable')      # interp1d sorts its knots
        min_idx, max_idx = min(truth_idx), max(truth_idx)
        if min_idx == 2:
            min_idx = 1
        if max_idx == max_frames - 1:
            max_idx = max_frames
        new_tubelet = {}
        for key in ['gt', 'class', 'class_index']:
            new_tubelet[key] = tubelet[key]
        new_tubelet['boxes'] = []
        out.append(new_tubelet)
        jobs.append((new_tubelet, np.asarray(truth_idx, dtype=np.float64)[order], fields[order],
                     list(range(min_idx, max_idx + 1))))
    dense = hot.series_interp([j[1] for j in jobs], [j[2] for j in jobs], [j[3] for j in jobs])
    for (new_tubelet, _, _, frames), vals in zip(jobs, dense):
        for dense_idx, v in zip(frames, vals):
            new_tubelet['boxes'].append({'frame': dense_idx, 'det_score': float(v[4]), 'anchor': float(v[5]),
                                         'bbox': [float(v[0]), float(v[1]), float(v[2]), float(v[3])]})
    new_score_proto['tubelets'] = out
    return new_score_proto


def raw_dets_spatial_max_pooling(vid_proto, track_proto, frame_to_det, class_idx, overlap_thres=0.7):
    """:493-535 -- detections as per-frame arrays {frame_id: (boxes [B,4], zs [B,C])}; class
    column zs[:, class_idx - 1] (:514).  Frames missing from frame_to_det or without boxes are
    skipped (:511-513)."""
    assert vid_proto['video'] == track_proto['video']
    score_proto = {'video': vid_proto['video'],
                   'method': "spatial_max_pooling_IOU_{}".format(overlap_thres)}
    tubelets_proto = tubelets_proto_from_tracks_proto(track_proto['tracks'], class_idx)
    logging.info("Sampling dets in {} for {}...".format(vid_proto['video'], imagenet_vdet_classes[class_idx]))
    frame_dets = {}
    for frame_id, (det_boxes, det_scores) in frame_to_det.items():
        if np.asarray(det_boxes).size == 0:
            continue
        frame_dets[frame_id] = (np.asarray(det_boxes), np.asarray(det_scores)[:, class_idx - 1].ravel())
    _spatial_max_pooling(vid_proto, tubelets_proto, frame_dets, overlap_thres)
    score_proto['tubelets'] = tubelets_proto
    do_score_completion(score_proto)
    return score_proto
