"""Region proposals (the API slot of the reference's vdet/proposal.py).  The reference's ``vid_proposals`` (:33-43) calls MATLAB
selective search, an external engine outside this build; here the proposals come from a region proposal network of the
caller's: any torch backbone and RPN head around ``ops.rpn_proposals``, the proposal layer on the
device.  ``get_windows`` (:8-30, the MATLAB call) is out of scope.

The ``net`` is ``image_det.im_detect``'s with three additions:
    net.rpn(feat) -> (scores [1,A,Hf,Wf] f32, deltas [1,4A,Hf,Wf] f32)   the foreground scores (logits or probabilities) and
                                                                          the anchor deltas of one frame's feature map
    net.anchors      float64 [A,4]  (``ops.generate_anchors``)
    net.feat_stride  the backbone's stride in pixels of the scaled image
Backbone and RPN head run on one frame at a time -- the shapes ``im_detect`` gives them --; the proposal layer takes the frames
of a chunk in one call."""
import numpy as np

from ..utils.common import imread
from ..utils.protocol import bbox_hash, boxes_proto_from_boxes, frame_path_at


def rpn_chunk(net, ims, pre_nms_top_n=6000, post_nms_top_n=300, nms_thresh=0.7, min_size=16, dw_max=None, return_candidates=False):
    """The frames ``ims`` (uint8 [H,W,3], one size) through ``net.prepare``, ``net.backbone``, ``net.rpn`` and
    ``ops.rpn_proposals``, which runs in the SCALED image's coordinates with ``min_size * im_scale``.  Returns (the frames'
    feature maps, ``ops.rpn_proposals``' dict -- rois in scaled coordinates, on the device --, im_scale)."""
    import torch
    from .. import ops
    feats, scores, deltas, scale, size = [], [], [], None, None
    with torch.no_grad():
        for im in ims:
            x, im_scale = net.prepare(im)
            if scale is None:
                scale, size = float(im_scale), tuple(x.shape[2:])
            elif float(im_scale) != scale or tuple(x.shape[2:]) != size:
                raise ValueError("rpn_chunk: the frames of a chunk must share one size and one scale")
            feat = net.backbone(x).contiguous()
            s, d = net.rpn(feat)
            feats.append(feat); scores.append(s.detach().float()); deltas.append(d.detach().float())
        out = ops.rpn_proposals(torch.cat(scores), torch.cat(deltas), net.anchors, size, stride=net.feat_stride,
                                pre_nms_top_n=pre_nms_top_n, post_nms_top_n=post_nms_top_n, nms_thresh=nms_thresh,
                                min_size=min_size * scale, dw_max=dw_max, return_candidates=return_candidates)
    return feats, out, scale


def rpn_vid_proposals(net, vid_proto, pre_nms_top_n=6000, post_nms_top_n=300, nms_thresh=0.7, min_size=16, dw_max=None, chunk=8,
                      images=None, integer_boxes=True):
    """The reference's ``vid_proposals`` with a region proposal network instead of selective search: a box_proto
    ``{'video', 'boxes': [{'frame', 'bbox', 'hash'}]}``, every frame's proposals in descending score order, in the ORIGINAL
    image's coordinates (the proposal layer's f32 boxes divided by ``im_scale`` in float64).

    ``integer_boxes`` (default): the list goes through ``boxes_proto_from_boxes`` as the reference's does, which truncates the
    coordinates to int.  False keeps the float64 coordinates (same keys, the hash over the same un-truncated values):
    ``video_det.fast_rcnn_det_vid_device`` fed that box_proto sees the boxes ``faster_rcnn_det_vid_device`` pools.
    ``images``: {frame id: uint8 [H,W,3]} instead of reading the frames' files."""
    from .. import _lib
    _lib.get_context()        # no library or no GPU: RuntimeError
    frames = vid_proto['frames']
    chunk = max(int(chunk), 1)
    frame_idx, boxes_list = [], []
    for i0 in range(0, len(frames), chunk):
        part = frames[i0:i0 + chunk]
        ims = [images[fr['frame']] if images is not None else imread(frame_path_at(vid_proto, fr['frame'])) for fr in part]
        _, out, im_scale = rpn_chunk(net, ims, pre_nms_top_n, post_nms_top_n, nms_thresh, min_size, dw_max)
        rois = (out['rois'].double() / im_scale).cpu().numpy()
        count = out['count'].cpu().numpy()
        for k, fr in enumerate(part):
            frame_idx.append(fr['frame'])
            boxes_list.append(rois[k, :count[k]])
    video = vid_proto['video']
    if integer_boxes:
        boxes = boxes_proto_from_boxes(frame_idx, boxes_list, video)
    else:
        boxes = [{'frame': int(f), 'bbox': [float(v) for v in bb], 'hash': bbox_hash(video, f, bb)}
                 for f, bbs in zip(frame_idx, boxes_list) for bb in bbs]
    return {'video': video, 'boxes': boxes}


def vid_proposals(vid_proto, method='selective_search'):
    """Reference :33-43 runs MATLAB selective search, an external engine outside this build: use ``rpn_vid_proposals``."""
    raise RuntimeError("selective search is an external engine (MATLAB, reference vdet/proposal.py:8-30); "
                       "rpn_vid_proposals(net, vid_proto) makes the proposals with a region proposal network on the device")
