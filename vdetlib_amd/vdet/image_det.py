"""Still-image NMS wrapper (:117-123), the SVM scorer (:109-114) and the R-CNN feature loop of the reference's
vdet/image_det.py: ``googlenet_features`` / ``googlenet_rcnn`` (:56-106) warp their windows on the GPU (``ops.rcnn_patches``,
DESIGN.md section 10j) and drive any pycaffe-like ``net`` through the reference's blob protocol; the nets themselves are the
caller's.  ``fast_rcnn_det`` (:22-33) and the ``im_detect`` it calls run the Fast R-CNN route: any torch backbone and head of
the caller's around ``ops.roi_pool``, the box decode on the host in numpy float64
(``video_det.fast_rcnn_det_vid_device`` keeps the head's output on the device: section 10z).
Out of scope: ``simple_crop`` / ``googlenet_det`` (:12-53, a fixed-point uint8 resize)."""
import numpy as np

from ..utils.cython_nms import nms
from ..utils.log import logger as logging


def apply_image_nms(boxes, scores, thres=0.3):
    """boxes [N,4], scores [N] (any float dtype) -> keep list, descending score (:117-123)."""
    box_score = np.asarray(np.r_['-1', boxes, np.reshape(scores, (-1, 1))], dtype='float32')
    logging.info("Applying nms to image.")
    keep = nms(box_score, thres)
    logging.info("{} / {} boxes kept.".format(len(keep), len(boxes)))
    return keep


def googlenet_rcnn(img, boxes, net):
    """:56-57."""
    return googlenet_features(img, boxes, net, 'cls_score')


def googlenet_features(img, boxes, net, blob_name):
    """:75-106: the 224-pixel 'warp' windows of ``boxes`` (padding 16, minus the BGR mean, channel-major float32) through
    ``net`` in slices of 128, ``net.blobs[blob_name].data`` of every slice concatenated.  img uint8 [H,W,3] is uploaded once;
    every slice is one device call (``ops.rcnn_patches``).  ``net``: anything with pycaffe's blob protocol --
    ``blobs['data'].reshape(*shape)``, ``blobs['data'].data[...] = patches``, ``forward()``, ``blobs[blob_name].data``.
    ValueError for a box whose window is empty (the reference raises inside cv2.resize).  RuntimeError without a GPU."""
    import torch
    from .. import _lib, ops
    _lib.get_context()        # no library or no GPU: RuntimeError
    size = 224
    mean_values = np.asarray([103.939, 116.779, 123.68])
    batch_size = 128
    img = np.ascontiguousarray(img)
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3:
        raise ValueError("img must be uint8 [H,W,3]")
    boxes = np.asarray(boxes, dtype=np.float64).reshape(-1, 4)
    dev = torch.device('cuda', torch.cuda.current_device())
    d_img = torch.from_numpy(img).to(dev)[None]
    d_boxes = torch.from_numpy(np.ascontiguousarray(boxes)).to(dev)
    features = None
    for b0 in range(0, max(len(boxes), 1), batch_size):
        out = ops.rcnn_patches(d_img, d_boxes[b0:b0 + batch_size], crop_size=size, padding=16, mean=mean_values, mode='warp')
        bad = (out['ok'] == 0).nonzero()
        if bad.numel():
            raise ValueError("googlenet_features: the window of box %d is empty (the reference raises inside cv2.resize)"
                             % (b0 + int(bad[0])))
        patches = out['patches'].cpu().numpy()
        net.blobs['data'].reshape(*(patches.shape))
        net.blobs['data'].data[...] = patches
        net.forward()
        cur_feat = net.blobs[blob_name].data
        if features is None:
            features = np.copy(cur_feat)
        else:
            try:
                features = np.r_[features, cur_feat]
            except ValueError as e:
                logging.error("Unable to concatenate features.")
                raise e
    return np.asarray(features)


def bbox_transform_inv(boxes, deltas):
    """The box decode of Fast R-CNN's ``im_detect``, restated (the public code was not at hand): boxes [N,4], deltas [N,4*Cn]
    -> float64 [N,4*Cn].  Per box ``w = x2 - x1 + 1e-14``, ``ctr = x1 + 0.5*w``; per class ``pred_ctr = d*w + ctr``,
    ``pred_w = exp(dw)*w``, corners ``pred_ctr -/+ 0.5*pred_w``; y alike.  numpy float64 on the host, as the reference does."""
    boxes = np.asarray(boxes, dtype=np.float64).reshape(-1, 4)
    deltas = np.asarray(deltas, dtype=np.float64)
    pred = np.zeros(deltas.shape, dtype=np.float64)
    if len(boxes) == 0:
        return pred
    w = boxes[:, 2] - boxes[:, 0] + 1e-14
    h = boxes[:, 3] - boxes[:, 1] + 1e-14
    cx, cy = boxes[:, 0] + 0.5 * w, boxes[:, 1] + 0.5 * h
    pcx = deltas[:, 0::4] * w[:, None] + cx[:, None]
    pcy = deltas[:, 1::4] * h[:, None] + cy[:, None]
    pw = np.exp(deltas[:, 2::4]) * w[:, None]
    ph = np.exp(deltas[:, 3::4]) * h[:, None]
    pred[:, 0::4] = pcx - 0.5 * pw
    pred[:, 1::4] = pcy - 0.5 * ph
    pred[:, 2::4] = pcx + 0.5 * pw
    pred[:, 3::4] = pcy + 0.5 * ph
    return pred


def clip_boxes(boxes, im_shape):
    """x to [0, W-1], y to [0, H-1] (im_shape = (H, W, ...)) -> a new array."""
    boxes = np.array(boxes, dtype=np.float64)
    boxes[:, 0::2] = np.maximum(np.minimum(boxes[:, 0::2], im_shape[1] - 1), 0)
    boxes[:, 1::2] = np.maximum(np.minimum(boxes[:, 1::2], im_shape[0] - 1), 0)
    return boxes


def im_detect(net, img, boxes):
    """``fast_rcnn.test.im_detect``'s shape: (scores [N,Cn], pred_boxes [N,4*Cn]) as numpy, for the boxes [N,4] of ``img``
    [H,W,3] (image coordinates, as they are).  A valid ``det_fun`` of ``video_det.fast_rcnn_det_vid``.

    ``net`` is any object with ``prepare(img) -> (tensor [1,3,H',W'] on the GPU, im_scale)`` -- the mean subtraction and the
    image resize are the caller's, as the net is -- ``backbone(x) -> [1,K,Hf,Wf]``, ``head(pooled) -> (scores, deltas)``,
    ``spatial_scale`` and ``pooled``; optionally ``roi_mode`` ('max'), ``sampling`` and ``aligned`` (``ops.roi_pool``).  The
    backbone runs once, every box is pooled out of its map on the device (``box_scale = im_scale``), the decode
    (``bbox_transform_inv``, ``clip_boxes``) is numpy float64 on the host.  The reference de-duplicates RoIs that fall on the
    same cells first; that changes no result and is left out.  ValueError for a box that is not finite."""
    import torch
    from .. import _lib, ops
    _lib.get_context()        # no library or no GPU: RuntimeError
    boxes = np.ascontiguousarray(np.asarray(boxes, dtype=np.float64).reshape(-1, 4))
    with torch.no_grad():
        x, im_scale = net.prepare(img)
        feat = net.backbone(x)
        out = ops.roi_pool(feat.contiguous(), torch.from_numpy(boxes).to(feat.device), spatial_scale=net.spatial_scale,
                           pooled=net.pooled, box_scale=im_scale, mode=getattr(net, 'roi_mode', 'max'),
                           sampling=getattr(net, 'sampling', 2), aligned=getattr(net, 'aligned', False))
        bad = (out['ok'] == 0).nonzero()
        if bad.numel():
            raise ValueError("im_detect: box %d is not finite (or beyond 2^24 cells)" % int(bad[0]))
        scores, deltas = net.head(out['pooled'])
    scores, deltas = scores.detach().cpu().numpy(), deltas.detach().cpu().numpy()
    return scores, clip_boxes(bbox_transform_inv(boxes, deltas), np.shape(img))


def fast_rcnn_det(img, boxes, net):
    """:22-33 -- the scores of ``im_detect`` (there is no Caffe log level to lower here)."""
    scores, _ = im_detect(net, img, np.array(boxes))
    return scores


def svm_scores(features, svm_model):
    """reference vdet/image_det.py:109-114: ``features * (20 / feat_norm_mean) @ W + B``, the path's one dense
    contraction ([n, 1024] x [1024, 200]), on the GPU as a hand-written MFMA kernel
    (``vdet_svm_scores_f64`` / ``_f32``: v_mfma_f64_16x16x4_f64 / v_mfma_f32_16x16x4_f32) in numpy's result
    dtype -- float64 for the reference's .mat models, float32 when features and W both are.  The scaling, the
    squeeze of [n,k,1,1] features and the broadcast of B are the reference's; no CPU fallback."""
    from .. import _lib
    features = np.asarray(features)
    if features.ndim == 4:
        features = np.squeeze(features, axis=(2, 3))
    features = np.asarray(features) * (20. / svm_model['feat_norm_mean'])
    W = np.asarray(svm_model['W'])
    B = np.asarray(svm_model['B'])
    if features.ndim != 2 or W.ndim != 2 or features.shape[1] != W.shape[0]:
        raise ValueError("shapes %s and %s not aligned" % (features.shape, W.shape))
    # the product is computed in the dtype numpy's dot would use (features, W); B joins afterwards exactly as
    # ``+ B`` would (a float64 B on float32 operands promotes the SUM, not the contraction)
    dt = np.result_type(features.dtype, W.dtype)
    dt = np.dtype(np.float32) if dt == np.float32 else np.dtype(np.float64)
    a = np.ascontiguousarray(features, dtype=dt)
    w = np.ascontiguousarray(W, dtype=dt)
    n, k = a.shape
    m = w.shape[1]
    # the bias is fused only when it is a per-COLUMN row ([m] / [1, m]) of the product's dtype; anything else -- a
    # column-shaped [m, 1] B (numpy broadcasts it per row when n == m and raises otherwise), another dtype --
    # is added by numpy with numpy's own broadcasting rules
    fuse = (B.ndim <= 1 or B.shape == (1, m)) and B.size == m and np.result_type(dt, B.dtype) == dt
    bias = np.ascontiguousarray(B.reshape(m), dtype=dt) if fuse else None
    out = np.empty((n, m), dtype=dt)
    # a private context on its own stream: the shared per-device context (and whichever torch stream it follows)
    # is left alone
    global _svm_ctx
    if _svm_ctx is None:
        _svm_ctx = _lib.Context()
    ctx = _svm_ctx
    fn = ctx.lib.vdet_svm_scores_f32 if dt == np.float32 else ctx.lib.vdet_svm_scores_f64
    ctx.check(fn(ctx.h, a.ctypes.data, n, k, w.ctypes.data, bias.ctypes.data if bias is not None else None, m,
                 out.ctypes.data))
    return out if bias is not None else out + B


_svm_ctx = None
