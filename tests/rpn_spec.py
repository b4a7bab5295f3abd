"""THE rule of ops.rpn_proposals (csrc/proposal_kernels.hpp, include/vdet_hip.h: vdet_rpn_proposals) in numpy float64: the
proposal layer of a region proposal network, per frame.

It RESTATES the public py-faster-rcnn proposal layer (``rpn/generate_anchors.py``, ``rpn/proposal_layer.py``), which was NOT
at hand: parity with that code's float32 host arithmetic is unpinned.  The device is pinned to THIS file bit for bit.

Inputs of a frame: scores [A,Hf,Wf] f32 (the foreground half of the RPN's class output; logits or probabilities, the ranking
is monotone), deltas [4A,Hf,Wf] f32 (channel 4a+k is component k of anchor a), anchors [A,4] f64.

Anchor.  The candidate of flat index n = (h*Wf + w)*A + a has the roi  anchors[a] + (w*stride, h*stride, w*stride, h*stride)
in f64 (the products are exact).

Decode.  ``decode_spec.decode``'s arithmetic (f64, its exponential E, its clip, ONE rounding to f32) with two additions:
    w = (x2 - x1) + offset        offset = 1.0 is the RPN's pixel convention; 1e-14 reproduces decode_spec.decode bit for bit
    dw_max                        a dw or dh GREATER than dw_max becomes dw_max before E; NaN stays NaN; None: no clamp
and the boxes are clipped to im_size = (H, W): x to [0, W-1], y to [0, H-1].

Validity.  n is a candidate when its score is not NaN and, on the f32-rounded clipped box evaluated in f64,
(X2 - X1) + 1 >= min_size and (Y2 - Y1) + 1 >= min_size (a NaN coordinate fails the comparison).

Order.  Candidates by descending score, equal scores by DESCENDING flat index (the build's reading of ``argsort()[::-1]``,
include/vdet_hip.h:24-27); -0.0 == +0.0, +inf and -inf are ordinary scores.  The first pre_nms_top_n of that order are kept (ties
at the cut go to the highest indices), greedy NMS at nms_thresh runs over them in that order with the arithmetic of
utils/nms.pyx (``oracle.nms`` with the identity order), and the first post_nms_top_n survivors are the proposals.  More
survivors than post_nms_top_n is no error.

``proposals`` is the vectorised form, ``proposals_loop`` the plain loop test_rpn_cpu.py holds it against.
"""
import numpy as np

import decode_spec
from decode_spec import E, E_loop, clip, clip_loop

F32, F64 = np.float32, np.float64


def generate_anchors(base_size=16, ratios=(0.5, 1, 2), scales=(8, 16, 32)):
    """f64 [A,4], ratio-major (A = len(ratios) * len(scales)); np.round on the ratio widths and heights"""
    ratios, scales = np.asarray(ratios, F64), np.asarray(scales, F64)
    w = h = F64(base_size)
    ctr = F64(0.5) * (F64(base_size) - 1)         # the centre of (0, 0, base_size - 1, base_size - 1)
    ws = np.round(np.sqrt(w * h / ratios))
    hs = np.round(ws * ratios)
    ws = (ws[:, None] * scales[None, :]).reshape(-1)
    hs = (hs[:, None] * scales[None, :]).reshape(-1)
    return np.stack([ctr - F64(0.5) * (ws - 1), ctr - F64(0.5) * (hs - 1),
                     ctr + F64(0.5) * (ws - 1), ctr + F64(0.5) * (hs - 1)], axis=1)


def _check(scores, deltas, anchors):
    scores, deltas, anchors = np.asarray(scores), np.asarray(deltas), np.asarray(anchors)
    assert scores.dtype == F32 and deltas.dtype == F32 and anchors.dtype == F64, (scores.dtype, deltas.dtype, anchors.dtype)
    F, A, Hf, Wf = scores.shape
    assert anchors.shape == (A, 4) and deltas.shape == (F, 4 * A, Hf, Wf), (scores.shape, deltas.shape, anchors.shape)
    return F, A, Hf, Wf


def shifted_anchors(anchors, Hf, Wf, stride):
    """f64 [Hf*Wf*A, 4] in flat-index order"""
    sx = (np.arange(Wf, dtype=F64) * F64(stride))[None, :, None]
    sy = (np.arange(Hf, dtype=F64) * F64(stride))[:, None, None]
    a = np.asarray(anchors, F64)[None, None, :, :]
    out = np.empty((Hf, Wf, a.shape[2], 4), F64)
    out[..., 0], out[..., 2] = a[..., 0] + sx, a[..., 2] + sx
    out[..., 1], out[..., 3] = a[..., 1] + sy, a[..., 3] + sy
    return out.reshape(-1, 4)


def decode(rois, deltas, im_size, offset=1.0, dw_max=None):
    """rois [N,4] f64, deltas [N,4] f32 -> f32 [N,4]: decode_spec.decode with the width term and the clamp"""
    r, d = np.asarray(rois, F64), np.asarray(deltas, F32).astype(F64)
    H, W = im_size
    off = F64(offset)
    with np.errstate(all='ignore'):
        w = (r[:, 2] - r[:, 0]) + off
        h = (r[:, 3] - r[:, 1]) + off
        cx = r[:, 0] + F64(0.5) * w
        cy = r[:, 1] + F64(0.5) * h
        dw, dh = d[:, 2], d[:, 3]
        if dw_max is not None:
            dw = np.where(dw > F64(dw_max), F64(dw_max), dw)
            dh = np.where(dh > F64(dw_max), F64(dw_max), dh)
        pcx = d[:, 0] * w + cx
        pcy = d[:, 1] * h + cy
        pw = E(dw) * w
        ph = E(dh) * h
        out = np.stack([clip(pcx - F64(0.5) * pw, W - 1), clip(pcy - F64(0.5) * ph, H - 1),
                        clip(pcx + F64(0.5) * pw, W - 1), clip(pcy + F64(0.5) * ph, H - 1)], axis=-1)
        return out.astype(F32)


def _nms_identity(boxes, scores, thresh):
    from oracle import oracle
    if len(boxes) == 0:
        return []
    rows = np.concatenate([boxes, scores[:, None]], axis=1).astype(F32)
    return oracle.nms(rows, thresh, order=np.arange(len(rows), dtype=np.int64))


def _empty(F, pre, post):
    return dict(rois=np.full((F, post, 4), np.nan, F32), scores=np.full((F, post), np.nan, F32),
                index=np.full((F, post), -1, np.int32), count=np.zeros(F, np.int32),
                cand_index=np.full((F, pre), -1, np.int32), cand_cnt=np.zeros(F, np.int32),
                nms_cnt=np.zeros(F, np.int32), tie_cut=np.zeros(F, bool))


def _finish_frame(out, f, boxes, s, sel, pre, post, nms_thresh):
    """sel: the candidates of frame f in order (flat indices); NMS and the cut at post"""
    out['cand_cnt'][f] = len(sel)
    out['cand_index'][f, :len(sel)] = sel
    keep = _nms_identity(boxes[sel], s[sel], nms_thresh)
    out['nms_cnt'][f] = len(keep)            # (the survivors before the cut: the case list's guards read it)
    keep = np.asarray(keep[:post], np.int64)
    n = len(keep)
    out['count'][f] = n
    out['rois'][f, :n] = boxes[sel][keep]
    out['scores'][f, :n] = s[sel][keep]
    out['index'][f, :n] = sel[keep]


def proposals(scores, deltas, anchors, im_size, stride=16, pre_nms_top_n=6000, post_nms_top_n=300, nms_thresh=0.7, min_size=16,
              offset=1.0, dw_max=None):
    """scores [F,A,Hf,Wf] f32, deltas [F,4A,Hf,Wf] f32, anchors [A,4] f64 -> dict of rois [F,post,4] f32 (NaN behind the count),
    scores [F,post] f32 (NaN), index [F,post] int32 (-1), count [F], cand_index [F,pre] int32 (-1), cand_cnt [F]; for the case list's guards also nms_cnt [F] (the survivors before the cut at
    post) and tie_cut [F] (the cut at pre fell inside a class of equal scores)"""
    F, A, Hf, Wf = _check(scores, deltas, anchors)
    pre, post = int(pre_nms_top_n), int(post_nms_top_n)
    N = Hf * Wf * A
    rois = shifted_anchors(anchors, Hf, Wf, stride)
    out = _empty(F, pre, post)
    for f in range(F):
        s = np.ascontiguousarray(np.asarray(scores[f]).transpose(1, 2, 0)).reshape(N)
        d = np.ascontiguousarray(np.asarray(deltas[f]).reshape(A, 4, Hf, Wf).transpose(2, 3, 0, 1)).reshape(N, 4)
        boxes = decode(rois, d, im_size, offset, dw_max)
        b = boxes.astype(F64)
        with np.errstate(invalid='ignore'):
            ok = ~np.isnan(s) & ((b[:, 2] - b[:, 0]) + F64(1.0) >= F64(min_size)) & ((b[:, 3] - b[:, 1]) + F64(1.0) >= F64(min_size))
        idx = np.nonzero(ok)[0]
        # descending score, equal scores (numpy compares -0.0 == +0.0) by descending index: lexsort's last key is the primary one
        order = idx[np.lexsort((-idx, -s[idx].astype(F64)))]
        sel = order[:pre]
        out['tie_cut'][f] = len(order) > pre and s[order[pre - 1]] == s[order[pre]]      # (for the case list's guards)
        _finish_frame(out, f, boxes, s, sel, pre, post, nms_thresh)
    return out


def decode_one(roi, d, im_size, offset, dw_max):
    """one box, operation by operation"""
    H, W = im_size
    x1, y1, x2, y2 = (F64(v) for v in roi)
    dx, dy, dw, dh = (F64(v) for v in d)
    off = F64(offset)
    with np.errstate(all='ignore'):
        w, h = (x2 - x1) + off, (y2 - y1) + off
        cx, cy = x1 + F64(0.5) * w, y1 + F64(0.5) * h
        if dw_max is not None:
            if dw > F64(dw_max):
                dw = F64(dw_max)
            if dh > F64(dw_max):
                dh = F64(dw_max)
        pcx, pcy = dx * w + cx, dy * h + cy
        pw, ph = E_loop(dw) * w, E_loop(dh) * h
        return (F32(clip_loop(pcx - F64(0.5) * pw, W - 1)), F32(clip_loop(pcy - F64(0.5) * ph, H - 1)),
                F32(clip_loop(pcx + F64(0.5) * pw, W - 1)), F32(clip_loop(pcy + F64(0.5) * ph, H - 1)))


def proposals_loop(scores, deltas, anchors, im_size, stride=16, pre_nms_top_n=6000, post_nms_top_n=300, nms_thresh=0.7,
                   min_size=16, offset=1.0, dw_max=None):
    """``proposals`` as a plain loop over frames, cells and anchors"""
    F, A, Hf, Wf = _check(scores, deltas, anchors)
    pre, post = int(pre_nms_top_n), int(post_nms_top_n)
    N = Hf * Wf * A
    out = _empty(F, pre, post)
    for f in range(F):
        boxes, s, cand = np.empty((N, 4), F32), np.empty(N, F32), []
        for h in range(Hf):
            for w in range(Wf):
                for a in range(A):
                    n = (h * Wf + w) * A + a
                    roi = (anchors[a, 0] + F64(w * stride), anchors[a, 1] + F64(h * stride),
                           anchors[a, 2] + F64(w * stride), anchors[a, 3] + F64(h * stride))
                    boxes[n] = decode_one(roi, deltas[f, 4 * a:4 * a + 4, h, w], im_size, offset, dw_max)
                    s[n] = scores[f, a, h, w]
                    X1, Y1, X2, Y2 = (F64(v) for v in boxes[n])
                    if s[n] == s[n] and (X2 - X1) + F64(1.0) >= F64(min_size) and (Y2 - Y1) + F64(1.0) >= F64(min_size):
                        cand.append(n)
        # insertion into the order: a candidate goes before another when its score is greater, or equal with a greater index
        cand.sort(key=lambda n: (-float(s[n]) if s[n] != 0 else 0.0, -n))
        out['tie_cut'][f] = len(cand) > pre and s[cand[pre - 1]] == s[cand[pre]]
        _finish_frame(out, f, boxes, s, np.asarray(cand[:pre], np.int64), pre, post, nms_thresh)
    return out


assert decode_spec.EPS == F64(1e-14)
