"""The rules of RoI pooling (ops.roi_pool / ops.tubelet_rois, include/vdet_hip.h: vdet_roi_pool) in numpy: the definition the
device is compared with bit for bit.

Both rules are RESTATED from public code -- 'max' from the forward pass of Caffe's ROIPoolingLayer (Fast R-CNN, Dtype = float),
'align' from the RoIAlign forward (He et al. 2017) as the common detection libraries ship it -- which was not at hand when this
was written: the restatement could not be checked against it.  This file is the definition.

Inputs of both modes: features [Fi,K,Hf,Wf] float32 (f16 / bf16 features are widened exactly by the caller; the f32 result is
rounded once to their dtype, also by the caller), boxes [N,4] as they are (no 1-based shift), image_idx [N] or None (image 0),
spatial_scale, pooled = (ph, pw), box_scale.

A RoI is r = f32(f64(box) * f64(box_scale)) per coordinate.  ok = 0 and an all-zero output where a coordinate of r is not
finite, |r * f32(spatial_scale)| > 2^24 (an f32 product), or the image index is outside [0, Fi).

Every function exists twice: ``*_loop`` is the plain transcription, one scalar operation at a time; the other is vectorised
over channels (and, for 'align', over the samples of a RoI) and visits the cells / samples in the same order."""
import numpy as np

F32 = np.float32
FLT_MAX = np.finfo(np.float32).max
LIMIT = F32(2.0 ** 24)


def rois(boxes, box_scale):
    """r = f32(f64(box) * f64(box_scale)) -> float32 [N,4]."""
    with np.errstate(over='ignore', invalid='ignore'):
        return (np.asarray(boxes).astype(np.float64).reshape(-1, 4) * np.float64(box_scale)).astype(np.float32)


def roi_ok(r, spatial_scale, img, Fi):
    """The status of one RoI r (float32 [4]) cut from image ``img``."""
    with np.errstate(over='ignore', invalid='ignore'):
        prod = r * F32(spatial_scale)
        return bool(np.all(np.isfinite(r)) and np.all(np.abs(prod) <= LIMIT) and 0 <= int(img) < Fi)


def c_round(x):
    """C round() of float32 values with |x| <= 2^24: halves away from zero -> int64."""
    x = np.asarray(x, dtype=np.float64)
    return (np.sign(x) * np.floor(np.abs(x) + 0.5)).astype(np.int64)


def int_edges(r, spatial_scale):
    """x1c, y1c, x2c, y2c of 'max': round(r * f32(spatial_scale)), the product in f32."""
    return [int(v) for v in c_round(r * F32(spatial_scale))]


def max_bins(r, spatial_scale, Hf, Wf, ph, pw):
    """(hs [ph], he [ph], ws [pw], we [pw]) of 'max': the f32 bin edges, shifted by the start cell and clamped to the map."""
    x1c, y1c, x2c, y2c = int_edges(r, spatial_scale)
    rw, rh = max(x2c - x1c + 1, 1), max(y2c - y1c + 1, 1)
    bw, bh = F32(rw) / F32(pw), F32(rh) / F32(ph)
    p, q = np.arange(ph), np.arange(pw)
    hs = np.floor(p.astype(F32) * bh).astype(np.int64) + y1c
    he = np.ceil((p + 1).astype(F32) * bh).astype(np.int64) + y1c
    ws = np.floor(q.astype(F32) * bw).astype(np.int64) + x1c
    we = np.ceil((q + 1).astype(F32) * bw).astype(np.int64) + x1c
    return np.clip(hs, 0, Hf), np.clip(he, 0, Hf), np.clip(ws, 0, Wf), np.clip(we, 0, Wf)


def integer_bins(r, spatial_scale, Hf, Wf, ph, pw):
    """The same edges in exact integer arithmetic (floor(p*rh/ph), ceil((p+1)*rh/ph)): NOT the rule -- what the f32 edges are
    told apart from (tests/test_roipool_cpu.py guards that the case list holds RoIs where the two differ)."""
    x1c, y1c, x2c, y2c = int_edges(r, spatial_scale)
    rw, rh = max(x2c - x1c + 1, 1), max(y2c - y1c + 1, 1)
    p, q = np.arange(ph), np.arange(pw)
    hs, he = (p * rh) // ph + y1c, -((-(p + 1) * rh) // ph) + y1c
    ws, we = (q * rw) // pw + x1c, -((-(q + 1) * rw) // pw) + x1c
    return np.clip(hs, 0, Hf), np.clip(he, 0, Hf), np.clip(ws, 0, Wf), np.clip(we, 0, Wf)


def _prepare(features, boxes, image_idx, box_scale, pooled):
    features = np.asarray(features)
    assert features.dtype == np.float32 and features.ndim == 4
    r = rois(boxes, box_scale)
    N = len(r)
    idx = np.zeros(N, np.int64) if image_idx is None else np.asarray(image_idx).astype(np.int64)
    ph, pw = pooled
    out = np.zeros((N, features.shape[1], ph, pw), np.float32)
    return features, r, idx, out, np.zeros(N, np.uint8)


# ---------------------------------------------------------------------------------------------- 'max'
def roi_pool_max_loop(features, boxes, image_idx=None, spatial_scale=1 / 16., pooled=(7, 7), box_scale=1.0):
    features, r, idx, out, ok = _prepare(features, boxes, image_idx, box_scale, pooled)
    Fi, K, Hf, Wf = features.shape
    ph, pw = pooled
    for n in range(len(r)):
        if not roi_ok(r[n], spatial_scale, idx[n], Fi):
            continue
        ok[n] = 1
        hs, he, ws, we = max_bins(r[n], spatial_scale, Hf, Wf, ph, pw)
        for k in range(K):
            plane = features[idx[n], k]
            for p in range(ph):
                for q in range(pw):
                    if he[p] <= hs[p] or we[q] <= ws[q]:
                        continue                                      # an empty bin: 0
                    best = F32(-FLT_MAX)
                    for h in range(hs[p], he[p]):
                        for w in range(ws[q], we[q]):
                            if plane[h, w] > best:                    # NaN never wins, -inf never wins
                                best = plane[h, w]
                    out[n, k, p, q] = best
    return out, ok


def roi_pool_max(features, boxes, image_idx=None, spatial_scale=1 / 16., pooled=(7, 7), box_scale=1.0):
    """Vectorised over channels; the cells of a bin are visited row-major, one ``where(v > best)`` per cell, so that the first
    of two equal cells (+0.0 / -0.0) stays."""
    features, r, idx, out, ok = _prepare(features, boxes, image_idx, box_scale, pooled)
    Fi, K, Hf, Wf = features.shape
    ph, pw = pooled
    for n in range(len(r)):
        if not roi_ok(r[n], spatial_scale, idx[n], Fi):
            continue
        ok[n] = 1
        hs, he, ws, we = max_bins(r[n], spatial_scale, Hf, Wf, ph, pw)
        img = features[idx[n]]
        for p in range(ph):
            for q in range(pw):
                if he[p] <= hs[p] or we[q] <= ws[q]:
                    continue
                cells = img[:, hs[p]:he[p], ws[q]:we[q]].reshape(K, -1)
                best = np.full(K, -FLT_MAX, np.float32)
                for j in range(cells.shape[1]):
                    v = cells[:, j]
                    best = np.where(v > best, v, best)
                out[n, :, p, q] = best
    return out, ok


# ---------------------------------------------------------------------------------------------- 'align'
def align_axis(r1, r2, spatial_scale, size, pn, sampling, aligned):
    """One axis of 'align': per sample j = p*sampling + i of the pn bins -> (valid, lo, hi, l, h).  Everything float32, every
    product and sum a separate operation."""
    scale, off = F32(spatial_scale), F32(0.5 if aligned else 0.0)
    s = r1 * scale - off
    ext = r2 * scale - off - s
    if not aligned and ext < F32(1.0):
        ext = F32(1.0)
    b = ext / F32(pn)
    valid, lo, hi, l, h = [], [], [], [], []
    for p in range(pn):
        for i in range(sampling):
            y = s + F32(p) * b + (F32(i) + F32(0.5)) * b / F32(sampling)
            if y < F32(-1.0) or y > F32(size):
                valid.append(False); lo.append(0); hi.append(0); l.append(F32(0)); h.append(F32(0))
                continue
            if y <= F32(0):
                y = F32(0)
            a = int(y)
            if a >= size - 1:
                a = c = size - 1
                y = F32(a)
            else:
                c = a + 1
            ly = y - F32(a)
            valid.append(True); lo.append(a); hi.append(c); l.append(ly); h.append(F32(1.0) - ly)
    return (np.asarray(valid), np.asarray(lo, np.int64), np.asarray(hi, np.int64), np.asarray(l, np.float32),
            np.asarray(h, np.float32))


def roi_align_loop(features, boxes, image_idx=None, spatial_scale=1 / 16., pooled=(7, 7), box_scale=1.0, sampling=2, aligned=False):
    features, r, idx, out, ok = _prepare(features, boxes, image_idx, box_scale, pooled)
    Fi, K, Hf, Wf = features.shape
    ph, pw = pooled
    S = sampling
    with np.errstate(over='ignore', invalid='ignore'):
        for n in range(len(r)):
            if not roi_ok(r[n], spatial_scale, idx[n], Fi):
                continue
            ok[n] = 1
            yv, ylo, yhi, ly, hy = align_axis(r[n, 1], r[n, 3], spatial_scale, Hf, ph, S, aligned)
            xv, xlo, xhi, lx, hx = align_axis(r[n, 0], r[n, 2], spatial_scale, Wf, pw, S, aligned)
            for k in range(K):
                plane = features[idx[n], k]
                for p in range(ph):
                    for q in range(pw):
                        acc = F32(0)
                        for iy in range(S):
                            for ix in range(S):
                                a, b = p * S + iy, q * S + ix
                                val = F32(0)
                                if yv[a] and xv[b]:
                                    w1, w2, w3, w4 = hy[a] * hx[b], hy[a] * lx[b], ly[a] * hx[b], ly[a] * lx[b]
                                    v1, v2 = plane[ylo[a], xlo[b]], plane[ylo[a], xhi[b]]
                                    v3, v4 = plane[yhi[a], xlo[b]], plane[yhi[a], xhi[b]]
                                    val = ((w1 * v1 + w2 * v2) + w3 * v3) + w4 * v4
                                acc = acc + val
                        out[n, k, p, q] = acc / F32(S * S)
    return out, ok


def roi_align(features, boxes, image_idx=None, spatial_scale=1 / 16., pooled=(7, 7), box_scale=1.0, sampling=2, aligned=False):
    """Vectorised over the channels and the samples of a RoI; the samples of a bin are summed iy-major, then ix."""
    features, r, idx, out, ok = _prepare(features, boxes, image_idx, box_scale, pooled)
    Fi, K, Hf, Wf = features.shape
    ph, pw = pooled
    S = sampling
    with np.errstate(over='ignore', invalid='ignore'):
        for n in range(len(r)):
            if not roi_ok(r[n], spatial_scale, idx[n], Fi):
                continue
            ok[n] = 1
            yv, ylo, yhi, ly, hy = align_axis(r[n, 1], r[n, 3], spatial_scale, Hf, ph, S, aligned)
            xv, xlo, xhi, lx, hx = align_axis(r[n, 0], r[n, 2], spatial_scale, Wf, pw, S, aligned)
            img = features[idx[n]]
            w1, w2 = hy[:, None] * hx[None, :], hy[:, None] * lx[None, :]
            w3, w4 = ly[:, None] * hx[None, :], ly[:, None] * lx[None, :]
            v1, v2 = img[:, ylo[:, None], xlo[None, :]], img[:, ylo[:, None], xhi[None, :]]
            v3, v4 = img[:, yhi[:, None], xlo[None, :]], img[:, yhi[:, None], xhi[None, :]]
            val = ((w1 * v1 + w2 * v2) + w3 * v3) + w4 * v4
            val = np.where(yv[:, None] & xv[None, :], val, F32(0)).astype(np.float32).reshape(K, ph, S, pw, S)
            acc = np.zeros((K, ph, pw), np.float32)
            for iy in range(S):
                for ix in range(S):
                    acc = acc + val[:, :, iy, :, ix]
            out[n] = acc / F32(S * S)
    return out, ok


def roi_pool(features, boxes, image_idx=None, spatial_scale=1 / 16., pooled=(7, 7), box_scale=1.0, mode='max', sampling=2,
             aligned=False, loop=False):
    """ops.roi_pool's signature on float32 numpy features -> (pooled float32 [N,K,ph,pw], ok uint8 [N])."""
    if mode == 'max':
        return (roi_pool_max_loop if loop else roi_pool_max)(features, boxes, image_idx, spatial_scale, pooled, box_scale)
    assert mode == 'align'
    return (roi_align_loop if loop else roi_align)(features, boxes, image_idx, spatial_scale, pooled, box_scale, sampling, aligned)


# ---------------------------------------------------------------------------------------------- the Fast R-CNN box decode
def bbox_transform_inv_loop(boxes, deltas):
    """The loop statement of image_det.bbox_transform_inv: float64, one box and one class at a time."""
    boxes = np.asarray(boxes, dtype=np.float64)
    deltas = np.asarray(deltas, dtype=np.float64)
    out = np.zeros(deltas.shape, np.float64)
    for n in range(len(boxes)):
        w = boxes[n, 2] - boxes[n, 0] + 1e-14
        h = boxes[n, 3] - boxes[n, 1] + 1e-14
        cx, cy = boxes[n, 0] + 0.5 * w, boxes[n, 1] + 0.5 * h
        for j in range(deltas.shape[1] // 4):
            dx, dy, dw, dh = deltas[n, 4 * j:4 * j + 4]
            pcx, pcy = dx * w + cx, dy * h + cy
            pw, ph = np.exp(dw) * w, np.exp(dh) * h
            out[n, 4 * j:4 * j + 4] = [pcx - 0.5 * pw, pcy - 0.5 * ph, pcx + 0.5 * pw, pcy + 0.5 * ph]
    return out


def clip_boxes_loop(boxes, im_shape):
    boxes = np.array(boxes, dtype=np.float64)
    for n in range(boxes.shape[0]):
        for j in range(boxes.shape[1]):
            hi = (im_shape[1] if j % 2 == 0 else im_shape[0]) - 1
            boxes[n, j] = max(min(boxes[n, j], hi), 0)
    return boxes
