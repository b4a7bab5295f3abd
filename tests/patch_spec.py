"""Numpy restatement of the R-CNN window warp (ops.rcnn_patches / ops.tubelet_patches): what the device must equal bit for bit.

Geometry: ``rcnn_img_crop`` of the reference (utils/common.py:208-280), line for line, with Python 2's ``round`` (half AWAY from
zero) spelled out.  Resize: the rule the project fixes for a bilinear resize of 64-bit input -- per destination column
``fx = float32((dx + 0.5) * (src_w / float(dst_w)) - 0.5)``, ``sx = floor(fx)``, ``fx -= sx`` in float32, clamped at both ends
with a zero fraction, weights ``1.f - fx`` / ``fx`` in float32 widened to float64, rows first (``S[sx]*a0 + S[sx+1]*a1``) then
columns (``r0*b0 + r1*b1``), every product and sum a separate float64 operation.  Parity of that rule with OpenCV's
``cv2.resize(..., INTER_LINEAR)`` is UNPINNED: OpenCV is not available where the goldens are made.

One window at a time in plain Python; imports nothing from the package under test.
"""
import math

import numpy as np


def round_half_away(x):
    """Python 2's round(): halves go away from zero (2.5 -> 3, -0.5 -> -1).  Never Python 3's round, never numpy's."""
    x = float(x)
    if x != x or x in (float('inf'), float('-inf')):
        return x
    return math.floor(x + 0.5) if x >= 0 else -math.floor(-x + 0.5)


def _finite(x):
    return x - x == 0.0


def geometry(in_bbox, H, W, crop_mode, S, padding):
    """-> dict(ok, x1, y1, src_w, src_h, crop_w, crop_h, pad_w, pad_h): the source rectangle (inclusive origin, size), the size it
    is resized to and where it is placed.  ok = 0: the reference raises inside cv2.resize (or the input is not finite, or a
    'warp' window without padding leaves the image)."""
    bad = dict(ok=0, x1=0, y1=0, src_w=0, src_h=0, crop_w=S, crop_h=S, pad_w=0, pad_h=0)
    b = [float(v) for v in in_bbox]
    if not all(_finite(v) for v in b):
        return bad
    bbox = [v - 1.0 for v in b]
    use_square = crop_mode == 'square'
    pad_w = pad_h = 0
    crop_width = crop_height = S
    if padding > 0 or use_square:
        scale = S * 1.0 / (S - padding * 2)
        half_height = (bbox[3] - bbox[1] + 1) / 2.0
        half_width = (bbox[2] - bbox[0] + 1) / 2.0
        center = [bbox[0] + half_width, bbox[1] + half_height]
        if use_square:
            if half_height > half_width:
                half_width = half_height
            else:
                half_height = half_width
        bbox = [round_half_away(v) for v in (center[0] - half_width * scale, center[1] - half_height * scale,
                                             center[0] + half_width * scale, center[1] + half_height * scale)]
        if not all(_finite(v) for v in bbox):
            return bad
        unclipped_height = bbox[3] - bbox[1] + 1
        unclipped_width = bbox[2] - bbox[0] + 1
        pad_x1 = -bbox[0] if -bbox[0] > 0 else 0.0
        pad_y1 = -bbox[1] if -bbox[1] > 0 else 0.0
        bbox[0] = bbox[0] if bbox[0] > 0 else 0.0
        bbox[1] = bbox[1] if bbox[1] > 0 else 0.0
        bbox[2] = bbox[2] if bbox[2] < W - 1 else float(W - 1)
        bbox[3] = bbox[3] if bbox[3] < H - 1 else float(H - 1)
        clipped_height = bbox[3] - bbox[1] + 1
        clipped_width = bbox[2] - bbox[0] + 1
        if not (unclipped_height >= 1 and unclipped_width >= 1 and clipped_height >= 1 and clipped_width >= 1):
            return bad
        scale_x = S * 1.0 / unclipped_width
        scale_y = S * 1.0 / unclipped_height
        crop_width = int(round_half_away(clipped_width * scale_x))
        crop_height = int(round_half_away(clipped_height * scale_y))
        pad_x1 = int(round_half_away(pad_x1 * scale_x))
        pad_y1 = int(round_half_away(pad_y1 * scale_y))
        pad_h = pad_y1
        pad_w = pad_x1
        if pad_y1 + crop_height > S:
            crop_height = S - pad_y1
        if pad_x1 + crop_width > S:
            crop_width = S - pad_x1
        if crop_width < 1 or crop_height < 1:
            return bad
    else:
        bbox = [float(math.trunc(v)) for v in bbox]
        if not (0 <= bbox[0] <= bbox[2] <= W - 1 and 0 <= bbox[1] <= bbox[3] <= H - 1):
            return bad          # (numpy would slice a shorter or a wrapped window: flagged instead)
    x1, y1, x2, y2 = [int(v) for v in bbox]
    return dict(ok=1, x1=x1, y1=y1, src_w=x2 - x1 + 1, src_h=y2 - y1 + 1, crop_w=crop_width, crop_h=crop_height, pad_w=pad_w,
                pad_h=pad_h)


def _axis(src, dst):
    """Source index pairs and float64 weights of one axis: (s0 [dst], s1 [dst], w0 [dst], w1 [dst])."""
    d = np.arange(dst, dtype=np.float64)
    f = ((d + 0.5) * (src / float(dst)) - 0.5).astype(np.float32)
    s = np.floor(f)
    f = f - s                              # float32
    s = s.astype(np.int64)
    lo = s < 0
    s[lo] = 0
    f[lo] = 0
    hi = s >= src - 1
    s[hi] = src - 1
    f[hi] = 0
    assert f.dtype == np.float32
    w0 = (np.float32(1) - f).astype(np.float64)
    w1 = f.astype(np.float64)
    return s, np.minimum(s + 1, src - 1), w0, w1


def resize_linear(window, dst_w, dst_h):
    """window [h,w,ch] of any dtype -> float64 [dst_h,dst_w,ch]."""
    win = np.asarray(window).astype(np.float64)
    h, w = win.shape[:2]
    if (w, h) == (dst_w, dst_h):
        return win.copy()
    x0, x1, a0, a1 = _axis(w, dst_w)
    y0, y1, b0, b1 = _axis(h, dst_h)
    a0, a1 = a0[None, :, None], a1[None, :, None]
    r0 = win[y0][:, x0] * a0 + win[y0][:, x1] * a1
    r1 = win[y1][:, x0] * a0 + win[y1][:, x1] * a1
    return r0 * b0[:, None, None] + r1 * b1[:, None, None]


def rcnn_window(img, in_bbox, crop_mode, S, padding, mean=None):
    """One window: (float32 [S,S,3] in the image's channel order -- the reference's rcnn_img_crop result --, ok)."""
    img = np.asarray(img)
    out = np.zeros((S, S, 3), dtype=np.float32)
    g = geometry(in_bbox, img.shape[0], img.shape[1], crop_mode, S, padding)
    if not g['ok']:
        return out, 0
    win = img[g['y1']:g['y1'] + g['src_h'], g['x1']:g['x1'] + g['src_w'], :]
    tmp = resize_linear(win, g['crop_w'], g['crop_h'])
    if mean is not None:
        tmp = tmp - np.asarray(mean, dtype=np.float64).reshape((1, 1, 3))
    out[g['pad_h']:g['pad_h'] + g['crop_h'], g['pad_w']:g['pad_w'] + g['crop_w']] = tmp
    return out, 1


def rcnn_patches(images, boxes, image_idx=None, crop_mode='warp', S=224, padding=16, mean=None):
    """images [Fi,H,W,3] uint8, boxes [M,4] -> (patches float32 [M,3,S,S], ok uint8 [M]).  An image index out of range: ok = 0."""
    images = np.asarray(images)
    boxes = np.asarray(boxes)
    M = boxes.shape[0]
    patches = np.zeros((M, 3, S, S), dtype=np.float32)
    ok = np.zeros((M,), dtype=np.uint8)
    for m in range(M):
        i = 0 if image_idx is None else int(image_idx[m])
        if not 0 <= i < images.shape[0]:
            continue
        win, ok[m] = rcnn_window(images[i], boxes[m].astype(np.float64), crop_mode, S, padding, mean)
        patches[m] = win.transpose(2, 0, 1)
    return patches, ok


def sampling_boxes(boxes, offsets):
    """sampling_boxes (vdet/tubelet_cls.py:136-142, return_orig=True) with the draw supplied: boxes [N,4], offsets [N,num,4] ->
    float64 [N,num+1,4]; w = x2-x1, h = y2-y1 (no +1)."""
    b = np.asarray(boxes).astype(np.float64)
    off = np.asarray(offsets, dtype=np.float64)
    w, h = b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]
    whwh = np.stack([w, h, w, h], axis=1)[:, None, :]
    return np.concatenate([b[:, None, :], b[:, None, :] + off * whwh], axis=1)


def tubelet_slots(tracks, ntracks, f0, f1):
    """The present slots of frames f0 <= f < f1 in the order ((f-f0)*C + c)*T + t: int32 [count,3] rows (c,t,f)."""
    tracks = np.asarray(tracks)
    C, T = tracks.shape[:2]
    out = []
    for f in range(f0, f1):
        for c in range(C):
            for t in range(T):
                if t < int(ntracks[c]) and tracks[c, t, f, 0] == tracks[c, t, f, 0]:
                    out.append((c, t, f))
    return np.asarray(out, dtype=np.int32).reshape(-1, 3)
