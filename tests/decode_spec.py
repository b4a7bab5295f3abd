"""THE rule of ops.decode_boxes, ops.det_nms_volume_deltas and ops.tubelet_dets (csrc/decode_kernels.hpp, include/vdet_hip.h:
vdet_decode_boxes) in numpy float64: the Fast R-CNN box decode, per box and class.

It is the arithmetic of ``image_det.bbox_transform_inv`` followed by ``image_det.clip_boxes``.  With the roi (x1,y1,x2,y2),
widened exactly to f64 from f32 or taken as f64, and the class's deltas (dx,dy,dw,dh), f32 widened exactly:
    w   = (x2 - x1) + 1e-14        cx  = x1 + 0.5*w
    pcx = dx*w + cx                pw  = E(dw)*w
    X1  = pcx - 0.5*pw             X2  = pcx + 0.5*pw                       (y alike, with h, cy, dy, dh)
    out = f32(clip(X1, W-1)), f32(clip(Y1, H-1)), f32(clip(X2, W-1)), f32(clip(Y2, H-1))
Every product and every sum is ONE correctly rounded f64 operation (the library is built with -ffp-contract=off: no fused
multiply-add) and the only rounding to f32 is the last one (round to nearest even; beyond the f32 range: inf).

clip(v, hi) is numpy's ``np.maximum(np.minimum(v, hi), 0)`` written out, so that it does not depend on the host's vector unit:
    NaN if v is NaN;  hi if v > hi;  v if v > 0;  else +0.0
-- a NaN stays a NaN (the device's fmin / fmax would drop it) and -0.0, like every v <= 0, becomes +0.0.  A roi or delta that
is not finite therefore gives NaN coordinates or clipped ones, nothing else: no status, no error.

E is the only departure from the host functions, which call np.exp: an exponential as a FIXED sequence of IEEE f64 operations
that numpy has too (compare, multiply, rint, subtract, add, ldexp), which the kernel repeats bit for bit:
    NaN -> NaN;   x > E_HI = 709 -> +inf;   x < E_LO = -708 -> +0.0    (both signs of infinity included); otherwise
    k = rint(x * LOG2E)            (|k| <= 1023)
    r = (x - k*LN2_HI) - k*LN2_LO  (k*LN2_HI is exact: LN2_HI has 21 trailing zero bits; |r| <= 0.3466)
    p = 1/13!;  p = p*r + 1/n! for n = 12 .. 0      (Horner, degree 13: the remainder r^14/14! is below 5e-18)
    E = ldexp(p, k)                (exact: p lies in [0.70, 1.42] and k in [-1022, 1023], the result is a normal number)
exp(x) overflows from x = 709.78 on and is subnormal below x = -708.40; E gives up the two slivers (709, 709.78] and
[-708.40, -708) so that ldexp never rounds.  No clamp of dw is added: the restated Fast R-CNN rule has none.
"""
import math

import numpy as np

F32, F64 = np.float32, np.float64

E_HI, E_LO = F64(709.0), F64(-708.0)
E_LOG2E = F64(1.4426950408889634)                 # 0x3FF71547652B82FE
E_LN2_HI = F64(float.fromhex('0x1.62e42feep-1'))  # 6.93147180369123816490e-01 (fdlibm's ln2HI)
E_LN2_LO = F64(float.fromhex('0x1.a39ef35793c76p-33'))  # 1.90821492927058770002e-10 (fdlibm's ln2LO)
E_COEF = tuple(F64(1.0) / F64(math.factorial(n)) for n in range(13, -1, -1))    # 1/13! .. 1/0!, each one rounding of the quotient
EPS = F64(1e-14)


def E(x):
    """f64 array (or scalar) -> f64: the sequence the kernel repeats"""
    x = np.asarray(x, F64)
    with np.errstate(all='ignore'):
        nan, hi, lo = np.isnan(x), x > E_HI, x < E_LO
        xs = np.where(nan | hi | lo, F64(0.0), x)
        k = np.rint(xs * E_LOG2E)
        r = (xs - k * E_LN2_HI) - k * E_LN2_LO
        p = E_COEF[0]
        for c in E_COEF[1:]:
            p = p * r + c
        out = np.ldexp(p, k.astype(np.int32))
    return np.where(nan, F64(np.nan), np.where(hi, F64(np.inf), np.where(lo, F64(0.0), out)))


def clip(v, hi):
    """np.maximum(np.minimum(v, hi), 0), written out"""
    v = np.asarray(v, F64)
    with np.errstate(invalid='ignore'):
        return np.where(np.isnan(v), v, np.where(v > hi, F64(hi), np.where(v > 0, v, F64(0.0))))


def _check(rois, deltas):
    rois, deltas = np.asarray(rois), np.asarray(deltas)
    assert rois.dtype in (F32, F64) and deltas.dtype == F32, (rois.dtype, deltas.dtype)
    assert rois.shape[-1] == 4 and deltas.shape[-1] == 4 and deltas.shape[:-2] == rois.shape[:-1], (rois.shape, deltas.shape)
    return rois.astype(F64), deltas.astype(F64)


def decode(rois, deltas, im_size):
    """rois [...,4] f32 / f64, deltas [...,K,4] f32, im_size (H, W) -> float32 [...,K,4]"""
    r, d = _check(rois, deltas)
    H, W = im_size
    with np.errstate(all='ignore'):
        w = ((r[..., 2] - r[..., 0]) + EPS)[..., None]
        h = ((r[..., 3] - r[..., 1]) + EPS)[..., None]
        cx = r[..., 0, None] + F64(0.5) * w
        cy = r[..., 1, None] + F64(0.5) * h
        pcx = d[..., 0] * w + cx
        pcy = d[..., 1] * h + cy
        pw = E(d[..., 2]) * w
        ph = E(d[..., 3]) * h
        out = np.stack([clip(pcx - F64(0.5) * pw, W - 1), clip(pcy - F64(0.5) * ph, H - 1),
                        clip(pcx + F64(0.5) * pw, W - 1), clip(pcy + F64(0.5) * ph, H - 1)], axis=-1)
        return out.astype(F32)


def E_loop(x):
    """E for one python float, operation by operation"""
    x = F64(x)
    if x != x:
        return F64(np.nan)
    if x > E_HI:
        return F64(np.inf)
    if x < E_LO:
        return F64(0.0)
    k = F64(np.rint(x * E_LOG2E))
    r = (x - k * E_LN2_HI) - k * E_LN2_LO
    p = E_COEF[0]
    for c in E_COEF[1:]:
        p = F64(p * r) + c
    return F64(math.ldexp(float(p), int(k)))


def clip_loop(v, hi):
    if v != v:
        return v
    if v > hi:
        return F64(hi)
    return v if v > 0 else F64(0.0)


def decode_loop(rois, deltas, im_size):
    """``decode`` as a plain loop over boxes and classes (the transcription test_decode_cpu.py holds ``decode`` against)"""
    r, d = _check(rois, deltas)
    H, W = im_size
    K = d.shape[-2]
    r2, d2 = r.reshape(-1, 4), d.reshape(-1, K, 4)
    out = np.empty(d2.shape, F32)
    with np.errstate(all='ignore'):
        for n in range(len(r2)):
            x1, y1, x2, y2 = r2[n]
            w, h = (x2 - x1) + EPS, (y2 - y1) + EPS
            cx, cy = x1 + F64(0.5) * w, y1 + F64(0.5) * h
            for k in range(K):
                dx, dy, dw, dh = d2[n, k]
                pcx, pcy = dx * w + cx, dy * h + cy
                pw, ph = E_loop(dw) * w, E_loop(dh) * h
                out[n, k] = (F32(clip_loop(pcx - F64(0.5) * pw, W - 1)), F32(clip_loop(pcy - F64(0.5) * ph, H - 1)),
                             F32(clip_loop(pcx + F64(0.5) * pw, W - 1)), F32(clip_loop(pcy + F64(0.5) * ph, H - 1)))
    return out.reshape(d.shape)


SRC_PAD = np.int32(-2 ** 31)


def dets_as_tracks(dets, sel_idx, keep, keep_cnt, first_class=1):
    """The rank layout of ops.dets_as_tracks from a loop: the kept rows of every (frame, class), in keep order"""
    F, K, topk = sel_idx.shape
    C = K - first_class
    out = dict(tracks=np.full((C, topk, F, 5), np.nan, F32), score=np.full((C, topk, F), np.nan, F64),
               src=np.full((C, topk, F), SRC_PAD, np.int32), cnt=np.zeros((C, F), np.int32), ntracks=np.zeros(C, np.int32))
    for f in range(F):
        for c in range(C):
            j = c + first_class
            n = int(keep_cnt[f, j])
            out['cnt'][c, f] = n
            out['ntracks'][c] = max(out['ntracks'][c], n)
            for r in range(n):
                row = int(keep[f, j, r])
                out['tracks'][c, r, f] = dets[f, j, row]
                out['score'][c, r, f] = F64(dets[f, j, row, 4])
                out['src'][c, r, f] = sel_idx[f, j, row]
    return out
