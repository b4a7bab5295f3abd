"""THE rule of ops.soft_nms_tracks (csrc/softnms_kernels.hpp, include/vdet_hip.h: vdet_soft_nms_tracks) in numpy float32.

Soft-NMS (Bodla et al., ICCV 2017) of one (class, frame) list.  The rows are nms_tracks' rows in its order
(test_nms_tracks_cpu.list_rows); every row carries a CURRENT f32 score, at first the f32 rounding of its source score.
  1. every row whose current score is < min_score (compared in f32) is removed;
  2. while a row is alive: the alive row with the largest current score (-0.0 == +0.0, equal scores by DESCENDING row index) is
     emitted with its current score bit for bit and is no longer alive; for every other alive row j, ovr is the f32 overlap
     of utils/nms.pyx:57-64 with the emitted box as box i (a zero union raises ZeroDivisionError), a NaN ovr changes
     nothing, and otherwise
       'linear':  iff (double)ovr >= thresh:  s_j = s_j * (1.0f - ovr)              (two f32 operations)
       'gauss':   s_j = s_j * g(-(ovr * ovr) / sigma)                               (thresh unused)
     after which a score that is NaN (inf * 0) or < min_score removes the row.
Every round is vectorised over the alive rows with float32 arrays: element by element these are the same single, correctly
rounded f32 operations as the scalar loop, so the bits are the loop's.

g is an exponential as a FIXED sequence of f32 operations that numpy has too (multiply, rint, subtract, add, ldexp, compare):
the argument rounded to a multiple of 2^-20, range reduction by ln 2 in two pieces, a degree-6 polynomial by Horner's scheme,
ldexp.  The rounding of the argument is what makes g MONOTONE over every float32: the polynomial's own rounding noise is about
one unit in the last place, which reorders neighbouring float32 arguments (2931 increases over the floats of [-87, 0] without
it), while one grid step moves the result by 8 to 16 units (no increase on the whole grid, nor on the grids of 2^-18 .. 2^-22).
The device repeats the sequence (the library is built with -ffp-contract=off) and must equal it on bits."""
import numpy as np

from test_nms_tracks_cpu import SRC_PAD, list_rows

F32 = np.float32
METHODS = ('linear', 'gauss')
SIGMA_MIN = 1.0 / 64            # the entry point's lower limit: with ovr <= 1 the argument of g stays in [-64, 0]
DEFAULTS = dict(method='linear', thresh=0.3, sigma=0.5, min_score=0.001)

G_CUT = F32(-87.0)              # exp(x) < 2^-126 from x = -87.34 on: below the cut g is +0.0 (every other result is a normal float)
G_GRID = F32(2.0 ** 20)         # the argument is rounded to a multiple of 1 / G_GRID (exact operations: a power of two, rint)
G_LOG2E = F32(1.4426950408889634)
G_LN2_HI = F32(0.693359375)     # 355 / 512: k * G_LN2_HI is exact for |k| < 2^15
G_LN2_LO = F32(-2.12194440e-4)  # ln 2 - G_LN2_HI
# exp(r) ~ 1 + r + r^2 (c2 + c3 r + c4 r^2 + c5 r^3 + c6 r^4) on |r| <= ln 2 / 2: a weighted least-squares fit towards the
# minimax polynomial, 3.1e-9 relative before any rounding
G_COEF = tuple(F32(c) for c in (0.0013814590638503432, 0.0083687175065279, 0.04166838899254799, 0.1666652113199234,
                                0.4999999403953552))


def g(x):
    """the Gaussian weight's exponential: float32 array (or scalar) x <= 0 -> float32, the sequence the kernel repeats"""
    x = np.asarray(x, F32)
    with np.errstate(invalid='ignore', over='ignore', under='ignore'):
        cut = x < G_CUT
        xs = np.rint(np.where(cut, F32(0.0), x) * G_GRID) * (F32(1.0) / G_GRID)
        kf = np.rint(xs * G_LOG2E)
        r = xs - kf * G_LN2_HI
        r = r - kf * G_LN2_LO
        p = G_COEF[0]
        for c in G_COEF[1:]:
            p = p * r + c
        p = p * r + F32(1.0)
        p = p * r + F32(1.0)
        out = np.ldexp(p.astype(F32), kf.astype(np.int32)).astype(F32)
    return np.where(cut, F32(0.0), out).astype(F32)


def overlaps(bi, boxes):
    """(ovr, uni) of utils/nms.pyx:57-64, box i = bi [4], boxes j = boxes [m,4], float32 operation by operation with the
    reference's max / min (a if a >= b else b; a if a <= b else b: with a NaN the second operand wins)"""
    one, zero = F32(1.0), F32(0.0)
    with np.errstate(all='ignore'):
        iarea = ((bi[2] - bi[0]) + one) * ((bi[3] - bi[1]) + one)
        jarea = ((boxes[:, 2] - boxes[:, 0]) + one) * ((boxes[:, 3] - boxes[:, 1]) + one)
        xx1 = np.where(bi[0] >= boxes[:, 0], bi[0], boxes[:, 0])
        yy1 = np.where(bi[1] >= boxes[:, 1], bi[1], boxes[:, 1])
        xx2 = np.where(bi[2] <= boxes[:, 2], bi[2], boxes[:, 2])
        yy2 = np.where(bi[3] <= boxes[:, 3], bi[3], boxes[:, 3])
        w = (xx2 - xx1) + one
        w = np.where(zero >= w, zero, w)
        h = (yy2 - yy1) + one
        h = np.where(zero >= h, zero, h)
        inter = (w * h).astype(F32)
        uni = ((iarea + jarea) - inter).astype(F32)
        ovr = (inter / uni).astype(F32)
    return ovr, uni


def soft_nms(dets, method='linear', thresh=0.3, sigma=0.5, min_score=0.001):
    """dets [n,5] float32 -> (order [m] row indices in emission order, scores [m] float32 as emitted)"""
    assert method in METHODS
    dets = np.ascontiguousarray(dets, F32).reshape(-1, 5)
    boxes, s = dets[:, :4], dets[:, 4].copy()
    lo, sg = F32(min_score), F32(sigma)
    with np.errstate(invalid='ignore'):
        alive = ~np.isnan(s) & ~(s < lo)
    order, out = [], []
    while alive.any():
        idx = np.flatnonzero(alive)
        top = s[idx].max()
        i = int(idx[s[idx] == top][-1])                     # -0.0 == +0.0; the highest row index among the equal
        order.append(i); out.append(s[i])
        alive[i] = False
        idx = np.flatnonzero(alive)
        if not len(idx):
            break
        ovr, uni = overlaps(boxes[i], boxes[idx])
        if (uni == 0).any():
            raise ZeroDivisionError("float division")
        with np.errstate(all='ignore'):
            if method == 'linear':
                hit = ovr.astype(np.float64) >= thresh      # (False for a NaN ovr)
                new = (s[idx] * (F32(1.0) - ovr)).astype(F32)
            else:
                hit = ~np.isnan(ovr)
                new = (s[idx] * g(-(ovr * ovr) / sg)).astype(F32)
            s[idx] = np.where(hit, new, s[idx])
            alive[idx] = ~np.isnan(s[idx]) & ~(s[idx] < lo)
    return np.array(order, np.int64), np.array(out, F32)


def expected(tracks, ntracks, score, tboxes=None, still=None, method='linear', thresh=0.3, sigma=0.5, min_score=0.001,
             top_still=None, R=None):
    """Every list's rows through soft_nms, written into the rank layout (test_nms_tracks_cpu.expected's, plus score0).
    ZeroDivisionError where soft_nms raises it.  Rows past R are dropped, cnt is the full count."""
    C, T, F = tracks.shape[:3]
    if R is None:
        ts = 0 if still is None else (min(still[2].shape[2], 1024 - T) if top_still is None else top_still)
        R = max(ts + T, 1)
    out = dict(tracks=np.full((C, R, F, 5), np.nan, F32), score=np.full((C, R, F), np.nan), score0=np.full((C, R, F), np.nan),
               src=np.full((C, R, F), SRC_PAD, np.int32), cnt=np.zeros((C, F), np.int32), ntracks=np.zeros(C, np.int32))
    for c in range(C):
        for f in range(F):
            dets, s64, src = list_rows(c, f, tracks, ntracks, score, tboxes, still, top_still)
            order, s = soft_nms(dets, method, thresh, sigma, min_score)
            out['cnt'][c, f] = len(order)
            for r, i in enumerate(order[:R]):
                out['tracks'][c, r, f, :4], out['tracks'][c, r, f, 4] = dets[i, :4], s[r]
                out['score'][c, r, f], out['score0'][c, r, f], out['src'][c, r, f] = np.float64(s[r]), s64[i], src[i]
            out['ntracks'][c] = max(out['ntracks'][c], min(len(order), R))
    return out
