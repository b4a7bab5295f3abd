"""THE rule of ops.nms_tubelets (csrc/tubenms_kernels.hpp, include/vdet_hip.h: vdet_nms_tubelets) in numpy.

NMS over whole tubelets of one class by spatio-temporal overlap.  The reference has no such function; the rule is the project's.
  A box exists at (c,t,f) iff t < ntracks[c] (clamped to 0..T) and tracks[c,t,f,0] is not NaN; tboxes, when given, are the boxes.
  1. ts[t] (f64): a [C,T] score as given; for a [C,T,F] score the 'mean' (the f64 sum in ASCENDING frame order from 0.0, over
     the frames where the box exists and the value is not NaN, divided by their count) or the 'max' over the same frames (+0.0
     between -0.0 and +0.0); NaN without such a frame.  A tubelet with no box or a NaN ts is ABSENT.
  2. per shared frame of tubelets a <= b: q = softnms_spec.overlaps (f32, a as box i); iff 0 < q <= FLT_MAX the frame gives
     k = rint(q * 2^24) (product in f32, saturated at 2^32 - 1), else 0.
  3. S = sum of k (an integer: no order), I = shared frames, n[t] = boxes.
  4. den = n[a] + n[b] - I ('union'), I ('shared'), min(n[a], n[b]) ('min'); ovr = 0.0 if den == 0 or I < min_shared, else
     float(S) / (float(den) * 16777216.0).
  5. the present tubelets by descending ts (-0.0 == +0.0, ties by DESCENDING slot), walked greedily with ovr >= thresh.
  6. the kept tubelets compacted into rank order (``expected``)."""
import numpy as np

from softnms_spec import overlaps

F32 = np.float32
NORMS = ('union', 'shared', 'min')
REDUCES = ('mean', 'max')
SRC_PAD = np.iinfo(np.int32).min
SCALE = F32(16777216.0)
FLT_MAX = np.finfo(np.float32).max


def counts(ntracks, T):
    return np.clip(np.asarray(ntracks, np.int64), 0, T)


def exists(tracks, ntracks):
    """[C,T,F] bool"""
    C, T, F = tracks.shape[:3]
    live = np.arange(T)[None, :] < counts(ntracks, T)[:, None]
    return live[:, :, None] & ~np.isnan(tracks[..., 0])


def tubelet_scores(tracks, ntracks, score, reduce='mean'):
    """ts [C,T] f64, NaN for an absent tubelet"""
    C, T, F = tracks.shape[:3]
    ex = exists(tracks, ntracks)
    score = np.asarray(score)
    ts = np.full((C, T), np.nan)
    for c in range(C):
        for t in range(T):
            if not ex[c, t].any():
                continue
            if score.ndim == 2:
                ts[c, t] = np.float64(score[c, t])
                continue
            vals = [np.float64(score[c, t, f]) for f in range(F) if ex[c, t, f] and not np.isnan(score[c, t, f])]
            if not vals:
                continue
            if reduce == 'mean':
                s = np.float64(0.0)
                for x in vals:
                    s = s + x
                ts[c, t] = s / np.float64(len(vals))
            else:
                m = max(vals)
                if m == 0.0:        # the sign of a zero maximum must not depend on the order of the frames
                    m = np.float64(0.0) if any(x == 0.0 and not np.signbit(x) for x in vals) else np.float64(-0.0)
                ts[c, t] = m
    return ts


def quantise(q):
    """k [m] uint64 of f32 quotients q [m]"""
    with np.errstate(all='ignore'):
        ok = (q > 0) & (q <= FLT_MAX)
        r = np.rint((np.where(ok, q, F32(0.0)) * SCALE).astype(F32)).astype(np.float64)
    return np.where(r >= 4294967296.0, 4294967295.0, r).astype(np.uint64)


def pair_sums(boxes, ex):
    """One class: boxes [T,F,4] f32, ex [T,F] bool -> (S [T,T] uint64, I [T,T] int64, n [T] int64), symmetric"""
    T = ex.shape[0]
    S, I = np.zeros((T, T), np.uint64), np.zeros((T, T), np.int64)
    for f in np.flatnonzero(ex.any(axis=0)):
        idx = np.flatnonzero(ex[:, f])
        for p, a in enumerate(idx):
            rest = idx[p:]                      # (a itself: the diagonal follows the same rule)
            q, _ = overlaps(boxes[a, f], boxes[rest, f])
            S[a, rest] += quantise(q)
            I[a, rest] += 1
    up = np.triu(np.ones((T, T), bool), 1)
    S = np.where(up.T, S.T, S)
    I = np.where(up.T, I.T, I)
    return S, I, ex.sum(axis=1).astype(np.int64)


def tube_overlaps(S, I, n, norm='union', min_shared=1):
    """ovr [T,T] f64 of every pair (no notion of absent here)"""
    if norm == 'union':
        den = n[:, None] + n[None, :] - I
    elif norm == 'shared':
        den = I
    else:
        den = np.minimum(n[:, None], n[None, :])
    zero = (den == 0) | (I < min_shared)
    with np.errstate(all='ignore'):
        ovr = S.astype(np.float64) / (np.where(zero, 1, den).astype(np.float64) * 16777216.0)
    return np.where(zero, 0.0, ovr)


def order_of(ts):
    """the present slots by descending ts, -0.0 == +0.0, equal scores by descending slot"""
    idx = [t for t in range(len(ts)) if not np.isnan(ts[t])]
    out = []
    while idx:                                   # selection by maximum: the definition, no sort's tie rule involved
        top = max(ts[t] for t in idx)
        t = max(u for u in idx if ts[u] == top)
        out.append(t)
        idx.remove(t)
    return out


def select(ts, ovr, thresh):
    """One class -> (kept slots in rank order, by [T])"""
    T = len(ts)
    by = np.full(T, -1, np.int32)
    kept = []
    for t in order_of(ts):
        if by[t] >= 0:
            continue
        by[t] = t
        kept.append(t)
        for u in range(T):
            if by[u] < 0 and not np.isnan(ts[u]) and ovr[t, u] >= thresh:
                by[u] = t
    return kept, by


def expected(tracks, ntracks, score, tboxes=None, anchors=None, series=(), thresh=0.5, norm='union', reduce='mean', min_shared=1):
    """Everything ops.nms_tubelets returns, as numpy (``overlaps`` always)."""
    assert norm in NORMS and reduce in REDUCES
    C, T, F = tracks.shape[:3]
    ex = exists(tracks, ntracks)
    ts = tubelet_scores(tracks, ntracks, score, reduce)
    boxes = tracks[..., :4] if tboxes is None else tboxes
    out = dict(tracks=np.full((C, T, F, 5), np.nan, F32), ntracks=np.zeros(C, np.int32), src=np.full((C, T), SRC_PAD, np.int32),
               tscore=np.full((C, T), np.nan), by=np.full((C, T), -1, np.int32), overlaps=np.full((C, T, T), np.nan),
               series=tuple(np.full((C, T, F), np.nan) for _ in series))
    if tboxes is not None:
        out['tboxes'] = np.full((C, T, F, 4), np.nan, F32)
    if anchors is not None:
        out['anchors'] = np.zeros((C, T, 3), F32)
    for c in range(C):
        S, I, n = pair_sums(np.ascontiguousarray(boxes[c], F32), ex[c])
        ovr = tube_overlaps(S, I, n, norm, min_shared)
        present = ~np.isnan(ts[c])
        out['overlaps'][c] = np.where(present[:, None] & present[None, :], ovr, np.nan)
        kept, by = select(ts[c], ovr, thresh)
        out['by'][c], out['ntracks'][c] = by, len(kept)
        for r, t in enumerate(kept):
            out['src'][c, r], out['tscore'][c, r] = t, ts[c, t]
            out['tracks'][c, r] = tracks[c, t]
            if tboxes is not None:
                out['tboxes'][c, r] = tboxes[c, t]
            if anchors is not None:
                out['anchors'][c, r] = anchors[c, t]
            for x, y in zip(out['series'], series):
                x[c, r] = y[c, t]
    return out
