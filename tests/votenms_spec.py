"""THE rule of ops.vote_nms_tracks (csrc/votenms_kernels.hpp, include/vdet_hip.h: vdet_vote_nms_tracks) in numpy.

Bounding-box voting (Gidaris & Komodakis, ICCV 2015) of one (class, frame) list.  The rows are nms_tracks' rows in its order
(test_nms_tracks_cpu.list_rows).
  1. KEPT ROWS: oracle.nms(dets, thresh) -- the kept rows, their order, and its ZeroDivisionError.
  2. VOTERS of the kept row i: i itself, untested, and every other row j of the list (suppressed or kept) with uni != 0 and
     (double)ovr >= vote_thresh, (ovr, uni) = softnms_spec.overlaps with i as box i.  A NaN ovr or a zero union is no voter and
     raises nothing.
  3. WEIGHTS: 'score' (double)s_j if s_j > 0 else 0.0, s_j the row's f32 score; 'uniform' 1.0.
  4. SUMS: sw and the four sx_k in float64, sequentially over the voters in ascending row index, starting from 0.0:
     sw += w_j; sx_k += w_j * (double)box_j[k].  Written with np.cumsum over [0.0, terms...]: cumsum adds one element after the
     other, so the bits are the loop's (test_votenms_cpu checks it against the loop).
  5. RESULT: if sw > 0 and all four sx_k / sw are finite, the box is (float)(sx_k / sw); otherwise the row keeps its own box.
With vote_thresh > 1 only i votes, w * x is exact in float64 and (w * x) / w == x: the box comes back as it is.  The one value
this does not hold for on bits is a coordinate of -0.0, which 0.0 + w * -0.0 turns into +0.0 -- on the device as here."""
import numpy as np

from softnms_spec import overlaps
from test_nms_tracks_cpu import SRC_PAD, _oracle, list_rows

F32 = np.float32
WEIGHTS = ('score', 'uniform')
DEFAULTS = dict(thresh=0.5, vote_thresh=0.5, weights='score')


def voters(dets, i, vote_thresh):
    """the voters of row i, ascending"""
    ovr, uni = overlaps(dets[i, :4], dets[:, :4])
    with np.errstate(invalid='ignore'):
        v = (uni != 0) & (ovr.astype(np.float64) >= vote_thresh)         # (False for a NaN ovr)
    v[i] = True
    return np.flatnonzero(v)


def weights_of(dets, weights):
    assert weights in WEIGHTS
    s = dets[:, 4]
    return np.where(s > 0, s.astype(np.float64), 0.0) if weights == 'score' else np.ones(len(dets))


def vote(dets, keep, vote_thresh=0.5, weights='score'):
    """dets [n,5] float32, keep = the kept rows in rank order -> (voted boxes [m,4] float32, votes [m] int32)"""
    dets = np.ascontiguousarray(dets, F32).reshape(-1, 5)
    w, b64 = weights_of(dets, weights), dets[:, :4].astype(np.float64)
    voted, votes = dets[list(keep), :4].copy(), np.zeros(len(keep), np.int32)
    for r, i in enumerate(keep):
        idx = voters(dets, i, vote_thresh)
        votes[r] = len(idx)
        with np.errstate(all='ignore'):
            sw = np.cumsum(np.concatenate([[0.0], w[idx]]))[-1]
            sx = np.cumsum(np.concatenate([np.zeros((1, 4)), w[idx, None] * b64[idx]]), axis=0)[-1]
            if sw > 0:
                q = sx / sw
                if np.isfinite(q).all():
                    voted[r] = q.astype(F32)
    return voted, votes


def expected(tracks, ntracks, score, tboxes=None, still=None, thresh=0.5, top_still=None, R=None, vote_thresh=0.5, weights='score'):
    """Every list's rows through oracle.nms and vote, written into the rank layout (test_nms_tracks_cpu.expected's, plus box0
    and votes).  ZeroDivisionError where oracle.nms raises it.  Rows past R are dropped, cnt is the full count."""
    o = _oracle()
    C, T, F = tracks.shape[:3]
    if R is None:
        ts = 0 if still is None else (min(still[2].shape[2], 1024 - T) if top_still is None else top_still)
        R = max(ts + T, 1)
    out = dict(tracks=np.full((C, R, F, 5), np.nan, F32), score=np.full((C, R, F), np.nan), src=np.full((C, R, F), SRC_PAD, np.int32),
               cnt=np.zeros((C, F), np.int32), ntracks=np.zeros(C, np.int32), box0=np.full((C, R, F, 4), np.nan, F32),
               votes=np.zeros((C, R, F), np.int32))
    for c in range(C):
        for f in range(F):
            dets, s64, src = list_rows(c, f, tracks, ntracks, score, tboxes, still, top_still)
            keep = list(o.nms(dets, thresh))
            out['cnt'][c, f] = len(keep)
            out['ntracks'][c] = max(out['ntracks'][c], min(len(keep), R))
            keep = keep[:R]
            n = len(keep)
            if n:
                voted, votes = vote(dets, keep, vote_thresh, weights)
                out['tracks'][c, :n, f, :4], out['tracks'][c, :n, f, 4] = voted, dets[keep, 4]
                out['score'][c, :n, f], out['src'][c, :n, f] = s64[keep], src[keep]
                out['box0'][c, :n, f], out['votes'][c, :n, f] = dets[keep, :4], votes
    return out
