"""The rule of multi-context suppression in numpy: sort-based, no device, no torch.  The device calls
``ops.context_classes`` / ``ops.suppress_context`` are pinned to it on bits.

For a video of scores [F,B,C] (class innermost):
  1. a score is a candidate if it is not NaN and -- with ``score_thresh`` -- is > float32(score_thresh); n = their count
  2. k = min(top, n) with ``top``; else max(1, floor(float64(ratio) * float64(n))) clamped to n
  3. thresh = the k-th largest candidate by float order (-0.0 == +0.0, returned as +0.0); +inf when n == 0
  4. hits[c] = candidates of class c with score >= thresh (every tie counts); all zero when n == 0
  5. high[c] = hits[c] >= min_hits
Suppression: out = scores - float32(penalty) where the frame's video has high[c] == False and the score is not NaN; every
other element is copied bit for bit.
"""
import numpy as np


def rank(n, ratio=0.0003, top=None):
    """k of step 2 (0 when n == 0)."""
    n = int(n)
    if n == 0:
        return 0
    if top is not None:
        return min(int(top), n)
    return min(n, max(1, int(np.floor(np.float64(ratio) * np.float64(n)))))


def _videos(F, frame_off):
    if frame_off is None:
        return [(0, F)]
    off = [int(x) for x in frame_off]
    return list(zip(off[:-1], off[1:]))


def context_classes_one(scores, ratio=0.0003, top=None, min_hits=1, score_thresh=None):
    """One video: (thresh f32, n int, hits int32 [C], high bool [C])."""
    s = np.asarray(scores, dtype=np.float32)
    C = s.shape[-1]
    flat = s.reshape(-1, C)
    cand = ~np.isnan(flat)
    if score_thresh is not None:
        with np.errstate(invalid='ignore'):
            cand &= flat > np.float32(score_thresh)
    n = int(cand.sum())
    if n == 0:
        return np.float32(np.inf), 0, np.zeros(C, np.int32), np.zeros(C, bool)
    k = rank(n, ratio, top)
    vals = np.sort(flat[cand])                   # ascending float order; -0.0 and +0.0 compare equal
    t = np.float32(vals[n - k])
    if t == 0:
        t = np.float32(0.0)
    with np.errstate(invalid='ignore'):
        hits = (cand & (flat >= t)).sum(axis=0).astype(np.int32)
    return t, n, hits, hits >= min_hits


def context_classes(scores, ratio=0.0003, top=None, min_hits=1, score_thresh=None, frame_off=None):
    """(thresh [V] f32, n [V] int64, hits [V,C] int32, high [V,C] bool); without frame_off the V axis is dropped."""
    s = np.asarray(scores, dtype=np.float32)
    res = [context_classes_one(s[a:b], ratio, top, min_hits, score_thresh) for a, b in _videos(s.shape[0], frame_off)]
    t = np.array([r[0] for r in res], np.float32)
    n = np.array([r[1] for r in res], np.int64)
    hits = np.stack([r[2] for r in res])
    high = np.stack([r[3] for r in res])
    if frame_off is None:
        return t[0], n[0], hits[0], high[0]
    return t, n, hits, high


def suppress_context(scores, high, penalty=0.4, frame_off=None):
    s = np.asarray(scores, dtype=np.float32)
    high = np.asarray(high, dtype=bool)
    if frame_off is None:
        high = high[None]
    out = s.copy()
    p = np.float32(penalty)
    for v, (a, b) in enumerate(_videos(s.shape[0], frame_off)):
        blk = s[a:b]
        low = ~high[v][None, None, :] & ~np.isnan(blk)
        with np.errstate(invalid='ignore', over='ignore'):
            sub = (blk - p).astype(np.float32)
        out[a:b] = np.where(low, sub, blk)
    # np.where copies bits; make sure of it for the NaN payloads
    keep = np.isnan(s)
    out.view(np.uint32)[keep] = s.view(np.uint32)[keep]
    return out
