"""Seq-NMS (Han et al. 2016) in numpy: THE rule ops.seq_nms / ops.seq_nms_batch are pinned to on bits (no GPU, no product code).

One class of one video at a time: tracks [R,F,5] f32 (x1, y1, x2, y2, score), ntracks, an optional score [R,F] f32 / f64.
  node      row (r, f) with r < ntracks (clamped to 0..R), tracks[r,f,0] not NaN and a finite score (score[r,f] when a score
            tensor is given, else tracks[r,f,4]; taken as f64, which is exact).
  hit       hit(a, b, t): the f32 arithmetic of utils/nms.pyx:57-65, every operation rounded to f32 (knife_spec.quotient has the
            same operation order); true iff uni > 0 and (double)(inter / uni) >= t.  A zero, negative or NaN union is false.
  link      node (q, f) -> node (r, f+1) iff hit(box[q,f], box[r,f+1], link_thres).
  round k   over the live nodes, frames ascending: best[r,f] = s[r,f] + b, b the largest best[q,f-1] among the live q that link
            to (r,f) and have best[q,f-1] >= 0 (ptr = the lowest such q that attains it); with none best = s exactly, ptr = -1.
            The end node is the live node with the largest best (ties: lowest frame, then lowest slot).  The rounds stop when
            no node is live, or best_end < min_score, or k == max_seqs.  The path is ptr followed back from the end node;
            best_end is its left-to-right f64 sum.  New score of the path's nodes: 'avg' best_end / len (one f64 division),
            'max' the largest s on the path (folded left to right with m = s if s > m else m, so of -0.0 and +0.0 the earlier
            stays).  Every other live node (q,f) of a path node's frame with hit(box[r,f], box[q,f], nms_thres) is suppressed;
            path nodes become members of sequence k; both leave the live set.
  leftover  a node still live after the rounds; it keeps its score.

Frames before the first one the last sequence touched keep their best / ptr (their live sets did not change and the pass
only looks back), so a round restarts there: the same numbers, fewer of them computed.
"""
import numpy as np

F32, F64 = np.float32, np.float64
NO_NODE = np.iinfo(np.int32).min
LEFTOVER, SUPPRESSED = -1, -2
RESCORE = ('avg', 'max')


def hit_matrix(a, b, t):
    """hit(a[i], b[j], t) for a [..., n, 4], b [..., m, 4] -> bool [..., n, m]."""
    a = np.asarray(a, F32)[..., :, None, :]
    b = np.asarray(b, F32)[..., None, :, :]
    one, zero = F32(1), F32(0)
    with np.errstate(all='ignore'):
        xx1 = np.where(a[..., 0] >= b[..., 0], a[..., 0], b[..., 0])
        yy1 = np.where(a[..., 1] >= b[..., 1], a[..., 1], b[..., 1])
        xx2 = np.where(a[..., 2] <= b[..., 2], a[..., 2], b[..., 2])
        yy2 = np.where(a[..., 3] <= b[..., 3], a[..., 3], b[..., 3])
        w = (xx2 - xx1) + one
        w = np.where(zero >= w, zero, w)
        h = (yy2 - yy1) + one
        h = np.where(zero >= h, zero, h)
        inter = w * h
        aa = ((a[..., 2] - a[..., 0]) + one) * ((a[..., 3] - a[..., 1]) + one)
        ab = ((b[..., 2] - b[..., 0]) + one) * ((b[..., 3] - b[..., 1]) + one)
        uni = (aa + ab) - inter
        q = inter / uni
        assert q.dtype == F32
        return (uni > zero) & (q.astype(F64) >= F64(t))


def nodes_of(tracks, ntracks, score=None):
    """(node [R,F] bool, s [R,F] f64, nt) of one class."""
    tracks = np.asarray(tracks, F32)
    R, F = tracks.shape[:2]
    nt = int(min(max(int(ntracks), 0), R))
    if score is None:
        s = tracks[:, :, 4].astype(F64)
    else:
        assert score.dtype in (F32, F64) and score.shape == (R, F)
        s = score.astype(F64)
    node = (np.arange(R)[:, None] < nt) & ~np.isnan(tracks[:, :, 0]) & np.isfinite(s)
    return node, s, nt


def seq_nms(tracks, ntracks, score=None, link_thres=0.5, nms_thres=0.3, rescore='avg', max_seqs=32, min_score=-np.inf):
    """One class.  Returns the dict of outputs (tracks, score, seq, ntracks, nseq, seq_sum, seq_len, seq_end, exhausted)."""
    assert rescore in RESCORE and max_seqs >= 1
    tracks = np.ascontiguousarray(tracks, F32)
    R, F = tracks.shape[:2]
    node, s, nt = nodes_of(tracks, ntracks, score)
    S = int(max_seqs)
    boxes = np.ascontiguousarray(tracks[:, :, :4].transpose(1, 0, 2))               # [F,R,4]
    link = hit_matrix(boxes[:-1], boxes[1:], link_thres) if F > 1 else np.zeros((0, R, R), bool)   # [f][q,r]: (q,f) -> (r,f+1)
    same = hit_matrix(boxes, boxes, nms_thres)                                       # [f][r,q]: a = the path node
    live = node.copy()
    seq = np.where(node, LEFTOVER, NO_NODE).astype(np.int32)
    new = np.where(node, s, np.nan)
    best = np.full((R, F), np.nan)
    mx = np.full((R, F), np.nan)
    ptr = np.full((R, F), -1, np.int64)
    ln = np.zeros((R, F), np.int64)
    seq_sum, seq_len, seq_end = np.full(S, np.nan), np.zeros(S, np.int32), np.full((S, 2), -1, np.int32)
    k, start = 0, 0
    with np.errstate(all='ignore'):
        while live.any() and k < S:
            for f in range(start, F):
                lv, sf = live[:, f], s[:, f]
                has = np.zeros(R, bool)
                if f > 0:
                    ok = link[f - 1] & (live[:, f - 1] & (best[:, f - 1] >= 0))[:, None]          # [q,r]
                    has = ok.any(0)
                    m = np.where(ok, best[:, f - 1][:, None], -np.inf)
                    p = m.argmax(0)                          # the first (lowest) q that attains the largest
                    b, pm, pl = best[p, f - 1], mx[p, f - 1], ln[p, f - 1]
                    ext = lv & has
                    best[:, f] = np.where(lv, np.where(has, sf + b, sf), np.nan)
                    mx[:, f] = np.where(ext, np.where(sf > pm, sf, pm), sf)
                    ptr[:, f] = np.where(ext, p, -1)
                    ln[:, f] = np.where(ext, pl + 1, 1)
                else:
                    best[:, f] = np.where(lv, sf, np.nan)
                    mx[:, f], ptr[:, f], ln[:, f] = sf, -1, 1
            top = np.where(live, best, -np.inf).max()
            if top < min_score:
                break
            at = live & (best == top)
            fe = int(at.any(0).argmax())
            re = int(at[:, fe].argmax())
            top = best[re, fe]                               # the end node's own sum (-0.0 == +0.0 in the comparison above)
            n = int(ln[re, fe])
            val = top / F64(n) if rescore == 'avg' else mx[re, fe]
            seq_sum[k], seq_len[k], seq_end[k] = top, n, (fe, re)
            r, f = re, fe
            while True:
                gone = same[f][r] & live[:, f]
                gone[r] = False
                seq[gone, f], new[gone, f] = SUPPRESSED, np.nan
                seq[r, f], new[r, f] = k, val
                live[gone, f] = False
                live[r, f] = False
                if ptr[r, f] < 0:
                    break
                r, f = int(ptr[r, f]), f - 1
            assert fe - f + 1 == n
            start = f
            k += 1
    out = np.full((R, F, 5), np.nan, F32)
    keep = seq >= LEFTOVER
    out[keep, :4] = tracks[keep, :4]
    out[keep, 4] = new[keep].astype(F32)
    return dict(tracks=out, score=new, seq=seq, ntracks=np.int32(nt), nseq=np.int32(k), seq_sum=seq_sum, seq_len=seq_len,
                seq_end=seq_end, exhausted=np.uint8(not live.any()))


KEYS = ('tracks', 'score', 'seq', 'ntracks', 'nseq', 'seq_sum', 'seq_len', 'seq_end', 'exhausted')


def seq_nms_classes(tracks, ntracks, score=None, **kw):
    """ops.seq_nms in numpy: tracks [C,R,F,5], ntracks [C], score [C,R,F] or None; the outputs with a leading class axis."""
    outs = [seq_nms(tracks[c], ntracks[c], None if score is None else score[c], **kw) for c in range(len(tracks))]
    return {k: np.stack([o[k] for o in outs]) for k in KEYS}


def best_path_brute(tracks, ntracks, score=None, link_thres=0.5):
    """The largest left-to-right f64 sum over ALL linked paths of nodes, by exhaustive enumeration (tiny inputs only)."""
    tracks = np.asarray(tracks, F32)
    R, F = tracks.shape[:2]
    node, s, _ = nodes_of(tracks, ntracks, score)
    boxes = tracks[:, :, :4].transpose(1, 0, 2)
    link = hit_matrix(boxes[:-1], boxes[1:], link_thres) if F > 1 else np.zeros((0, R, R), bool)
    top = [-np.inf]

    def walk(r, f, total):
        top[0] = max(top[0], total)
        if f + 1 < F:
            for q in range(R):
                if node[q, f + 1] and link[f][r, q]:
                    walk(q, f + 1, total + s[q, f + 1])
    for f in range(F):
        for r in range(R):
            if node[r, f]:
                walk(r, f, s[r, f])
    return top[0]
