"""The specification of ops.rescore_tubelets in numpy, and the inputs its tests share (no GPU, no product code).

spec() restates include/vdet_hip.h (vdet_rescore_tubelets) from the oracle's pieces, all of them on the LIST of a tubelet's
present frames as the reference works on its list of box dicts: oracle.spatial_maxpool / oracle.iou per box, the floor rule
of rcnn_sampling_dets_scoring, oracle.score_completion, and the list max-pool of oracle.rescored_tubelets.  The pool is written
centre first (the running value starts at the box's own score and a neighbour replaces it when it compares greater), which is
python's max() of oracle.rescored_tubelets on every NaN-free list and what the header states for lists with a NaN.
"""
import numpy as np

import synth
from oracle import oracle

SENTINEL = -1e5


def spec(tracks, ntracks, boxes, scores, floor=None, overlap_thres=0.7, window=3, complete=None):
    """One video.  Returns (det f64 [C,T,F], pooled f64, tboxes f32 [C,T,F,4], src i32, eindex): eindex says that some tubelet
    had no valid score under completion (its det keeps the sentinels, its pooled stays NaN)."""
    tracks = np.asarray(tracks, np.float32)
    C, T, F = tracks.shape[:3]
    complete = floor is None if complete is None else bool(complete)
    h = window // 2
    det = np.full((C, T, F), np.nan)
    pooled = np.full((C, T, F), np.nan)
    tboxes = np.full((C, T, F, 4), np.nan, np.float32)
    src = np.full((C, T, F), -1, np.int32)
    eindex = False
    for c in range(C):
        for t in range(min(int(ntracks[c]), T)):
            fr = [f for f in range(F) if not np.isnan(tracks[c, t, f, 0])]
            s = []
            for f in fr:
                row = tracks[c, t, f, :4]
                ss, bb, hit = oracle.spatial_maxpool([row], boxes[f], scores[f, :, c], overlap_thres)
                j = -1
                if hit[0]:
                    with np.errstate(all='ignore'):
                        cand = np.flatnonzero(oracle.iou([row], boxes[f]).ravel() > overlap_thres)
                    j = int(cand[np.argmax(scores[f, cand, c])])
                    assert np.array_equal(bb[0], boxes[f, j].astype(np.float64), equal_nan=True)
                    assert np.array_equal(ss[0], np.float64(scores[f, j, c]), equal_nan=True)
                take, val = bool(hit[0]), ss[0]
                if floor is not None:
                    fl = np.float64(floor[c, t, f])
                    take = take and bool(val > fl)
                    if not take:
                        val = fl
                s.append(val)
                tboxes[c, t, f] = bb[0].astype(np.float32) if take else row
                src[c, t, f] = j if take else -1
            det[c, t, fr] = s
            comp = np.asarray(s, np.float64)
            if complete and len(s):
                try:
                    comp = oracle.score_completion(s)
                except IndexError:
                    eindex = True
                    continue
                det[c, t, fr] = comp
            n = len(comp)
            pool = []
            for i in range(n):
                m = comp[i]
                for g in range(i - h, i + h + 1):
                    x = comp[g] if 0 <= g < n else SENTINEL
                    if x > m:
                        m = x
                pool.append(m)
            pooled[c, t, fr] = pool
    return det, pooled, tboxes, src, eindex


def spec_batch(tracks, ntracks, boxes, scores, frame_off, floor=None, **kw):
    """Per-video lists of spec()'s outputs for tubelets in video_batch's layout (tracks / floor: one array per video)."""
    outs, eindex = [], False
    for v in range(len(frame_off) - 1):
        a, b = int(frame_off[v]), int(frame_off[v + 1])
        o = spec(tracks[v], ntracks[v], boxes[a:b], scores[a:b], None if floor is None else floor[v], **kw)
        outs.append(o[:4])
        eindex = eindex or o[4]
    return [list(x) for x in zip(*outs)], eindex


# ---------------------------------------------------------------------------------------------
# the input recipe
# ---------------------------------------------------------------------------------------------
def volume(seed, F, B, C):
    """Proposals drifting 3 px per frame, every odd one its even neighbour + 1 px (two candidates per hit); scores with every
    (4k+1)-th proposal tied to the 4k-th (tied maxima)."""
    rng = np.random.RandomState(seed)
    base = synth.boxes_1(rng, B)
    base[1::2] = base[0:2 * (B // 2):2] + np.float32(1)
    boxes = np.stack([base + np.float32(3 * f) for f in range(F)], 0).astype(np.float32)
    scores = rng.rand(F, B, C).astype(np.float32)
    n = len(range(1, B, 4))
    scores[:, 1::4] = scores[:, 0::4][:, :n]
    return boxes, scores


def tubelets(seed, boxes, C, T):
    """tracks [C,T,F,5] f32 with holes, misses and hits, and a floor [C,T,F] f64.  A tubelet whose every box would miss gets
    its first present box turned into a hit."""
    F, B = boxes.shape[:2]
    k = np.random.RandomState(seed + 1).randint(0, 10, (C, T, F))
    floor = np.random.RandomState(seed + 2).rand(C, T, F)
    tracks = np.full((C, T, F, 5), np.nan, np.float32)
    for c in range(C):
        for t in range(T):
            p = 2 * ((7 * c + 3 * t) % max(B // 2, 1))
            for f in range(F):
                if k[c, t, f] < 2:
                    continue
                tracks[c, t, f, :4] = boxes[f, p] + np.float32(402 if k[c, t, f] < 5 else 2)
                tracks[c, t, f, 4] = 0.5
            present = np.flatnonzero(k[c, t] >= 2)
            if len(present) and not np.any(k[c, t] >= 5):
                tracks[c, t, present[0], :4] = boxes[present[0], p] + np.float32(2)
    return tracks, floor


def planted_floor(tracks, floor):
    """The floor as a scorer that sees only (class, frame, box) can plant it: slots of one class with the same box on a frame
    share the value of the last of them."""
    out = np.array(floor, np.float64)
    C, T, F = tracks.shape[:3]
    for c in range(C):
        for f in range(F):
            d = {}
            for t in range(T):
                if not np.isnan(tracks[c, t, f, 0]):
                    d[tuple(float(x) for x in tracks[c, t, f, :4])] = out[c, t, f]
            for t in range(T):
                if not np.isnan(tracks[c, t, f, 0]):
                    out[c, t, f] = d[tuple(float(x) for x in tracks[c, t, f, :4])]
    return out


def census(tracks, ntracks, boxes, scores, floor, overlap_thres=0.7):
    """What a case exercises (one video): counts of hits, misses, tied maxima, gap kinds, inner holes, floor outcomes."""
    C, T, F = tracks.shape[:3]
    out = dict(hits=0, misses=0, multi=0, tied=0, leading=0, trailing=0, interior=0, inner_hole=0, all_miss=0, det_wins=0,
               floor_wins=0)
    for c in range(C):
        for t in range(min(int(ntracks[c]), T)):
            fr = [f for f in range(F) if not np.isnan(tracks[c, t, f, 0])]
            if not fr:
                continue
            if len(fr) != fr[-1] - fr[0] + 1:
                out['inner_hole'] += 1
            miss = []
            for f in fr:
                cand = np.flatnonzero(oracle.iou([tracks[c, t, f, :4]], boxes[f]).ravel() > overlap_thres)
                miss.append(len(cand) == 0)
                if len(cand) == 0:
                    out['misses'] += 1
                    continue
                out['hits'] += 1
                sc = scores[f, cand, c]
                out['multi'] += len(cand) >= 2
                out['tied'] += int(np.sum(sc == sc.max()) >= 2)
                if sc[np.argmax(sc)] > floor[c, t, f]:
                    out['det_wins'] += 1
                else:
                    out['floor_wins'] += 1
            if all(miss):
                out['all_miss'] += 1
                continue
            i = 0
            while i < len(miss):
                if not miss[i]:
                    i += 1
                    continue
                j = i
                while j < len(miss) and miss[j]:
                    j += 1
                out['leading' if i == 0 else ('trailing' if j == len(miss) else 'interior')] += 1
                i = j
    return out


# B -> the seed of the recipe's checked 9-frame case
PARITY_SEEDS = {5: 9100, 300: 9101, 1100: 9103}


def batch_case(seed, frame_off, B, C=2, T=3):
    """Videos of the given frame ranges, each from the recipe (the LAST video takes `seed`, the one before seed + 10, ...).
    Returns numpy (boxes [F,B,4], scores [F,B,C], tracks per video, ntracks [V,C], floor per video, census summed)."""
    off = [int(x) for x in frame_off]
    V = len(off) - 1
    bx, sc, tr, fl, total = [], [], [], [], None
    for v in range(V):
        s = seed + 10 * (V - 1 - v)
        b, q = volume(s, off[v + 1] - off[v], B, C)
        t, f = tubelets(s, b, C, T)
        cz = census(t, np.full(C, T), b, q, f)
        total = cz if total is None else {k: total[k] + cz[k] for k in cz}
        bx.append(b); sc.append(q); tr.append(t); fl.append(f)
    return np.concatenate(bx), np.concatenate(sc), tr, np.full((V, C), T, np.int32), fl, total


def check_census(cz, frame_off):
    """No parity case passes vacuously.  Gaps and inner holes need a tubelet of several boxes: they are required of every
    case with a video of at least 9 frames; a case of one-frame videos (each tubelet is one box, which the recipe makes a
    hit) can only show hits, ties and the two floor outcomes."""
    assert cz['all_miss'] == 0, cz
    assert cz['hits'] > 0 and cz['tied'] > 0 and cz['det_wins'] > 0 and cz['floor_wins'] > 0, cz
    if max(np.diff(np.asarray(frame_off))) >= 9:
        assert cz['misses'] > 0 and cz['leading'] > 0 and cz['trailing'] > 0 and cz['interior'] > 0 and cz['inner_hole'] > 0, cz


# ---------------------------------------------------------------------------------------------
# the reference's recorded outputs (tests/golden/make_rescore_golden.py)
# ---------------------------------------------------------------------------------------------
def load_golden():
    import gzip
    import json
    import os
    with gzip.open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'rescore_golden.json.gz'), 'rt') as f:
        return json.load(f)['cases']


def golden_inputs(case):
    boxes, scores = volume(case['seed'], case['F'], case['B'], case['C'])
    tracks, floor = tubelets(case['seed'], boxes, case['C'], case['T'])
    return boxes, scores, tracks, planted_floor(tracks, floor)


def golden_arrays(case, part):
    """{field: [C,T,F] f64 (bbox: [C,T,F,4]) with NaN where the reference's tubelet has no box} of 'maxpool' / 'sampling'."""
    C, T, F = case['C'], case['T'], case['F']
    fields = [k for k in case[part][0][0] if k != 'frame']
    out = {k: np.full((C, T, F) + ((4,) if k == 'bbox' else ()), np.nan) for k in fields}
    for c in range(C):
        for t, tub in enumerate(case[part][c]):
            fr = [f - 1 for f in tub['frame']]
            for k in fields:
                out[k][c, t, fr] = np.asarray(tub[k], np.float64).reshape((len(fr),) + out[k].shape[3:])
    return out
