"""The inputs of the tubelet-NMS tests (tests/tubenms_spec.py is the rule): random tubelet sets whose slots REPEAT a few
objects, the hand-worked pairs, the planted set, and the shape lists with the reason for every size.  All small: a case and
its expected result take well under a second."""
import functools

import numpy as np

F32 = np.float32
CHUNK = 32          # csrc/tubenms_kernels.hpp: kTubeFC, the frames a workgroup stages at a time
TILE = 32           # ... kTubeTile, the slots per side of a pair tile = the bits of one word of a bit row

# T: one slot, one pair, the word edge of the bit rows (31 / 32 / 33), two and three tiles per side (64 / 65), the limit
T_SIZES = (1, 2, 31, 32, 33, 64, 65, 256)
# F: one frame, two, one below / at / above the chunk, more than three chunks
F_SIZES = (1, 2, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 4)


def linear_box(rng, F, size_lo=20, size_hi=120, frac=False):
    """[F,4]: a box on a linear path"""
    x0, y0 = rng.uniform(0, 400, 2)
    w, h = rng.uniform(size_lo, size_hi, 2)
    v = rng.uniform(-3, 3, 2)
    f = np.arange(F)
    b = np.stack([x0 + v[0] * f, y0 + v[1] * f, x0 + v[0] * f + w, y0 + v[1] * f + h], 1)
    return b if frac else np.rint(b)


@functools.lru_cache(maxsize=None)
def random_set(seed, C, T, F, nser=2, tboxes=True, objects=3):
    """A set of C classes whose slots are jittered copies of a few objects per class over random temporal extents.
    Slot kinds by t % 8: 0..3 a copy with its own extent, 4 a copy with holes, 5 a copy with ONE box, 6 all-NaN (an empty slot
    below ntracks), 7 disjoint in time from the slot before it where F allows.  ntracks by class: T, above T (clamped), below the
    live slots with finite garbage behind the count, 0.  Returns a dict of numpy arrays: tracks, ntracks, anchors, series (a
    tuple), tboxes (or None), score3 [C,T,F] f64 (NaN on a few existing boxes), score2 [C,T] f64."""
    rng = np.random.RandomState(seed)
    tracks = np.full((C, T, F, 5), np.nan, F32)
    tb = np.full((C, T, F, 4), np.nan, F32) if tboxes else None
    for c in range(C):
        objs = [linear_box(rng, F, frac=(c % 2 == 1)) for _ in range(objects)]
        for t in range(T):
            kind = t % 8
            if kind == 6:
                continue
            b = objs[rng.randint(objects)] + rng.uniform(-4, 4, (F, 4)) * (1 if c % 2 else 0) + np.rint(rng.uniform(-4, 4, (1, 4)))
            lo = rng.randint(0, max(F // 2, 1))
            hi = rng.randint(lo, F)
            if kind == 7 and F >= 4:
                lo, hi = F - F // 4, F - 1
            elif kind == 3 and F >= 4:
                lo, hi = 0, F // 4
            ex = np.zeros(F, bool)
            ex[lo:hi + 1] = True
            if kind == 4:
                ex &= rng.rand(F) > 0.4
            if kind == 5:
                ex[:] = False
                ex[rng.randint(F)] = True
            tracks[c, t, ex, :4] = b[ex]
            tracks[c, t, ex, 4] = rng.rand(int(ex.sum()))
            if tboxes:
                tb[c, t, ex] = b[ex] + rng.uniform(-2, 2, (int(ex.sum()), 4))
    ntracks = np.array([(T, T + 3, max(T // 2, 1), 0)[c % 4] for c in range(C)], np.int32)
    for c in range(C):                      # finite garbage behind the count: never read
        n = min(max(int(ntracks[c]), 0), T)
        tracks[c, n:] = rng.uniform(0, 300, tracks[c, n:].shape)
        if tboxes:
            tb[c, n:] = rng.uniform(0, 300, tb[c, n:].shape)
    ex = ~np.isnan(tracks[..., 0])
    score3 = np.where(ex, rng.randn(C, T, F), np.nan)
    score3[ex & (rng.rand(C, T, F) < 0.1)] = np.nan             # an existing box whose score is NaN: not part of the mean
    score3[:, ::5] = np.round(score3[:, ::5], 1)                # ties between tubelet scores become likely at small F
    score2 = rng.randn(C, T)
    if T >= 4:
        score2[:, 1], score2[:, 2] = score2[:, 0], np.nan       # a tie, and an absent tubelet by its score
    anchors = rng.rand(C, T, 3).astype(F32)
    series = tuple(np.where(ex, rng.randn(C, T, F), np.nan) for _ in range(nser))
    return dict(tracks=tracks, ntracks=ntracks, anchors=anchors, series=series, tboxes=tb, score3=score3, score2=score2)


def blank(C, T, F):
    """(tracks all NaN, ntracks = T)"""
    return np.full((C, T, F, 5), np.nan, F32), np.full(C, T, np.int32)


def put(tracks, c, t, frames, box, score=1.0):
    for f in frames:
        tracks[c, t, f] = list(box) + [score]


def exotic_set():
    """One class, 12 slots over 3 frames: NaN, inf, inverted and zero-size boxes, coordinates up to 65535 and fractional ones.
    Every slot exists on every frame (column 0 is never NaN here except where noted): the odd boxes give no contribution, and no
    error."""
    T, F = 12, 3
    tracks, ntracks = blank(1, T, F)
    big = [65000.0, 65100.0, 65535.0, 65535.0]
    rows = [
        [10, 10, 50, 50], [10, 10, 50, 50],                     # 0, 1: identical
        [10, np.nan, 50, 50],                                   # 2: a NaN coordinate behind column 0
        [10, 10, np.inf, 50],                                   # 3: an infinite side
        [-np.inf, 10, np.inf, 50],                              # 4: inf - (-inf)
        [50, 50, 10, 10],                                       # 5: inverted in both axes (a positive "area")
        [30, 30, 29, 29],                                       # 6: zero size ((29 - 30) + 1 = 0)
        [30, 30, 29, 40],                                       # 7: zero width
        big, [65001.5, 65100.25, 65535.0, 65534.75],            # 8, 9: large and fractional
        [10.5, 10.25, 50.125, 49.875],                          # 10: fractional, on top of 0 / 1
        [0, 0, 3.4e38, 3.4e38],                                 # 11: an area that overflows to inf
    ]
    for t, r in enumerate(rows):
        put(tracks, 0, t, range(F), r, score=0.5)
    score = np.linspace(1.0, 2.0, T)[None, :].copy()
    return tracks, ntracks, score


def score_edge_set():
    """One class, 10 identical, fully overlapping tubelets... apart from their scores: NaN, +/-0.0, ties, infinities.  With
    thresh > 1 the result is the order alone."""
    T, F = 10, 2
    tracks, ntracks = blank(1, T, F)
    for t in range(T):
        put(tracks, 0, t, range(F), [5 * t, 5 * t, 5 * t + 40, 5 * t + 40])
    score = np.array([[0.0, -0.0, np.nan, 1.5, 1.5, -np.inf, np.inf, -0.0, 0.0, 1.5]])
    return tracks, ntracks, score


def knife_pair():
    """Two tubelets with identical boxes on 1 of their 2 union frames: S = 2^24, den = 2, ovr == 0.5 exactly."""
    tracks, ntracks = blank(1, 2, 2)
    put(tracks, 0, 0, (0, 1), [10, 10, 50, 50])
    put(tracks, 0, 1, (0,), [10, 10, 50, 50])
    return tracks, ntracks, np.array([[2.0, 1.0]])


def contained_pair(F=8, short=2):
    """A long tubelet and a short one inside it, identical boxes where both exist: 'min' gives 1.0, 'union' short / F."""
    tracks, ntracks = blank(1, 2, F)
    put(tracks, 0, 0, range(F), [10, 10, 50, 50])
    put(tracks, 0, 1, range(3, 3 + short), [10, 10, 50, 50])
    return tracks, ntracks, np.array([[2.0, 1.0]])


@functools.lru_cache(maxsize=None)
def planted_set(seed=7, K=3, N=4, clutter=5, F=24, jitter=2.0):
    """K objects on linear paths, each copied N times with box jitter (uniform in +/-jitter px per coordinate and frame) and
    different temporal extents (every copy covers at least the middle half), plus ``clutter`` short random tubelets elsewhere.
    Objects are 60 to 120 px wide and start >= 250 px apart, so copies of one object overlap far above 0.5 and different
    objects not at all.  Returns (tracks [1,T,F,5], ntracks, score [1,T], object of every slot (-1 clutter))."""
    rng = np.random.RandomState(seed)
    T = K * N + clutter
    tracks, ntracks = blank(1, T, F)
    owner = np.full(T, -1)
    slots = rng.permutation(T)
    f = np.arange(F)
    for k in range(K):
        w, h = rng.uniform(60, 120, 2)
        x0, y0 = 250.0 * k, 250.0 * k
        v = rng.uniform(-2, 2, 2)
        path = np.stack([x0 + v[0] * f, y0 + v[1] * f, x0 + v[0] * f + w, y0 + v[1] * f + h], 1)
        for i in range(N):
            t = slots[k * N + i]
            lo, hi = rng.randint(0, F // 4 + 1), rng.randint(3 * F // 4, F)
            tracks[0, t, lo:hi + 1, :4] = path[lo:hi + 1] + rng.uniform(-jitter, jitter, (hi + 1 - lo, 4))
            tracks[0, t, lo:hi + 1, 4] = 1.0
            owner[t] = k
    for i in range(clutter):
        t = slots[K * N + i]
        lo = rng.randint(0, F - 3)
        x0, y0 = 1000 + 200.0 * i, rng.uniform(0, 100)
        tracks[0, t, lo:lo + 3, :4] = [x0, y0, x0 + 30, y0 + 30]
        tracks[0, t, lo:lo + 3, 4] = 1.0
    score = rng.permutation(T).astype(np.float64)[None, :]
    score[0, owner < 0] -= 100.0                                 # clutter scores below every object copy
    return tracks, ntracks, score, owner


@functools.lru_cache(maxsize=None)
def planted_video(seed=11, F=12, K=3, B=12, C=2):
    """boxes [F,B,4] / scores [F,B,C] f32: K objects per class on linear paths (box k of every frame, drifting 2 px a frame,
    scores near 1 and all different, highest on every fourth frame), the other boxes low-scored clutter.  top_anchors(3K)
    therefore picks three anchors on every object, and the anchor route tracks it three times: whether a tubelet runs through
    the whole video or from its anchor on, the copies of an object are nested in time with identical boxes ('min' gives 1.0)."""
    rng = np.random.RandomState(seed)
    boxes = np.zeros((F, B, 4), F32)
    for b in range(B):
        x0, y0 = (300.0 * b, 50.0) if b < K else (rng.uniform(0, 800), rng.uniform(400, 800))
        w, h = (80.0, 60.0) if b < K else tuple(rng.uniform(10, 30, 2))
        for f in range(F):
            d = 2.0 * f if b < K else float(rng.uniform(-200, 200))
            boxes[f, b] = [x0 + d, y0 + d, x0 + d + w, y0 + d + h]
    scores = (rng.permutation(F * B * C).reshape(F, B, C) / float(F * B * C) * 0.1).astype(F32)
    scores[:, :K, :] += F32(0.7)
    scores[::4, :K, :] += F32(0.1)          # the first anchors of a class: every object on frames 0, 4, 8, ...
    return boxes, scores
