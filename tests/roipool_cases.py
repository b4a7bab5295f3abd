"""The case list of RoI pooling, shared by tests/test_roipool_cpu.py (spec against its loop transcription) and
tests/test_roipool_gpu.py (device against the spec).  A case is a dict: name, feat float32 [Fi,K,Hf,Wf], boxes [N,4] (f64 unless
the name says f32), idx int32 [N] or None, scale, pooled, box_scale, kind ('geometry' / 'value' / 'shape' / 'align').

The geometry cases share ONE feature tensor [2,3,64,64] drawn as normal - 2: most cells are negative, so the 0 of an empty bin
differs from any maximum.  At scale 1/16 the map is 1024 x 1024 pixels."""
import functools

import numpy as np

FLT_MAX = np.finfo(np.float32).max
SCALE = 1 / 16.


@functools.lru_cache(maxsize=None)
def geometry_features():
    return (np.random.RandomState(41).normal(size=(2, 3, 64, 64)) - 2).astype(np.float32)


def cells(x1, y1, x2, y2):
    """The box whose rounded cell box is exactly [x1..x2] x [y1..y2] at scale 1/16."""
    return [16. * x1, 16. * y1, 16. * x2, 16. * y2]


# RoIs whose cell extent is a multiple of the pooled size: (pooled, boxes).  'max' is max_pool2d of the crop on these.
CELL_ALIGNED = [((7, 7), [cells(3, 5, 16, 25), cells(0, 0, 6, 6), cells(10, 20, 37, 33), cells(8, 2, 56, 57), cells(57, 57, 63, 63)]),
                ((2, 4), [cells(1, 1, 8, 4), cells(30, 40, 33, 41), cells(0, 0, 63, 63)]),
                ((14, 7), [cells(2, 4, 8, 31), cells(20, 8, 40, 63)])]

HALFWAY = [8., 24., 40., -8., -24.]         # * 1/16 = 0.5, 1.5, 2.5, -0.5, -1.5 -> 1, 2, 3, -1, -2 (halves away from zero)


def _case(name, kind, feat, boxes, idx=None, scale=SCALE, pooled=(7, 7), box_scale=1.0, dtype=np.float64):
    boxes = np.asarray(boxes, dtype=dtype).reshape(-1, 4)
    if idx is None and feat.shape[0] != 1:
        idx = np.arange(len(boxes)) % feat.shape[0]
    return dict(name=name, kind=kind, feat=feat, boxes=boxes, idx=None if idx is None else np.asarray(idx, dtype=np.int32),
                scale=scale, pooled=pooled, box_scale=box_scale)


def value_features():
    """[1,2,8,8]; pooled (4,4) over the whole map makes 2 x 2 bins.  Channel 0, bin (row, column):
    (0,0) only NaN; (0,1) NaN and values; (0,2) only -inf; (0,3) -inf and -FLT_MAX; (1,0) +inf among values; (1,1) -0.0 before +0.0
    among negatives; (1,2) +0.0 before -0.0; (1,3) only -FLT_MAX; (2,0) NaN first, then -inf, then a value."""
    f = (np.random.RandomState(42).normal(size=(1, 2, 8, 8)) - 2).astype(np.float32)
    c = f[0, 0]
    c[0:2, 0:2] = np.nan
    c[0, 2] = np.nan; c[1, 3] = np.nan
    c[0:2, 4:6] = -np.inf
    c[0:2, 6:8] = -np.inf; c[1, 6] = -FLT_MAX
    c[2, 1] = np.inf
    c[2:4, 2:4] = [[-1, -0.0], [0.0, -3]]
    c[2:4, 4:6] = [[-1, 0.0], [-0.0, -3]]
    c[2:4, 6:8] = -FLT_MAX
    c[4, 0] = np.nan; c[4, 1] = -np.inf
    f[0, 1, 5, 5] = np.nan
    f[0, 1, 6, 2] = np.inf
    return f


@functools.lru_cache(maxsize=None)
def cases():
    g = geometry_features()
    rng = np.random.RandomState(43)
    out = []
    for i, (pooled, boxes) in enumerate(CELL_ALIGNED):
        out.append(_case('cell_aligned_%d' % i, 'geometry', g, boxes, pooled=pooled))
    out.append(_case('one_cell', 'geometry', g, [cells(10, 12, 10, 12), cells(0, 0, 0, 0), cells(63, 63, 63, 63)]))
    out.append(_case('f32_edges_57_wide', 'geometry', g, [cells(2, 10, 58, 30), cells(5, 3, 61, 59)]))
    out.append(_case('f32_edges_62_high', 'geometry', g, [cells(10, 1, 30, 62), cells(4, 0, 17, 61)], pooled=(14, 7)))
    h = HALFWAY
    out.append(_case('halfway_rounding', 'geometry', g,
                     [[h[0], h[1], 200, 200], [h[1], h[2], 300, 280], [h[3], h[4], 100, 120], [h[4], h[3], 90, 200],
                      [h[2], h[0], h[2] + 144, h[1] + 80], [16, 16, h[0] + 160, h[1] + 128], [h[3], h[3], h[0], h[1]]]))
    out.append(_case('borders', 'geometry', g,
                     [[-100, 200, 200, 400], [200, -100, 400, 200], [800, 200, 1200, 400], [200, 800, 400, 1300],
                      [-50, -50, 1100, 1100], [1000, 1000, 1023, 1023], [1008, 0, 1040, 15]]))
    out.append(_case('outside', 'geometry', g, [[1100, 1100, 1300, 1300], [-500, -500, -100, -100], [100, 1040, 300, 1200],
                                                 [-300, 100, -30, 300], [2. ** 28, 0, 2. ** 28, 100]]))
    out.append(_case('inverted', 'geometry', g, [[400, 400, 200, 200], [400, 100, 200, 300], [100, 400, 300, 200]]))
    x1, y1 = rng.uniform(-40, 1150, 12), rng.uniform(-40, 1150, 12)
    out.append(_case('box_scale', 'geometry', g, np.stack([x1, y1, x1 + rng.uniform(0, 500, 12), y1 + rng.uniform(0, 500, 12)], 1),
                     box_scale=600. / 720.))
    good = [100, 120, 300, 360]
    out.append(_case('not_finite', 'geometry', g,
                     [good, [np.nan, 1, 50, 50], good, [1, 1, np.inf, 50], [1, -np.inf, 50, 50], [1e30, 1, 2, 3], [1, 1, 2, 1e300],
                      [1, -1e30, 2, 3], [2. ** 28 + 32, 0, 2. ** 28 + 32, 100], [0, 0, 100, -2. ** 29], good]))
    out.append(_case('not_finite_f32', 'geometry', g, [good, [np.nan, 1, 50, 50], [1, 1, np.inf, 50], [1e30, 1, 2, 3], good],
                     dtype=np.float32))
    out.append(_case('image_index', 'geometry', g, [good] * 6, idx=[0, -1, 1, 2, 1, -2 ** 31]))
    # values
    out.append(_case('values', 'value', value_features(), [cells(0, 0, 7, 7), cells(0, 0, 3, 3), cells(0, 0, 7, 1)], pooled=(4, 4)))
    out.append(_case('values_one_bin', 'value', value_features(), [cells(0, 0, 7, 7), cells(0, 0, 1, 1), cells(4, 0, 5, 1)], pooled=(1, 1)))
    # shapes
    def rand_boxes(n, Hf, Wf, seed):
        r = np.random.RandomState(seed)
        x1, y1 = r.uniform(-3, Wf + 1, n) * 16, r.uniform(-3, Hf + 1, n) * 16
        return np.stack([x1, y1, x1 + r.uniform(0, Wf * 12, n), y1 + r.uniform(0, Hf * 12, n)], 1)
    feats = lambda shape, seed: (np.random.RandomState(seed).normal(size=shape) - 2).astype(np.float32)
    out.append(_case('K1', 'shape', feats((1, 1, 9, 11), 50), rand_boxes(6, 9, 11, 51), pooled=(3, 5)))
    out.append(_case('K65', 'shape', feats((2, 65, 9, 11), 52), rand_boxes(5, 9, 11, 53), pooled=(7, 7)))
    out.append(_case('K130_two_chunks', 'shape', feats((2, 130, 9, 11), 54), rand_boxes(4, 9, 11, 55), pooled=(7, 7)))
    out.append(_case('K65_14x14', 'shape', feats((1, 65, 9, 11), 56), rand_boxes(3, 9, 11, 57), pooled=(14, 14)))
    out.append(_case('map_1x1', 'shape', feats((1, 3, 1, 1), 58), [[0, 0, 15, 15], [-20, -20, 40, 40], [3, 3, 4, 4], [30, 0, 50, 10]],
                     pooled=(3, 5)))
    out.append(_case('map_5x7', 'shape', feats((2, 3, 5, 7), 59), rand_boxes(10, 5, 7, 60), pooled=(7, 7)))
    out.append(_case('pooled_1x1', 'shape', g, rand_boxes(8, 64, 64, 61), pooled=(1, 1)))
    out.append(_case('pooled_32x32', 'shape', feats((1, 5, 40, 48), 62), rand_boxes(4, 40, 48, 63), pooled=(32, 32)))
    out.append(_case('N0', 'shape', g[:1], np.zeros((0, 4))))
    out.append(_case('N1', 'shape', g[:1], [[100, 120, 300, 360]]))
    out.append(_case('N300', 'shape', g, rand_boxes(300, 64, 64, 64) * 0.4, pooled=(3, 5)))
    # 'align': samples at y = -1, y = Hf and lo = Hf - 1 (scale 1, sampling 1, pooled (2,2): the samples lie at y1 + .5, y1 + 1.5)
    out.append(_case('align_rim', 'align', feats((1, 2, 8, 8), 65),
                     [[-1.5, -1.5, 0.5, 0.5], [6.5, 6.5, 8.5, 8.5], [-1.75, -1.75, 0.25, 0.25], [6.75, 6.75, 8.75, 8.75],
                      [-1.5, 6.5, 0.5, 8.5], [2.25, 3.5, 6.75, 7.0]], scale=1.0, pooled=(2, 2)))
    return out


def align_params(case):
    """The (sampling, aligned) pairs 'align' runs a case with: all six on the geometry and rim cases."""
    if case['kind'] in ('geometry', 'align'):
        return [(s, a) for s in (1, 2, 3) for a in (False, True)]
    return [(2, False), (3, True)]


def runs():
    """Every (case index, mode, sampling, aligned) of the list."""
    out = []
    for i, c in enumerate(cases()):
        if c['kind'] != 'align':
            out.append((i, 'max', 0, False))
        out += [(i, 'align', s, a) for s, a in align_params(c)]
    return out


def run_id(run):
    i, mode, s, a = run
    return cases()[i]['name'] + ('-max' if mode == 'max' else '-align%d%s' % (s, 'a' if a else ''))
