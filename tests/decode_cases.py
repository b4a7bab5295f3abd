"""The case list the numpy rule (decode_spec.py) and the device (test_decode_gpu.py) share: ``cases()`` returns
(name, rois [n,4] f32 / f64, deltas [n,K,4] f32, (H, W)) tuples, built once and never written to."""
import functools

import numpy as np

F32, F64 = np.float32, np.float64
NAN, INF = np.nan, np.inf

EDGE_NAMES = ('on_border', 'beyond_border', 'neg_zero', 'dw_pm10', 'overflow_edge', 'nonfinite_roi', 'nonfinite_delta',
              'zero_width', 'inverted', 'f64_rois')


def random_case(seed, n, K, im_size=(375, 500), f64=False, spread=0.5):
    """rois inside the image (as proposals are), deltas N(0, spread): the shape of a head's output"""
    rng = np.random.RandomState(seed)
    H, W = im_size
    x1, y1 = rng.uniform(0, W - 2, n), rng.uniform(0, H - 2, n)
    x2, y2 = x1 + rng.uniform(0, W - 1 - x1), y1 + rng.uniform(0, H - 1 - y1)
    rois = np.stack([x1, y1, x2, y2], axis=1)
    rois = rois if f64 else rois.astype(F32)
    deltas = (rng.standard_normal((n, K, 4)) * spread).astype(F32)
    return rois, deltas


def _one(rois, deltas, dtype=F32):
    rois = np.asarray(rois, dtype).reshape(-1, 4)
    deltas = np.asarray(deltas, F32)
    return rois, deltas.reshape(len(rois), -1, 4)


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    for seed, n, K, f64 in ((1, 150, 5, False), (2, 97, 1, False), (3, 40, 67, False), (4, 150, 5, True)):
        out.append(('random_%d' % seed,) + random_case(seed, n, K, f64=f64) + ((375, 500),))
    z = [0.0, 0.0, 0.0, 0.0]
    # corners that land exactly on 0, W-1 and H-1: x1 = 0 gives X1 = 0.5w - 0.5w = 0; a side of 1023 absorbs the 1e-14
    out.append(('on_border',) + _one([[0, 0, 1023, 767], [0, 0, 1023, 767]], [[z], [[0, 0, -0.0, -0.0]]]) + ((768, 1024),))
    # ... and just beyond them: 99 + 1e-14 rounds up to the next f64 after 99; a negative x1 by 2^-40
    out.append(('beyond_border',) + _one([[0, 0, 99, 49], [-2.0 ** -40, -2.0 ** -40, 99, 49], [5, 5, 99.5, 49.5],
                                          [-3, -4, 20, 20]],
                                         [[z, [0.25, 0.25, 0, 0]], [z, [0, 0, 0.5, 0.5]], [z, [1, 1, 0, 0]], [z, [-1, -1, 1, 1]]])
               + ((50, 100),))
    nz = -0.0
    out.append(('neg_zero',) + _one([[nz, nz, nz, nz], [nz, nz, 10, 10], [1e-14, 1e-14, 0, 0], [nz, 0.0, 0.0, nz]],
                                    [[[nz, nz, nz, nz], [nz, nz, -INF, -INF]]] * 4, F64) + ((50, 100),))
    out.append(('dw_pm10',) + _one([[10, 10, 20, 20], [10, 10, 10.001, 10.001], [0, 0, 499, 374]],
                                   [[[0, 0, 10, 10], [0, 0, -10, -10], [0.1, -0.1, 10, -10]]] * 3) + ((375, 500),))
    # the edges of E: 709 is the last finite argument, -708 the last non-zero one; f32 neighbours on both sides
    e = [F32(709.0), np.nextafter(F32(709.0), F32(INF)), np.nextafter(F32(709.0), F32(0)), F32(-708.0),
         np.nextafter(F32(-708.0), F32(-INF)), np.nextafter(F32(-708.0), F32(0)), F32(88.7), F32(-103.0), F32(3.4e38), F32(-3.4e38)]
    out.append(('overflow_edge',) + _one([[10, 10, 20, 20], [1e-300, 1e-300, 3e-300, 3e-300], [0, 0, 1e300, 1e300]],
                                         [[[0, 0, a, b] for a, b in zip(e, e[::-1])]] * 3, F64) + ((375, 500),))
    out.append(('nonfinite_roi',) + _one([[NAN, 1, 20, 20], [1, NAN, 20, 20], [1, 1, NAN, 20], [1, 1, 20, NAN], [INF, 1, 20, 20],
                                          [1, -INF, 20, 20], [1, 1, INF, 20], [-INF, 1, INF, -INF], [NAN] * 4],
                                         [[z, [0.1, 0.1, 0.1, 0.1]]] * 9) + ((375, 500),))
    bad = [[NAN, 0, 0, 0], [0, NAN, 0, 0], [0, 0, NAN, 0], [0, 0, 0, NAN], [INF, 0, 0, 0], [0, -INF, 0, 0], [0, 0, INF, 0],
           [0, 0, 0, -INF], [INF, INF, -INF, INF], [NAN] * 4]
    out.append(('nonfinite_delta',) + _one([[10, 10, 20, 20], [0, 0, 0, 0]], [bad, bad]) + ((375, 500),))
    out.append(('zero_width',) + _one([[7, 7, 7, 7], [7, 3, 7, 30], [0, 0, 0, 0], [499, 374, 499, 374]],
                                      [[z, [0.5, 0.5, 1, 1], [1e14, -1e14, 30, 30]]] * 4) + ((375, 500),))
    out.append(('inverted',) + _one([[20, 20, 10, 10], [20, 5, 10, 30], [1e-14, 0, 0, 1e-14]],
                                    [[z, [0.5, -0.5, 1, -1], [-2, 2, 3, 3]]] * 3) + ((375, 500),))
    # f64 rois that no f32 holds: rounding them to f32 first would move the result
    rois, deltas = random_case(5, 64, 3, f64=True)
    out.append(('f64_rois', rois + 1e-9 / 3, deltas, (375, 500)))
    for c in out:
        c[1].setflags(write=False); c[2].setflags(write=False)
    return tuple(out)
