#!/usr/bin/env python3
"""Generate tests/golden/knife_pairs.npz: box pairs on the knife edge of the IoU threshold test, found by tests/knife_spec.py
with fixed seeds (numpy only: runs anywhere).  The fixture holds the box pairs and nothing else; their classes are
recomputed by whoever reads it (tests/test_knife_edge_cpu.py asserts the counts printed here).

  int_<t>_a / _b    uint16 [n, 4]   integer form, cell-local coordinates
  frac_<t>_a / _b   uint16 [n, 4]   fractional form, cell-local coordinates in units of 2^-4 px
  reach_<t>_a / _b  uint16 [n, 4]   the reach-tight families (y1 = 0), thresholds of the search plus 1e-3 and 1.0
  unit_same_a, unit_near_a / _b     float32: identical boxes and near-duplicates with quotient exactly 1

Classes the search cannot reach, and why:
  UP at 0.25 and 0.5 (both forms): none exists.  t32 is a power of two, so t32 * uni is exact and, next to the threshold,
    inter and t32 * uni lie within a factor of two of each other: r = inter - t32 * uni is exact (Sterbenz) and its sign
    is the sign of the real margin.  A real quotient below t32 differs from it by at least one unit in the last place of
    inter or uni, i.e. by 2^-24 relative, and the floats just below a power of two are 2^-24 apart relative: the quotient
    is at least one whole spacing below t32 and cannot round up to it.  test_knife_edge_cpu.py asserts that the fixture
    has none and checks the argument on directed samples.
  UP with a real quotient other than the decimal threshold at 0.1 (both forms): none for unions that fit a 4096 px cell.  t32 lies
    1.49e-9 above 1/10 and half an ulp is 3.7e-9, so the real quotient must lie in [1/10 - 2.3e-9, 1/10 + 1.5e-9): with
    inter and uni whole numbers of units (1 px^2, or 2^-8 px^2) that means |10 * inter - uni| < 2.3e-8 * uni, below 0.4
    for every union that fits a cell (2^24 units), hence 10 * inter == uni.  The 20 UP pairs at 0.1 all have IoU 1/10.
    (Boxes larger than a cell have rounded areas and may hold such a pair; they do not fit the one-pair-per-cell frames
    and were not searched.)

    python tests/golden/make_knife_pairs.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import knife_spec as K  # noqa: E402

ORDER = ('UP', 'UPDEEP', 'UPEXACT', 'BELOW1', 'BAND', 'ABOVE1', 'ZERO')


def main():
    out = {}
    for i, t in enumerate(K.THRESHOLDS):
        for form, search, unit in (('int', K.search_integer, 1), ('frac', K.search_fractional, K.FRAC_UNIT)):
            got = search(t, 7100 + 10 * i + (form == 'frac'))
            a = np.concatenate([got[k][0] for k in ORDER]) * unit
            b = np.concatenate([got[k][1] for k in ORDER]) * unit
            assert np.array_equal(a, np.rint(a)) and a.min() >= 0 and a.max() < 65536
            out['%s_%g_a' % (form, t)], out['%s_%g_b' % (form, t)] = a.astype(np.uint16), b.astype(np.uint16)
            c = K.classify(a / np.float32(unit), b / np.float32(unit), t)
            print('%-4s t=%-5g pairs=%3d ' % (form, t, a.shape[0]) + ' '.join('%s=%d' % (k, int(c[k].sum())) for k in K.CLASSES)
                  + ' UP(real != t)=%d' % sum(K.real_quotient(x, y) != K.Fraction(str(t))
                                               for x, y in zip(a[c['UP']] / np.float32(unit), b[c['UP']] / np.float32(unit))))
    for i, t in enumerate(K.FAMILY_THRESHOLDS):
        a, b = K.reach_family(t, 7300 + i)
        out['reach_%g_a' % t], out['reach_%g_b' % t] = a.astype(np.uint16), b.astype(np.uint16)
        c = K.classify(a, b, t)
        print('reach t=%-5g pairs=%3d sup=%d ' % (t, a.shape[0], int(c['sup'].sum())) + ' '.join('%s=%d' % (k, int(c[k].sum())) for k in K.CLASSES))
    same, near = K.unit_family(7400)
    out['unit_same_a'], out['unit_near_a'], out['unit_near_b'] = same[0], near[0], near[1]
    print('unit: %d identical, %d near-duplicates with quotient 1' % (same[0].shape[0], near[0].shape[0]))
    path = os.path.join(HERE, 'knife_pairs.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
