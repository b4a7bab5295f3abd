"""The one-sign threshold test of pred_sign (csrc/nms_kernels.hpp) against the reference's quotient, in numpy (no GPU).

The reference decides a pair by RN(inter / uni) >= t32 in float32 (knife_spec.quotient).  graph_lists_kernel and
iou_bits_sym_kernel decide it by ONE sign: with hg = (t32 - nextafter(t32, 0)) / 2,

    hit  <=>  the sign bit of  fma(hg, uni, fma(-t32, uni, inter))  is clear

-- the real quotient rounds to >= t32 iff it is at least the midpoint t32 - hg, the inner fma is exact wherever that matters
and the outer one has the sign of its real value.  The rule is restated here with knife_spec.fma_f32 (one rounding per
fma), with the kernels' unclamped h, and compared pair by pair with the quotient: on the pairs the knife-edge search finds
next to every threshold (UP: only the quotient's rounding says "suppress"; BAND: just below), on the closed-form families
and on a seeded bulk of random boxes.  Zero disagreements, and the search must have found UP and BAND pairs."""
import numpy as np
import pytest

import knife_spec as K

F32 = np.float32
THRESHOLDS = K.THRESHOLDS + (1e-3, 1.0)
SEED, DRAWS, BULK = 7, 20000, 200000


def half_gap(t32):
    """csrc/vdet_capi.hip half_gap: a power of two, 2^-26 for 0.3f."""
    t32 = F32(t32)
    return F32((t32 - np.nextafter(t32, F32(0))) * F32(0.5))


def one_sign(a, b, t32):
    """pred_sign on pairs [n, 4]: the reference's operation order, h NOT clamped, the sign bit of the folded margin."""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    one, zero = F32(1), F32(0)
    xx1 = np.maximum(a[:, 0], b[:, 0]); yy1 = np.maximum(a[:, 1], b[:, 1])
    xx2 = np.minimum(a[:, 2], b[:, 2]); yy2 = np.minimum(a[:, 3], b[:, 3])
    w = np.maximum(zero, (xx2 - xx1) + one)
    h = (yy2 - yy1) + one
    inter = (w * h).astype(F32)
    ai = ((a[:, 2] - a[:, 0]) + one) * ((a[:, 3] - a[:, 1]) + one)
    aj = ((b[:, 2] - b[:, 0]) + one) * ((b[:, 3] - b[:, 1]) + one)
    uni = ((ai + aj) - inter).astype(F32)
    m = K.fma_f32(half_gap(t32), uni, K.fma_f32(-F32(t32), uni, inter))
    return ~np.signbit(m)


def bulk_pairs(seed, n, frac):
    """Random overlapping boxes whose IoU spreads over (0, 1]: the second box is the first with every edge moved by up to a
    per-pair fraction of its size; every 17th pair is moved apart in y instead (negative unclamped h)."""
    rng = np.random.RandomState(seed)
    unit = 16.0 if frac else 1.0
    hi = 2000 * 16 if frac else 4000
    x1 = rng.randint(0, hi, n); y1 = rng.randint(0, hi, n)
    w = rng.randint(8, hi, n); h = rng.randint(8, hi, n)
    a = np.stack([x1, y1, x1 + w, y1 + h], 1)
    f = rng.rand(n, 1) ** 2 * 0.6
    d = ((rng.rand(n, 4) * 2 - 1) * f * np.stack([w, h, w, h], 1)).astype(np.int64)
    b = a + d
    b[:, 2] = np.maximum(b[:, 2], b[:, 0]); b[:, 3] = np.maximum(b[:, 3], b[:, 1])
    b[::17, 1] += 3 * h[::17] + 40; b[::17, 3] += 3 * h[::17] + 40
    return (a / unit).astype(F32), (b / unit).astype(F32)


@pytest.fixture(scope='module')
def found():
    out = {}
    for t in THRESHOLDS:
        pairs = []
        for search in (K.search_integer, K.search_fractional):
            for a, b in search(t, SEED, DRAWS).values():
                pairs.append((a, b))
        out[t] = (np.concatenate([p[0] for p in pairs]), np.concatenate([p[1] for p in pairs]))
    return out


def test_half_gap_is_a_power_of_two():
    assert float(half_gap(K.thresh_to_f32(0.3))) == 2.0 ** -26
    for t in THRESHOLDS + (1e-20, 0.999):
        hg = float(half_gap(K.thresh_to_f32(t)))
        m, _ = np.frexp(hg)
        assert m == 0.5 and hg >= 2.0 ** -126
        t32 = K.thresh_to_f32(t)
        assert float(t32) - 2.0 * hg == float(np.nextafter(t32, F32(0)))


@pytest.mark.parametrize('t', THRESHOLDS)
def test_search_pairs(found, t):
    a, b = found[t]
    t32 = K.thresh_to_f32(t)
    c = K.classify(a, b, t)
    print('t = %g: %d pairs, UP %d, BAND %d, BELOW1 %d, ABOVE1 %d, ZERO %d'
          % (t, a.shape[0], c['UP'].sum(), c['BAND'].sum(), c['BELOW1'].sum(), c['ABOVE1'].sum(), c['ZERO'].sum()))
    # (knife_spec.POW2 has no UP pair: r is exact near the edge.  1.0 is outside POW2 but the nested search finds no pair at
    #  all there -- its UP and BAND pairs are the business of test_threshold_one_has_band_pairs_and_cannot_have_up_pairs)
    if t not in K.POW2 + (1.0,):
        assert c['UP'].sum() >= 1 and c['BAND'].sum() >= 1, 'the search found no knife-edge pair: the test would be vacuous'
    for x, y in ((a, b), (b, a)):
        hit = one_sign(x, y, t32)
        assert np.array_equal(hit, K.quotient(x, y)[2] >= t32), np.flatnonzero(hit != (K.quotient(x, y)[2] >= t32))[:8]


def near_duplicates(seed, tries=4000):
    """Pairs for threshold 1.0 (knife_spec.unit_family's construction, every draw kept): a wide fractional box and the same
    box with its right edge one ulp to the left.  Where the areas round apart the quotient is the float32 just below 1."""
    rng = np.random.RandomState(seed)
    x2 = (rng.randint(60000, 65535, tries) + rng.randint(0, 256, tries) / 256.0).astype(F32)
    h = (rng.randint(0, 40 * 16, tries) / 16.0).astype(F32)
    big = np.stack([np.zeros(tries, F32), np.zeros(tries, F32), x2, h], 1)
    small = big.copy()
    small[:, 2] = np.nextafter(x2, F32(0))
    return big, small


def test_threshold_one_has_band_pairs_and_cannot_have_up_pairs():
    """At 1.0 an UP pair (inter < uni and RN(inter / uni) >= 1) does not exist in float32: the largest inter below uni is
    its predecessor, and uni - ulp over uni is at most 1 - 2^-24, itself a float32 below 1 -- checked here on every binade's
    ends and on random unions.  So "at least one UP pair" can only be asked of the BAND side at this threshold: the
    near-duplicates must hold BAND pairs (quotient one float32 below 1), and the rule must get all of them right."""
    rng = np.random.RandomState(SEED)
    uni = np.concatenate([np.ldexp(F32(1), np.arange(-20, 100)).astype(F32),
                          np.nextafter(np.ldexp(F32(1), np.arange(-20, 100)).astype(F32), F32(0)),
                          (rng.rand(100000) * 2.0 ** rng.randint(0, 90, 100000)).astype(F32) + F32(1)])
    assert np.all((np.nextafter(uni, F32(0)) / uni).astype(F32) < F32(1))
    a, b = near_duplicates(SEED)
    c = K.classify(a, b, 1.0)
    print('t = 1: %d near-duplicates, UP %d, BAND %d, ZERO %d' % (a.shape[0], c['UP'].sum(), c['BAND'].sum(), c['ZERO'].sum()))
    assert c['UP'].sum() == 0 and c['BAND'].sum() >= 1 and c['ZERO'].sum() >= 1
    for x, y in ((a, b), (b, a)):
        assert np.array_equal(one_sign(x, y, F32(1)), K.quotient(x, y)[2] >= F32(1))


REGULAR_COORD_MAX = 2.0 ** 60       # csrc/nms_kernels.hpp kRegularCoordMax: what frame_flags_kernel lets a regular frame hold


def huge_pairs():
    """Pairs whose unions are huge or whose boxes lie far apart, every coordinate within the bound of a regular frame: the
    unclamped h is hugely negative, the areas sum to ~2^124.  (Beyond the bound w * h or the area sum overflow, uni is inf
    and the folded margin would be inf - inf: such frames are not regular and never reach pred_sign.)"""
    M = REGULAR_COORD_MAX
    a = [[0, 0, 10, 10], [0, 0, 10, 10], [-M, -M, M, M], [-M, -M, M, M], [-M, -M, M, M], [0, 0, M, M], [0, 0, 10, 10], [-M, 0, M, 10]]
    b = [[0, M, 10, M], [0, -M, 10, -M], [-M, -M, M, M], [-M, -M, M, 0], [0, 0, 10, 10], [M, M, M, M], [0, 1e17, 10, 1e17 + 1e10], [-M, M, M, M]]
    return np.asarray(a, F32), np.asarray(b, F32)


@pytest.mark.parametrize('t', THRESHOLDS + (3.0, 2.0 ** 24))
def test_huge_and_far_apart_boxes_give_no_nan(t):
    t32 = K.thresh_to_f32(t)
    a, b = huge_pairs()
    assert np.abs(a).max() <= REGULAR_COORD_MAX and np.abs(b).max() <= REGULAR_COORD_MAX
    for x, y in ((a, b), (b, a)):
        inter, uni, q = K.quotient(x, y)
        assert np.all(np.isfinite(uni)) and np.all(uni > 0)
        with np.errstate(all='ignore'):
            m = K.fma_f32(half_gap(t32), uni, K.fma_f32(-F32(t32), uni, inter))
        assert not np.any(np.isnan(m))
        with np.errstate(all='ignore'):
            assert np.array_equal(one_sign(x, y, t32), q >= t32)
    if t <= 1.0:
        assert (K.quotient(a, b)[2] >= t32).any()          # (the identical huge boxes)


@pytest.mark.parametrize('t', THRESHOLDS)
def test_families(t):
    t32 = K.thresh_to_f32(t)
    fams = [K.reach_family(t, SEED)]
    if t == 1.0:
        fams += list(K.unit_family(SEED))
    for a, b in fams:
        assert a.shape[0]
        for x, y in ((a, b), (b, a)):
            assert np.array_equal(one_sign(x, y, t32), K.quotient(x, y)[2] >= t32)


@pytest.mark.parametrize('t', THRESHOLDS)
def test_bulk(t):
    t32 = K.thresh_to_f32(t)
    for frac in (False, True):
        a, b = bulk_pairs(SEED + int(frac), BULK // 2, frac)
        q = K.quotient(a, b)[2]
        assert (q >= t32).mean() > 0.01 or t == 1.0              # (both answers occur: the bulk is no one-sided check)
        assert (q < t32).mean() > 0.01
        assert np.array_equal(one_sign(a, b, t32), q >= t32)
