"""The knife-edge fixture and the claim the divide-free predicates rest on, without a GPU.

tests/golden/knife_pairs.npz holds box pairs whose IoU sits on the edge of the threshold test (tests/knife_spec.py); here
the fixture is re-classified so that a later edit cannot hollow it out, the numpy model is pinned to the oracle pair by
pair, and the kernels' rule -- sign of one fma, IEEE quotient inside a band of 2^-21 * t32 * uni below zero -- is checked
as a property on directed samples.
"""
import os
from fractions import Fraction

import numpy as np
import pytest

import knife_spec as K

F32 = np.float32
PAIRS = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'knife_pairs.npz')

# Non-exact UP pairs (real quotient != the decimal threshold) the search reaches: none at 0.1 for unions that fit a cell, no UP pair at all at the
# powers of two -- tests/golden/make_knife_pairs.py says why -- and at least 16 everywhere else.
UP_OTHER_MIN = {0.1: 0, 0.25: 0, 0.5: 0}


@pytest.fixture(scope="module")
def pairs():
    return K.load_pairs(PAIRS)


@pytest.mark.parametrize("form", ["int", "frac"])
@pytest.mark.parametrize("t", K.THRESHOLDS)
def test_fixture_holds_every_class(pairs, t, form):
    a, b = pairs[(form, t)]
    if form == "int":
        assert np.array_equal(a, np.rint(a)) and min(a.min(), b.min()) >= 0 and max(a.max(), b.max()) < K.INT_BOX
    else:
        assert np.array_equal(a * 16, np.rint(a * 16)) and not np.array_equal(a, np.rint(a))
        assert min(a.min(), b.min()) >= 0 and max(a.max(), b.max()) < K.FRAC_BOX
    c = K.classify(a, b, t)
    n = {k: int(c[k].sum()) for k in K.CLASSES}
    other = sum(K.real_quotient(x, y) != Fraction(str(t)) for x, y in zip(a[c['UP']], b[c['UP']]))
    print(form, t, n, 'UP with a real quotient other than t:', other)
    assert n['BAND'] >= 16 and n['ABOVE1'] >= 16 and n['BELOW1'] >= 4
    if t in K.POW2:
        assert n['UP'] == 0                      # none exists (see the generator's docstring)
    else:
        assert n['UP'] >= 16
    assert other >= UP_OTHER_MIN.get(t, 16)
    if t in K.EXACT:
        assert n['ZERO'] >= 16
    # UP pairs are the ones on which only the quotient says "suppress"; BAND pairs the ones the fallback must keep
    assert np.all(c['sup'][c['UP']]) and not np.any(c['sup'][c['BAND']]) and np.all(c['sup'][c['ABOVE1']])


def test_closed_form_families(pairs):
    for t in K.FAMILY_THRESHOLDS:
        a, b = pairs[('reach', t)]
        assert a.shape[0] >= 16 and a[:, 2].max() > 30000           # wide: 0.1 % is many pixels, float32 reach is coarse
        tf = Fraction(str(t))
        for x, y in zip(a, b):
            W, w = int(x[2] - x[0]) + 1, int(y[2] - y[0]) + 1
            assert w == tf * W and y[2] == x[2] and y[0] - x[0] == (1 - tf) * W      # flush right, offset exactly (1 - t) W
            assert K.real_quotient(x, y) == tf
    for kind in ('same', 'near'):
        a, b = pairs[('unit', kind)]
        inter, uni, q = K.quotient(a, b)
        assert a.shape[0] >= 4 and np.all(q == 1) and np.array_equal(a, b) == (kind == 'same')


def _all_pairs(pairs):
    for (form, t), (a, b) in sorted(pairs.items(), key=str):
        for tt in ((1.0,) if form == 'unit' else (t,)):
            yield form, tt, a, b


def test_model_is_the_oracle_pair_by_pair(pairs, oracle):
    """Each fixture pair alone in a two-box list, in both score orders: oracle.nms keeps or drops the second box exactly as
    q >= t32 says -- and the kernels' rule, in both of its forms, says the same."""
    n = 0
    for form, t, a, b in _all_pairs(pairs):
        c = K.classify(a, b, t)
        assert np.array_equal(K.decide_fma(a, b, t), c['sup']), (form, t)
        assert np.array_equal(K.decide_margins(a, b, t), c['sup']), (form, t)
        for i in range(a.shape[0]):
            for first, second in ((a[i], b[i]), (b[i], a[i])):
                d = np.array([list(first) + [0.9], list(second) + [0.8]], F32)
                want = [0] if c['sup'][i] else [0, 1]
                assert oracle.nms(d, t) == want, (form, t, i)
                assert oracle.nms(d[::-1].copy(), t) == [1 - k for k in want], (form, t, i)
                n += 1
    assert n > 2000


def test_the_tests_bite(pairs):
    """The two ways a site could be subtly wrong disagree with the reference on the fixture: the sign of r alone (no
    fallback) on every UP pair; a band of 2^-25 instead of 2^-21 on the UP pairs below it.  Per threshold and over both
    forms at least 16 pairs each -- except at the powers of two, where r is exact and no pair can tell (none exists)."""
    for t in K.THRESHOLDS:
        nosign = narrow = 0
        for form in ('int', 'frac'):
            a, b = pairs[(form, t)]
            sup = K.classify(a, b, t)['sup']
            nosign += int((K.decide_fma(a, b, t, fallback=False) != sup).sum())
            narrow += int((K.decide_fma(a, b, t, rel=2.0 ** -25) != sup).sum())
        print('t = %g: sign of r alone wrong on %d pairs, band 2^-25 wrong on %d pairs' % (t, nosign, narrow))
        if t in K.POW2:
            assert nosign == 0 and narrow == 0
        elif t == 0.1:       # (every UP pair in range has IoU exactly 1/10: r = -(t32 - 1/10) * uni = -2^-26 * t32 * uni)
            assert nosign >= 16 and narrow == 0
        else:
            assert nosign >= 16 and narrow >= 16


def _directed_samples(seed, n):
    rng = np.random.RandomState(seed)
    fixed = [K.thresh_to_f32(t) for t in K.THRESHOLDS + (1e-3, 1.0, 1e-20, 0.999)]
    rnd = np.concatenate([rng.uniform(0.01, 1.0, 40), np.exp(rng.uniform(np.log(1e-6), 0.0, 40))]).astype(F32)
    ts = np.concatenate([np.asarray(fixed, F32), rnd])
    t32 = ts[rng.randint(0, ts.size, n)]
    uni = np.exp2(rng.uniform(0.0, 32.0, n)).astype(F32)
    inter = (t32 * uni).astype(F32)
    for _ in range(8):          # -8 .. 8 ulps
        step = rng.randint(-1, 2, n)
        inter = np.where(step > 0, np.nextafter(inter, F32(np.inf)), np.where(step < 0, np.nextafter(inter, F32(0)), inter))
    return inter, uni, t32


def test_the_band_holds_every_pair_the_quotient_suppresses():
    """On directed (inter, uni, t32) -- uni log-uniform in [1, 2^32], inter = RN(t32 * uni) moved by up to 8 ulps:
    q >= t32 implies r >= -2^-22 * t32 * uni (the comment of iou_bits_sym_kernel) and qlo >= 0 (the two-margin form), and
    r >= 0 implies q >= t32.  At a power of two r < 0 implies q < t32 (no UP pair exists)."""
    inter, uni, t32 = _directed_samples(20261, 400000)
    with np.errstate(all='ignore'):
        q = (inter / uni).astype(F32)
    r, qlo = K.margins(inter, uni, t32)
    sup = q >= t32
    assert 0.2 < sup.mean() < 0.8 and int((sup & (r < 0)).sum()) > 1000          # the samples do straddle the edge
    bound = -(2.0 ** -22) * t32.astype(np.float64) * uni.astype(np.float64)      # (exact: 48-bit product, scaled)
    bad = np.flatnonzero(sup & (r.astype(np.float64) < bound))
    assert bad.size == 0, [(float(inter[i]), float(uni[i]), float(t32[i])) for i in bad[:5]]
    bad = np.flatnonzero(sup & (r < -K.band_of(uni, t32)))                        # pred_regular's own float32 bound
    assert bad.size == 0, [(float(inter[i]), float(uni[i]), float(t32[i])) for i in bad[:5]]
    bad = np.flatnonzero(sup & ~(qlo >= 0))
    assert bad.size == 0, [(float(inter[i]), float(uni[i]), float(t32[i])) for i in bad[:5]]
    bad = np.flatnonzero((r >= 0) & ~sup)
    assert bad.size == 0, [(float(inter[i]), float(uni[i]), float(t32[i])) for i in bad[:5]]
    m, _ = np.frexp(t32)
    pow2 = m == 0.5
    assert pow2.sum() > 10000 and not np.any(pow2 & sup & (r < 0))


def test_fma_model_is_single_rounded():
    """fma_f32 against rational arithmetic on operands near and far from cancellation."""
    rng = np.random.RandomState(5)
    a = rng.randn(300).astype(F32); b = np.exp2(rng.uniform(-20, 30, 300)).astype(F32)
    c = np.concatenate([(-a[:150] * b[:150]).astype(F32), rng.randn(150).astype(F32)])
    got = K.fma_f32(a, b, c)
    for i in range(300):
        want = K._rn_f32(Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i])))
        assert got[i] == want, i
    assert float(K.thresh_to_f32(0.3)) > 0.3 and float(K.thresh_to_f32(0.5)) == 0.5 and float(K.thresh_to_f32(0.7)) >= 0.7
    assert float(np.nextafter(K.thresh_to_f32(0.7), F32(0))) < 0.7


@pytest.mark.parametrize("B", [300, 600])
@pytest.mark.parametrize("t", K.FAMILY_THRESHOLDS[:-1])
def test_reach_frames_bite(t, B):
    """The reach frames of the GPU suite against a numpy model of the reach table (K.reach_model): the kernels' bound culls
    no suppressed pair; a bound without the margin and two pixels tighter culls every pair in the block test of
    iou_bits_sym_kernel / the adjacency kernel (at least 4 per frame), and in graph_lists_kernel's walk (frames of more than
    384 boxes) the pairs that cross a 256-rank tile (at least 2 per frame); one pixel tighter does the same wherever the
    inner box starts exactly (1 - t) * W to the right (thresholds that thresh_to_f32 does not round up)."""
    for seed in K.REACH_SEEDS:
        boxes, pr = K.reach_frame(t, B, seed)
        m = pr.shape[0]
        assert m == (B - 1) // 64 >= 4 and np.array_equal(boxes, np.rint(boxes)) and boxes.min() >= 0 and boxes.max() <= 65535
        off = np.abs(boxes[pr[:, 0], 0] - boxes[pr[:, 1], 0])
        wide = np.maximum(boxes[pr[:, 0], 2] - boxes[pr[:, 0], 0], boxes[pr[:, 1], 2] - boxes[pr[:, 1], 0]) + 1
        exact = bool(np.all(off == np.asarray([float((1 - Fraction(str(t))) * int(w)) for w in wide])))
        lost = {(mode, lists): K.reach_model(boxes, t, pr, mode, lists) for mode in K.REACH_MODES for lists in (False, True)}
        print(t, B, seed, 'exact' if exact else 'one pixel inside', lost)
        assert lost[('kernel', False)] == 0 and lost[('kernel', True)] == 0
        assert lost[('tight2', False)] == m
        assert lost[('tight1', False)] == (m if exact else 0)
        if B > 384:
            assert lost[('tight2', True)] >= 2 and lost[('tight1', True)] >= (2 if exact else 0)


# ---- the x-bucket windows -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", K.WINDOW_B)
@pytest.mark.parametrize("t", K.WINDOW_THRESHOLDS)
def test_window_frames_hold_what_they_are_built_for(oracle, t, B):
    """Every window frame of the GPU suite (tests/test_xwindow_gpu.py takes its B, band heights, thresholds, families and seed
    from K.WINDOW_B, K.window_band, K.WINDOW_THRESHOLDS, K.WINDOW_FAMILIES and K.WINDOW_SEED, as this test does): the family's
    geometry is what its name says, every pinned pair is a true partner by the referee of its site -- classify()['sup'] for the
    suppression graph, the oracle's link rule (its float32 IoU of the TRUNCATED current box >= the threshold) for the link
    scans, the oracle's float64 IoU > t on the strict frames of re-scoring -- and the windows as the kernels write them
    (window_model, mode 'kernel') hold every pinned pair at every site."""
    for family in K.WINDOW_FAMILIES:
        for strict in (False, True):
            boxes, pairs = K.window_frame(t, B, family, K.WINDOW_SEED, strict)
            assert boxes.shape == (B, 4) and boxes.dtype == F32 and pairs.shape[0] >= 2
            w, h = boxes[:, 2] - boxes[:, 0] + 1, boxes[:, 3] - boxes[:, 1] + 1
            assert np.isfinite(boxes).all() and w.min() > 0 and h.min() > 0 and boxes.min() >= 0 and boxes.max() <= 65535  # regular
            whole = bool(np.array_equal(boxes, np.rint(boxes)))
            assert whole == (family != 'frac')                                                       # kFlagU16 or not
            rank, cum, xmin, scale, wmax = K.window_index(boxes)
            O, I = boxes[pairs[:, 0]], boxes[pairs[:, 1]]
            assert np.array_equal(O[:, 2], I[:, 2]) or family == 'flat'                              # flush right, full height
            assert np.array_equal(O[:, [1, 3]], I[:, [1, 3]])
            if family == 'flat':
                assert scale == 0 and cum[1] == B
            elif family == 'coarse':
                assert scale == F32(1.0 / 16)
            else:
                assert scale == 1.0
            if family in ('unit', 'wmaxcap', 'frac'):          # O the last rank of a word, I the first of a later one
                assert np.all(rank[pairs[:, 0]] % 64 == 63) and np.all(rank[pairs[:, 1]] % 64 == 0)
                assert np.all(rank[pairs[:, 1]] - rank[pairs[:, 0]] >= 65)
                assert (wmax == K.WINDOW_W) == (family == 'wmaxcap')
                assert np.all((I[:, 2] - I[:, 0] + 1) / F32(t) * F32(1.001) > K.WINDOW_W)            # ... so min(wmax, .) decides
            if family == 'top':
                xmax = boxes[:, 0].max()
                assert sorted(I[:2, 0]) == [xmax - 1, xmax] and sorted(O[2:, 0]) == [xmin, xmin + 1]
                assert cum[256] - cum[255] == 2 and cum[255] % 64 == 0
            if family == 'coarse':                             # the pinned partner is alone in its bucket
                bk = [K.xbucket(x, xmin, scale) for x in boxes[:, 0]]
                alone = [bk.count(bk[r]) == 1 for r in pairs.ravel()]
                assert sum(alone) >= pairs.shape[0]
            for o, i in pairs:
                for q, p in ((o, i), (i, o)):
                    if strict:
                        with np.errstate(all='ignore'):
                            assert oracle.iou([boxes[q]], boxes[p:p + 1]).ravel()[0] > t
                        assert K.window_partner(boxes[q], boxes[p], t, 'xwindow')
                    else:
                        assert K.classify(boxes[q][None], boxes[p][None], t)['sup'][0]
                        cur = np.trunc(K.link_query(boxes[q]) if family == 'frac' else boxes[q])
                        assert float(oracle._iou_f32_row(cur, boxes[p:p + 1])[0]) >= t
                        assert K.window_partner(K.link_query(boxes[q]) if family == 'frac' else boxes[q], boxes[p], t, 'link')
            for site in K.WINDOW_SITES:
                if strict == (site == 'xwindow'):
                    true, lost = K.window_lost(boxes, pairs, t, site, 'kernel', family == 'frac')
                    assert true == 2 * pairs.shape[0] and lost == 0, (family, site)


@pytest.mark.parametrize("B", K.WINDOW_B)
@pytest.mark.parametrize("t", K.WINDOW_THRESHOLDS)
def test_window_frames_bite(t, B):
    """The condition that keeps the GPU tests from passing by accident: every single-token mistake of K.WINDOW_MUTANTS loses
    at least one pinned pair at every site it applies to, taken over the families -- per threshold and per frame size.

    Two mutants lose nothing on any frame, and cannot (K.WINDOW_UNKILLABLE says why): wmax_no_plus1 pulls the left bound in by
    (1 - t) px, less than the smallest margin of 1 px; no_trunc_slack removes a margin that nothing needs, because the link
    scans take the window and the IoU from the same truncated box.  They are asserted to lose NOTHING, so that a change of
    the model or the frames that makes them bite is noticed.  'nomargin' (margins removed, nothing moved inward) is printed
    only: whether it loses a pair hangs on one float32 rounding."""
    lost = {}
    for family in K.WINDOW_FAMILIES:
        for site in K.WINDOW_SITES:
            boxes, pairs = K.window_frame(t, B, family, K.WINDOW_SEED, site == 'xwindow')
            for mode in K.WINDOW_MODES:
                if mode in ('kernel', 'nomargin') or site in K.WINDOW_MUTANTS[mode]:
                    n = K.window_lost(boxes, pairs, t, site, mode, family == 'frac')[1]
                    lost.setdefault((site, mode), {})[family] = n
    for (site, mode), by in sorted(lost.items()):
        print('t = %g B = %d %-8s %-15s lost: %s' % (t, B, site, mode, ' '.join('%s=%d' % kv for kv in by.items())))
        total = sum(by.values())
        if mode == 'kernel' or mode in K.WINDOW_UNKILLABLE:
            assert total == 0, (site, mode, by)
        elif mode != 'nomargin':
            assert total >= 1, (site, mode, by)
    # which family pins what: the clamp at bucket 255 only 'top', cum[b1 + 1] 'top' and 'coarse' (unit buckets hide it behind
    # the 2 px margin), the word rounding every family with a word boundary, one pixel inward at re-scoring only 'frac'
    assert lost[('adj', 'clamp254')]['top'] >= 1 and lost[('adj', 'cum_b1')]['coarse'] >= 1 and lost[('adj', 'cum_b1')]['unit'] == 0
    for family in ('unit', 'wmaxcap', 'coarse', 'frac', 'top'):
        assert lost[('adj', 'floor_w1')][family] >= 1 and lost[('adj', 'ceil_w0')][family] >= 1
        assert all(lost[(site, 'own_width_left')][family] >= 1 for site in K.WINDOW_SITES)
    assert lost[('xwindow', 'in1')]['frac'] >= 1 and lost[('link', 'in1')]['frac'] >= 1 and lost[('adj', 'in1')]['frac'] >= 1
