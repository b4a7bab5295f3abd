"""The two statements of the IoU threshold test in numpy, and a search for the box pairs on which they could differ (no GPU,
no product code).

The reference decides a pair by RN(inter / uni) >= t32 in float32 (utils/nms.pyx as pair_pred in csrc/nms_kernels.hpp
restates it): quotient().  The divide-free hot paths take the sign of r = fma(-t32, uni, inter) and fall back to the
quotient inside a narrow band below zero -- pred_regular's r >= -(2^-21 * t32) * uni, pred_margins' second margin
qlo = fma(-t_lo, uni, inter) >= 0 with t_lo = t32 * (1 - 2^-21): margins().

A pair at a threshold is
  UP      q >= t32 and r < 0: only the quotient says "suppress" (the real quotient lies within half an ulp below t32)
  BAND    q <  t32 and -bnd <= r < 0: the fallback runs and must say "keep"; BELOW1 = those with q == nextafter(t32, 0)
  ABOVE1  q == nextafter(t32, 2)
  ZERO    r == 0 exactly
search_integer() / search_fractional() find such pairs (nested boxes, seeded, vectorised); reach_family() and
unit_family() build in closed form the pairs that sit exactly on the bound of the x-reach culling and on threshold 1.
grid_frame() / band_frame() put pairs into frames, every pair in a cell of its own.
"""
from fractions import Fraction

import numpy as np

F32 = np.float32
THRESHOLDS = (0.1, 0.25, 0.3, 0.45, 0.5, 0.7, 0.75, 0.9)       # searched
EXACT = (0.25, 0.5, 0.75)                                      # float32 holds them exactly
POW2 = (0.25, 0.5)                                             # ... and r is then exact near the edge: no UP pair exists
ONLY_EXACT_UP = (0.1,)                                         # every UP pair whose union fits a cell has IoU exactly t
FAMILY_THRESHOLDS = THRESHOLDS + (1e-3, 1.0)                   # closed-form families
CLASSES = ('UP', 'BAND', 'BELOW1', 'ABOVE1', 'ZERO')
BAND_REL = 2.0 ** -21

INT_CELL, INT_BOX = 4096, 3900          # integer form: 16 x 16 cells fill the u16 plane; boxes leave a strip for fillers
FRAC_CELL, FRAC_BOX = 250, 236          # fractional form (pixels): 8 x 8 cells below 2000 px
FRAC_UNIT = 16                          # coordinates are multiples of 2^-4 (the fixture stores them in these units)


def thresh_to_f32(t):
    """csrc/vdet_capi.hip thresh_to_f32: the smallest float32 f with (double)f >= t."""
    f = F32(t)
    if float(f) < float(t):
        f = np.nextafter(f, F32(np.inf))
    return f


def quotient(a, b):
    """(inter, uni, q) in float32, a = the "i" box, b = the "j" box, [..., 4]; the operation order of utils/nms.pyx."""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
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
        inter = (w * h).astype(F32)
        ai = ((a[..., 2] - a[..., 0]) + one) * ((a[..., 3] - a[..., 1]) + one)
        aj = ((b[..., 2] - b[..., 0]) + one) * ((b[..., 3] - b[..., 1]) + one)
        uni = ((ai + aj) - inter).astype(F32)
        q = (inter / uni).astype(F32)
    return inter, uni, q


def real_quotient(a, b):
    """inter / uni of one pair as a Fraction (float32 coordinates are dyadic rationals: exact)."""
    a = [Fraction(float(x)) for x in np.asarray(a, F32)]
    b = [Fraction(float(x)) for x in np.asarray(b, F32)]
    w = max(Fraction(0), min(a[2], b[2]) - max(a[0], b[0]) + 1)
    h = max(Fraction(0), min(a[3], b[3]) - max(a[1], b[1]) + 1)
    inter = w * h
    uni = (a[2] - a[0] + 1) * (a[3] - a[1] + 1) + (b[2] - b[0] + 1) * (b[3] - b[1] + 1) - inter
    return inter / uni


def _rn_f32(x):
    """A Fraction rounded once (to nearest, ties to even) to float32."""
    if x == 0:
        return F32(0)
    s, x = (-1, -x) if x < 0 else (1, x)
    e = x.numerator.bit_length() - x.denominator.bit_length() - 24
    while x >= Fraction(2) ** (e + 24):
        e += 1
    while x < Fraction(2) ** (e + 23):
        e -= 1
    e = max(e, -149)                                  # subnormals keep the exponent of the smallest normal's ulp
    y = x / Fraction(2) ** e
    n = y.numerator // y.denominator
    rem = y - n
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and n & 1):
        n += 1
    return F32(s * float(n) * 2.0 ** e)


def fma_f32(a, b, c):
    """RN_f32(a * b + c) with ONE rounding, elementwise on float32 arrays.  The product of two float32 is exact in
    float64 (24 + 24 <= 53 bits).  The float64 sum is exact whenever its TwoSum error term is zero -- always so near the
    threshold, where c cancels most of the product -- and an exact float64 rounds once to float32.  The remaining elements
    (operands of very different magnitude) are redone in rational arithmetic."""
    a, b, c = np.broadcast_arrays(np.asarray(a, F32), np.asarray(b, F32), np.asarray(c, F32))
    p = a.astype(np.float64) * b.astype(np.float64)
    c64 = c.astype(np.float64)
    s = p + c64
    bb = s - p
    err = (p - (s - bb)) + (c64 - bb)
    out = np.array(s.astype(F32))
    for i in np.flatnonzero((err != 0) & np.isfinite(s)):
        out.flat[i] = _rn_f32(Fraction(float(a.flat[i])) * Fraction(float(b.flat[i])) + Fraction(float(c.flat[i])))
    return out


def t_lo_of(t32):
    """pred_margins' second threshold exactly as the kernels write it (both operations in float32)."""
    return F32(t32) * (F32(1.0) - F32(4.76837158203125e-7))


def margins(inter, uni, t32):
    """(r, qlo): the single-rounded fma(-t32, uni, inter) and fma(-t_lo, uni, inter)."""
    t32 = np.asarray(t32, F32)
    return fma_f32(-t32, uni, inter), fma_f32(-t_lo_of(t32), uni, inter)


def band_of(uni, t32, rel=BAND_REL):
    """pred_regular's bnd = t32e * uni in float32, t32e = t32 * 2^-21 (rel: what another band constant would give)."""
    return (np.asarray(t32, F32) * F32(rel)) * np.asarray(uni, F32)


def classify(a, b, t):
    """Boolean masks by class name, plus 'sup' (the reference's decision q >= t32), for pairs a, b [n, 4] at threshold t."""
    t32 = thresh_to_f32(t)
    inter, uni, q = quotient(a, b)
    r, qlo = margins(inter, uni, t32)
    sup = q >= t32
    band = ~sup & (r < 0) & (r >= -band_of(uni, t32))
    return dict(sup=sup, UP=sup & (r < 0), BAND=band, BELOW1=band & (q == np.nextafter(t32, F32(0))),
                ABOVE1=q == np.nextafter(t32, F32(2)), ZERO=r == 0, r=r, qlo=qlo, q=q, uni=uni, inter=inter)


def decide_fma(a, b, t, rel=BAND_REL, fallback=True):
    """What a divide-free site decides: r >= 0, or the quotient inside the band of width rel * t32 * uni below zero.
    fallback=False: the sign of r alone.  With the defaults it is the kernels' rule."""
    t32 = thresh_to_f32(t)
    inter, uni, q = quotient(a, b)
    r, _ = margins(inter, uni, t32)
    hit = r >= 0
    if fallback:
        hit = hit | ((r >= -band_of(uni, t32, rel)) & (q >= t32))
    return hit


def decide_margins(a, b, t):
    """The two-margin form (pred_margins): sign(r) clear, or sign(qlo) clear and the quotient says yes."""
    t32 = thresh_to_f32(t)
    inter, uni, q = quotient(a, b)
    r, qlo = margins(inter, uni, t32)
    return (r >= 0) | ((qlo >= 0) & (q >= t32))


# ---------------------------------------------------------------------------------------------------------------------
# the pair search: nested boxes, outer W x H, inner w x h with w = rint(t32 * W * H / h), in "units" (1 for the integer
# form, 1/16 px for the fractional one -- a size of n units is a coordinate difference of n - 16 there, the +1 of the area)
# ---------------------------------------------------------------------------------------------------------------------
QUOTA = dict(UP=20, BAND=12, BELOW1=6, ABOVE1=16, ZERO=16)


def _nested_candidates(rng, t32, lo, hi, hmin, ndraw):
    W = rng.randint(lo, hi + 1, ndraw)
    H = rng.randint(lo, hi + 1, ndraw)
    out = []
    for Wk, Hk in zip(W, H):
        h = np.arange(max(hmin, int(np.ceil(float(t32) * Hk)) - 1), Hk + 1)
        w = np.rint(float(t32) * Wk * Hk / h).astype(np.int64)
        ok = (w >= hmin) & (w <= Wk)
        h, w = h[ok], w[ok]
        # cheap screen in float64 before the exact classification: |inter - t * uni| within 2^-19 * t * uni
        res = w * h - float(t32) * Wk * Hk
        near = np.abs(res) <= 2.0 ** -19 * float(t32) * Wk * Hk
        h, w = h[near], w[near]
        if h.size:
            out.append(np.stack([np.full(h.size, Wk), np.full(h.size, Hk), w, h], 1))
    return np.concatenate(out) if out else np.zeros((0, 4), np.int64)


def _nested_boxes(rng, whwh, unit, origin_max):
    """Cell-local float32 boxes of nested candidates [n, (W, H, w, h)] in units: the outer box starts at a random origin
    below origin_max units, the inner box at a random offset inside it."""
    n = whwh.shape[0]
    W, H, w, h = whwh.T
    ox, oy = rng.randint(0, origin_max + 1, n), rng.randint(0, origin_max + 1, n)
    dx, dy = (rng.rand(n) * (W - w + 1)).astype(np.int64), (rng.rand(n) * (H - h + 1)).astype(np.int64)
    a = np.stack([ox, oy, ox + W - unit, oy + H - unit], 1)
    b = np.stack([ox + dx, oy + dy, ox + dx + w - unit, oy + dy + h - unit], 1)
    return (a / float(unit)).astype(F32), (b / float(unit)).astype(F32)


def _search(t, seed, lo, hi, unit, origin_max, max_draws, chunk=200):
    """Pairs of every class at threshold t: {class: (a [n, 4], b [n, 4])}.  UP pairs whose real quotient is the decimal
    threshold itself (IoU exactly 3/10) are kept apart as 'UPEXACT': 4 of them, more where the others fall short of the quota;
    the first 16 UP pairs with r below -2^-25 * t32 * uni, of either kind, as 'UPDEEP'."""
    rng = np.random.RandomState(seed)
    t32 = thresh_to_f32(t)
    dec = Fraction(str(t))
    got = {k: ([], []) for k in CLASSES + ('UPEXACT', 'UPDEEP')}
    quota = dict(QUOTA, UPEXACT=QUOTA['UP'], UPDEEP=16)
    if t not in EXACT:
        quota['ZERO'] = 0
    if t in POW2:
        quota['UP'] = quota['UPEXACT'] = quota['UPDEEP'] = 0
    if t in ONLY_EXACT_UP:
        quota['UP'] = quota['UPDEEP'] = 0

    def full():
        return all(len(got[k][0]) >= quota[k] for k in quota)
    for _ in range(0, max_draws, chunk):
        cand = _nested_candidates(rng, t32, lo, hi, unit, chunk)
        if not cand.shape[0]:
            continue
        a, b = _nested_boxes(rng, cand, unit, origin_max)
        c = classify(a, b, t)
        taken = np.zeros(a.shape[0], bool)
        for k in ('UP', 'BELOW1', 'BAND', 'ABOVE1', 'ZERO'):
            for i in np.flatnonzero(c[k] & ~taken):
                kk = k
                if k == 'UP' and c['r'][i] < -band_of(c['uni'][i], t32, 2.0 ** -25) and len(got['UPDEEP'][0]) < quota['UPDEEP']:
                    kk = 'UPDEEP'       # (outside a band of 2^-25: the pairs that tell a band constant that is too small)
                elif k == 'UP' and real_quotient(a[i], b[i]) == dec:
                    kk = 'UPEXACT'
                if len(got[kk][0]) < quota[kk]:
                    got[kk][0].append(a[i]); got[kk][1].append(b[i])
                    taken[i] = True
        if full():
            break
    nex = max(4, QUOTA['UP'] - len(got['UP'][0]))
    got['UPEXACT'] = (got['UPEXACT'][0][:nex], got['UPEXACT'][1][:nex])
    return {k: (np.asarray(v[0], F32).reshape(-1, 4), np.asarray(v[1], F32).reshape(-1, 4)) for k, v in got.items()}


def search_integer(t, seed, max_draws=100000):
    """Integer form: integer coordinates, cell-local in [0, INT_BOX), union between about 1e6 and 2^24."""
    return _search(t, seed, 1000, INT_BOX - 4, 1, 3, max_draws)


def search_fractional(t, seed, max_draws=100000):
    """Fractional form: coordinates are multiples of 2^-4, cell-local in [0, FRAC_BOX) px; sizes of 62 .. 234 px make areas
    of 1e6 .. 1.4e7 units of 2^-8 (smaller boxes have too few distinct quotients next to most thresholds).  Coordinates
    below 2048 px on this grid have 15 significant bits, so a translation by whole pixels is exact in float32 and changes
    no rounding (grid_frame checks it at the final positions)."""
    return _search(t, seed, 1000, (FRAC_BOX - 2) * FRAC_UNIT, FRAC_UNIT, FRAC_UNIT - 1, max_draws)


def reach_family(t, seed, n=24, wmax=60000):
    """Reach-tight pairs in closed form, integer coordinates with y1 = 0: a box of width W and height H and an inner box of
    width t * W and full height, flush right.  The inner box starts exactly (1 - t) * W to the right of the outer one --
    the bound of reach_table_kernel -- and the outer box is exactly wrow / t wide, the bound of the adjacency kernel's
    left window; the real IoU is the threshold.  Even entries choose W first (a multiple of 20, of 1000 for 1e-3), odd
    entries the inner width first (the mirror: a multiple of the threshold's numerator, W = wrow / t)."""
    rng = np.random.RandomState(seed)
    tf = Fraction(str(t))
    a, b = [], []
    for k in range(n):
        if k % 2 == 0:
            step = 20 * tf.denominator // int(np.gcd(20, tf.denominator))
            W = step * int(rng.randint(1, wmax // step + 1))
        else:       # (every fourth entry is small: a narrow row whose left window is a few pixels)
            kmax = max(1, wmax // tf.denominator // (1 if k % 4 == 1 else 50))
            W = tf.denominator * int(rng.randint(1, kmax + 1))
        w = tf * W
        assert w.denominator == 1 and 1 <= w <= W <= wmax
        w, H = int(w), int(rng.randint(1, 41))
        x0 = int(rng.randint(0, 65536 - W))
        a.append([x0, 0, x0 + W - 1, H - 1])
        b.append([x0 + W - w, 0, x0 + W - 1, H - 1])
    return np.asarray(a, F32), np.asarray(b, F32)


def unit_family(seed, n=12, tries=4000):
    """Threshold 1: identical boxes, and fractional near-duplicates whose three areas (both boxes, the intersection) round
    to one float32, so that the quotient is exactly 1 although the boxes differ.  y1 = 0."""
    rng = np.random.RandomState(seed)
    W = rng.randint(100, 60000, n); H = rng.randint(1, 41, n); x0 = rng.randint(0, 5000, n)
    a = np.stack([x0, 0 * x0, x0 + W - 1, H - 1], 1).astype(F32)
    same = (a, a.copy())
    # near-duplicates: a wide box whose right edge moves by one ulp (2^-8 at 32768 .. 65535) -- kept when the areas round equal
    x2 = (rng.randint(60000, 65535, tries) + rng.randint(0, 256, tries) / 256.0).astype(F32)
    h = (rng.randint(0, 40 * 16, tries) / 16.0).astype(F32)
    big = np.stack([np.zeros(tries, F32), np.zeros(tries, F32), x2, h], 1)
    small = big.copy()
    small[:, 2] = np.nextafter(x2, F32(0))
    inter, uni, q = quotient(big, small)
    ok = np.flatnonzero((q == 1) & (inter == uni))[:n]
    return same, (big[ok], small[ok])


# ---------------------------------------------------------------------------------------------------------------------
# frames
# ---------------------------------------------------------------------------------------------------------------------
def pair_scores(npairs, nfill, seed):
    """Three score columns for 2 * npairs pair boxes (pair k = rows 2k, 2k + 1) followed by nfill fillers:
    0: the first box of each pair directly above the second (s_k and the next float below it, s_k strictly decreasing),
    1: the roles swapped,  2: a tie-free random permutation.  Fillers score below every pair in columns 0 and 1."""
    rng = np.random.RandomState(seed)
    B = 2 * npairs + nfill
    s = np.zeros((B, 3), F32)
    sk = (F32(0.99) - np.arange(npairs, dtype=F32) * F32(1.0 / 1024))
    assert npairs < 900 and np.all(np.diff(sk) < 0)
    below = np.nextafter(sk, F32(0))
    s[0:2 * npairs:2, 0], s[1:2 * npairs:2, 0] = sk, below
    s[0:2 * npairs:2, 1], s[1:2 * npairs:2, 1] = below, sk
    s[2 * npairs:, 0] = s[2 * npairs:, 1] = (rng.permutation(nfill) + 1).astype(F32) / F32(16384)
    s[:, 2] = (rng.permutation(B) + 1).astype(F32) / F32(B + 1)
    return s


def _order_pairs(a, b):
    """Rows 2k, 2k + 1 of the result are pair k; the box with the smaller x1 comes first for even k, second for odd k."""
    n = a.shape[0]
    lo_first = (a[:, 0] <= b[:, 0]) == (np.arange(n) % 2 == 0)
    first = np.where(lo_first[:, None], a, b)
    second = np.where(lo_first[:, None], b, a)
    out = np.empty((2 * n, 4), F32)
    out[0::2], out[1::2] = first, second
    return out


def cell_offsets(rng, n, cell, side):
    """[n, 4] translations (whole pixels) into n distinct cells of a side x side grid, in random order."""
    assert n <= side * side
    cells = rng.permutation(side * side)[:n]
    off = np.stack([cells % side, cells // side], 1).astype(F32) * F32(cell)
    return np.concatenate([off, off], 1)


def strip_fillers(rng, n, cell, box, side):
    """n small integer boxes inside the strips [box + 1, cell) that the pair boxes (all coordinates below box) leave free
    at the right of every cell: they overlap no pair box."""
    fc = rng.randint(0, side * side, n)
    strip = cell - box - 1
    fx = (fc % side) * cell + box + 1 + rng.randint(0, strip // 2, n)
    fy = (fc // side) * cell + rng.randint(0, cell - strip, n)
    fw, fh = rng.randint(1, strip // 2 + 1, n), rng.randint(1, strip, n)
    return np.stack([fx, fy, fx + fw - 1, fy + fh - 1], 1).astype(F32)


def grid_frame(a, b, cell, box, nfill, seed, side):
    """Boxes [2n + nfill, 4]: pair k translated into a cell of its own of a side x side grid (no two pairs overlap),
    fillers in the strips that the pairs leave free.  The translation is by whole pixels and is checked to change no
    float32 result of the pair."""
    assert max(a[:, 2:].max(), b[:, 2:].max()) < box
    rng = np.random.RandomState(seed)
    off4 = cell_offsets(rng, a.shape[0], cell, side)
    ta, tb = (a + off4).astype(F32), (b + off4).astype(F32)
    for x, y in zip(quotient(a, b), quotient(ta, tb)):
        assert np.array_equal(x, y)
    assert np.array_equal(ta - off4, a) and np.array_equal(tb - off4, b)
    return np.concatenate([_order_pairs(ta, tb), strip_fillers(rng, nfill, cell, box, side)], 0)


def band_frame(a, b, nfill, seed, band=64):
    """Reach-tight pairs (y1 = 0, heights below band) one per horizontal band, and nfill narrow filler boxes in bands of
    their own, spread over the whole x range so that the frame's x-buckets and 64-rank words are many and the reach
    window really culls."""
    n = a.shape[0]
    rng = np.random.RandomState(seed)
    assert (n + nfill) * band <= 65536 and max(a[:, 3].max(), b[:, 3].max()) < band
    bands = rng.permutation(n + nfill)
    off = np.zeros((n, 4), F32)
    off[:, 1] = off[:, 3] = bands[:n] * band
    fx = rng.randint(0, 65000, nfill)
    fy = bands[n:] * band
    fw, fh = rng.randint(1, 30, nfill), rng.randint(1, band, nfill)
    fill = np.stack([fx, fy, fx + fw - 1, fy + fh - 1], 1).astype(F32)
    return np.concatenate([_order_pairs((a + off).astype(F32), (b + off).astype(F32)), fill], 0)


def load_pairs(path):
    """The fixture as float32 pixel coordinates: {('int' | 'frac' | 'reach', t): (a, b)} and ('unit', 'same' | 'near')."""
    z = np.load(path)
    out = {}
    for t in FAMILY_THRESHOLDS:
        for form, unit in (('int', 1), ('frac', FRAC_UNIT), ('reach', 1)):
            k = '%s_%g' % (form, t)
            if k + '_a' in z.files:
                out[(form, t)] = ((z[k + '_a'] / F32(unit)).astype(F32), (z[k + '_b'] / F32(unit)).astype(F32))
    out[('unit', 'same')] = (z['unit_same_a'], z['unit_same_a'].copy())
    out[('unit', 'near')] = (z['unit_near_a'], z['unit_near_b'])
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the x-reach culling: frames on which the reach table decides, and a model of the table
# ---------------------------------------------------------------------------------------------------------------------
def reach_frame(t, B, seed, band=64):
    """A frame [B, 4] of integer boxes built RANK BY RANK in the x1 order (all x1 distinct), on which the reach table decides
    the fate of a suppressed pair per 64-rank block c = 1 .. (B - 1) // 64:
      - the pair's inner box is the FIRST box of block c (rank 64 c), so first[c] is its x1;
      - the outer box is the last box of block c - 1 and has the largest reach of that block (and, widths growing with c,
        of the widest quartile of its 256-rank tile), so reach[c - 1] is its own x1 + (1 - t) * W (+ margin);
      - no other box starts between the two.
    The inner box is flush right, full height and t * W wide, its x offset exactly (1 - t) * W; where thresh_to_f32 rounds
    the threshold up such a pair is not suppressed and the inner box is one pixel wider (offset (1 - t) * W - 1).
    Pairs whose block is a multiple of 4 have their boxes in different 256-rank tiles.  Everything else is narrow fillers
    in y bands of their own.  Returns (boxes, pair rows [m, 2]): pair k is rows 2k and 2k + 1, the fillers follow."""
    rng = np.random.RandomState(seed)
    tf = Fraction(str(t))
    step = 20 * tf.denominator // int(np.gcd(20, tf.denominator))
    m = (B - 1) // 64
    span_max = min(4500.0, float(1 - tf) * 20000.0)
    xs, ws, hs, ys = [], [], [], []          # by rank
    pair_ranks = []
    x = 0
    for c in range(1, m + 1):
        for i in range(63 if c == 1 else 62):                      # fillers up to the outer box
            xs.append(x + 1 + i); ws.append(int(rng.randint(1, 31))); hs.append(int(rng.randint(1, band)))
        W = step * max(1, int(round(span_max * (0.5 + 0.5 * c / m) / float(1 - tf) / step)))
        w = int(tf * W)
        assert tf * W == w
        X = x + 300
        H = int(rng.randint(1, 41))
        outer = np.array([X, 0, X + W - 1, H - 1], F32)
        if not classify(outer[None], np.array([[X + W - w, 0, X + W - 1, H - 1]], F32), t)['sup'][0]:
            w += 1                                                 # (t32 > t: IoU exactly t is not suppressed)
        inner = np.array([X + W - w, 0, X + W - 1, H - 1], F32)
        assert classify(outer[None], inner[None], t)['sup'][0]
        pair_ranks.append((len(xs), len(xs) + 1))
        assert len(xs) == 64 * c - 1
        xs += [X, X + W - w]; ws += [W, w]; hs += [H, H]
        x = X + W - w
    for i in range(B - len(xs)):
        xs.append(x + 1 + i); ws.append(int(rng.randint(1, 31))); hs.append(int(rng.randint(1, band)))
    xs, ws, hs = np.asarray(xs), np.asarray(ws), np.asarray(hs)
    assert np.all(np.diff(xs) > 0) and (xs + ws).max() <= 65535
    is_pair = np.zeros(B, bool)
    is_pair[np.asarray(pair_ranks).ravel()] = True
    y = np.zeros(B, np.int64)
    y[np.asarray(pair_ranks)[:, 0]] = y[np.asarray(pair_ranks)[:, 1]] = np.arange(m) * band
    y[~is_pair] = (m + rng.permutation(B - 2 * m)) * band
    assert y.max() + band <= 65536
    boxes = np.stack([xs, y, xs + ws - 1, y + hs - 1], 1).astype(F32)
    # rows: pair k at rows 2k, 2k + 1 (the outer box first for even k, the inner one for odd k), then the fillers, shuffled
    pr = np.asarray(pair_ranks)
    pr[1::2] = pr[1::2, ::-1]
    ranks = np.concatenate([pr.ravel(), rng.permutation(np.flatnonzero(~is_pair))])
    return boxes[ranks], np.arange(2 * m).reshape(m, 2)


REACH_SEEDS = (11, 12)          # the reach frames every volume of tests/test_knife_edge_gpu.py holds
REACH_MODES = dict(kernel=None, nomargin=0.0, tight1=1.0, tight2=2.0)


def reach_model(boxes, t, pairs, mode, lists):
    """How many of the frame's pairs (rows [m, 2]) a reach bound would cull -- never evaluate -- although the reference
    suppresses them.  mode 'kernel' is reach_table_kernel's bound x1 + (1 - t) * w * 1.001 + 1 in float32; 'nomargin' the
    bound without the margin, 'tight1' / 'tight2' one / two pixels tighter still.  lists=False: the block test of
    iou_bits_sym_kernel and the adjacency kernel (first[c] <= reach[r], and the tile-pair test before it); lists=True:
    graph_lists_kernel's walk of one (256-rank tile, width quartile) item over the blocks to its right, which ends at the
    first block beyond the item's reach."""
    boxes = np.asarray(boxes, F32)
    B = boxes.shape[0]
    order = np.argsort(boxes[:, 0], kind='stable')
    rank = np.empty(B, np.int64)
    rank[order] = np.arange(B)
    xb = boxes[order]
    omt = F32(max(0.0, 1.0 - float(t)))
    w = (xb[:, 2] - xb[:, 0]) + F32(1)
    if mode == 'kernel':
        reach = ((xb[:, 0] + (omt * w) * F32(1.001)) + F32(1)).astype(F32)
    else:
        reach = ((xb[:, 0] + omt * w) - F32(REACH_MODES[mode])).astype(F32)
    nb = (B + 63) // 64
    first = xb[0::64, 0]
    breach = np.array([reach[64 * r:64 * r + 64].max() for r in range(nb)], F32)
    sup = classify(boxes[pairs[:, 0]], boxes[pairs[:, 1]], t)['sup']
    lost = 0
    for k in np.flatnonzero(sup):
        p, q = sorted(rank[pairs[k]])
        r, c = p >> 6, q >> 6
        if not lists:
            rt, ct = r >> 2, c >> 2
            tile_cut = ct > rt and first[4 * ct] > breach[4 * rt:4 * rt + 4].max()
            lost += bool(tile_cut or (c > r and first[c] > breach[r]))
        else:
            mt = p >> 8
            rows = np.arange(256 * mt, min(B, 256 * mt + 256))
            wd = xb[rows, 2] - xb[rows, 0]
            slot = np.empty(rows.size, np.int64)
            slot[np.lexsort((rows, wd))] = np.arange(rows.size)
            mine = slot >> 6 == slot[p - 256 * mt] >> 6
            qreach = reach[rows[mine]].max()
            last = 4 * mt
            while last + 1 < nb and ((last + 1) >> 2 == mt or first[last + 1] <= qreach):
                last += 1
            lost += bool(c > last)
    return lost


# ---------------------------------------------------------------------------------------------------------------------
# the x-bucket windows: frames whose pinned pairs sit on the window's edge and on a 64-rank word boundary, and a model of
# the three dialects of the window (csrc/nms_kernels.hpp adj_build_kernel and xwindow, csrc/track_kernels.hpp link scans)
# ---------------------------------------------------------------------------------------------------------------------
WINDOW_FAMILIES = ('unit', 'top', 'wmaxcap', 'coarse', 'frac', 'flat')
WINDOW_THRESHOLDS = (0.3, 0.5, 0.7)
WINDOW_SITES = ('adj', 'xwindow', 'link')
WINDOW_B = (322, 642, 1026, 2114)      # B - 2 a multiple of 64: the two partners in bucket 255 of 'top' are the whole last word
# (322 / 642: the two adj_build_kernel instantiations; 1026: beyond the link table's 1024; 2114: a list of more than 2048)
WINDOW_SEED = 7                 # the seed of the frames the suites share
WINDOW_W = 100                  # the outer boxes' width: t * W is an integer for every searched threshold
# mutant -> the sites it applies to.  'nomargin' is reported only (whether it loses a pair hangs on one float32 rounding).
WINDOW_MUTANTS = dict(own_width_left=WINDOW_SITES, in1=WINDOW_SITES, cum_b1=WINDOW_SITES, floor_w1=('adj',), ceil_w0=('adj',),
                      clamp254=WINDOW_SITES, wmax_no_plus1=WINDOW_SITES, no_trunc_slack=('link',))
# Mutants no frame can kill, with the reason (tests/test_knife_edge_cpu.py asserts that they lose nothing here either):
#   wmax_no_plus1   a left partner j satisfies x1_c - x1_j <= (1 - t) w_j <= (1 - t) (wmax' + 1) < (1 - t) wmax' + 1 with
#                   wmax' = max(x2 - x1): the missing + 1 pulls the bound in by (1 - t) < 1 px, less than the smallest margin
#                   (1 px at xwindow, 2 px at the other two sites)
#   no_trunc_slack  the link scans take window AND IoU from the truncated current box, so truncation opens no gap between
#                   the two; the bound is exact in real arithmetic and the 0.2 % of omt covers the float32 rounding
WINDOW_UNKILLABLE = ('wmax_no_plus1', 'no_trunc_slack')
WINDOW_MODES = ('kernel', 'nomargin') + tuple(WINDOW_MUTANTS)


def iou64(a, b):
    """The re-scoring IoU: float64 arithmetic on float32 coordinates, + 1 convention (oracle.iou on one pair)."""
    a, b = np.asarray(a, F32).astype(np.float64), np.asarray(b, F32).astype(np.float64)
    w = min(a[2], b[2]) - max(a[0], b[0]) + 1.0
    h = min(a[3], b[3]) - max(a[1], b[1]) + 1.0
    inter = max(w, 0.0) * max(h, 0.0)
    return inter / ((a[2] - a[0] + 1.0) * (a[3] - a[1] + 1.0) + (b[2] - b[0] + 1.0) * (b[3] - b[1] + 1.0) - inter)


def window_partner(query, partner, t, site):
    """Is `partner` a true partner of `query` by the referee of the site: the reference's float32 quotient for the
    suppression graph ('adj'), the oracle's link rule on the TRUNCATED current box ('link'), float64 IoU > t for
    re-scoring ('xwindow')."""
    query, partner = np.asarray(query, F32), np.asarray(partner, F32)
    if site == 'xwindow':
        return bool(iou64(query, partner) > t)
    if site == 'link':
        query = np.trunc(query)
    return bool(classify(query[None], partner[None], t)['sup'][0])


def _fill_x(ra, xa, rb, xb, g):
    """x1 of the rb - ra - 1 filler ranks strictly between two anchored ranks: on the grid g, strictly inside (xa, xb), in
    ascending order (fillers may share an x1; an anchored box keeps its x1 to itself)."""
    n = rb - ra - 1
    if n <= 0:
        return []
    inner = int(round((xb - xa) / g)) - 1
    assert inner >= 1, (ra, xa, rb, xb)
    return [xa + g * (1 + (i * inner) // n) for i in range(n)]


def window_band(B):
    """The height of a y band: every box has a band of its own below 65536."""
    return 64 if B <= 1000 else 16


def window_frame(t, B, family, seed, strict=False, band=None):
    """A regular frame [B, 4] built RANK BY RANK in the x1 order whose pinned pairs sit on the edge of the x-bucket window
    and on a 64-rank word boundary.  A pair is an outer box O of width W = 100 and an inner box I, flush right, full height,
    t * W wide: I starts exactly (1 - t) * W right of O, the bound of the window on both sides.  Where the exact-t pair does
    not count -- classify() says "keep" because thresh_to_f32 rounds the threshold up, or strict=True, the float64
    IoU > t of re-scoring, where it never counts -- I is one grid step wider.  Every pinned box has an x1 of its own;
    everything else is narrow fillers (at most 30 wide) in y bands of their own, which may share an x1 with each other.

    unit     x1 range exactly 256 (scale == 1.0, one pixel per bucket).  O is the LAST rank of a word, I the FIRST rank of a
             later word (64 or more filler ranks between them): one pair pins the right side from O (hi, cum[b1 + 1],
             (r1 + 63) >> 6) and the left side from I (lo, r0 >> 6).  One filler is 3 W wide, so w_c / t decides on the left.
    wmaxcap  the same without the wide filler: the outer boxes are the frame's widest and min(wmax, .) decides on the left.
    frac     unit on a grid of quarter pixels (not a kFlagU16 frame): O on whole pixels, I a quarter wider where the exact
             pair does not count, xmin on .75 so that I starts exactly on a bucket's edge.
    top      unit scale; partners I with x1 == xmax and x1 == xmax - 1 (both in bucket 255, the whole last word, hi beyond
             xmax) and the mirror image: partners O with x1 == xmin and xmin + 1, lo left of xmin.
    coarse   x1 range 4096 (16 px per bucket, wider than any margin).  Right pins: I alone in its bucket, on the bucket's
             first pixel, first rank of a word.  Left pins: O alone in its bucket, on its last pixel, last rank of a word.
    flat     every x1 equal (scale == 0, one bucket): I flush LEFT.  Nothing can be culled; the frame checks the path.
    Returns (boxes, pair rows [m, 2] = (row of O, row of I)): pair k is rows 2k, 2k + 1 (O first for even k), then fillers."""
    assert family in WINDOW_FAMILIES and B >= 322 and (B - 2) % 64 == 0
    band = window_band(B) if band is None else band
    rng = np.random.RandomState(seed)
    tf = Fraction(str(t))
    W = WINDOW_W
    g = 0.25 if family == 'frac' else 1.0
    assert (tf * W).denominator == 1
    span = 4096.0 if family == 'coarse' else 256.0
    xmin = 1000.0 - (0.25 if family == 'frac' else 0.0)
    xmax = xmin + span
    heights = {}

    def pair_at(k, xo=None, xi=None, left=False):
        """(O, I) as (x1, x2) from the x1 of one of them; the smallest I that counts."""
        H = heights.setdefault(k, int(rng.randint(8, min(41, band))))
        w = float(tf * W)
        while True:
            o = xo if xo is not None else (xi if left else xi - (W - w))
            O = np.array([o, 0, o + W - 1, H - 1], F32)
            I = np.array([o, 0, o + w - 1, H - 1] if left else [o + W - w, 0, o + W - 1, H - 1], F32)
            if (iou64(O, I) > t) if strict else bool(classify(O[None], I[None], t)['sup'][0]):
                return (float(O[0]), float(O[2])), (float(I[0]), float(I[2]))
            w += g

    pins = {}           # rank -> (x1, x2, pair, is_outer)
    anchors = {}        # rank -> x1 of a filler that must stand exactly there
    wide = None         # rank of the 3 W wide filler

    def pin(k, ro, ri, O, I):
        assert ro not in pins and ri not in pins and ro not in anchors and ri not in anchors
        pins[ro] = (O[0], O[1], k, True)
        pins[ri] = (I[0], I[1], k, False)

    if family == 'flat':
        x1 = np.full(B, xmin)
        for k in range(3):
            O, I = pair_at(k, xo=xmin, left=True)
            pin(k, 2 * k, 2 * k + 1, O, I)
    elif family in ('unit', 'wmaxcap', 'frac'):
        xo = float(np.ceil(xmin + 8))                                # (frac: O on whole pixels)
        for k in range(min(3, (B - 3) // 128)):
            O, I = pair_at(k, xo=xo)
            pin(k, 64 * (2 * k + 1) - 1, 64 * (2 * k + 2), O, I)
            xo = float(np.ceil(I[0] + 6))
        assert xo < xmax - 4
        wide = None if family == 'wmaxcap' else 5
    elif family == 'top':
        m = (B - 2) // 64 - 1
        Oa, Ia = pair_at(0, xi=xmax)
        Ob, Ib = pair_at(1, xi=xmax - 1)
        pin(0, 64 * m - 1, B - 1, Oa, Ia)
        pin(1, 64 * m - 2, B - 2, Ob, Ib)
        assert Ob[0] < Oa[0]
        Oc, Ic = pair_at(2, xo=xmin)
        Od, Id = pair_at(3, xo=xmin + 1)
        pin(2, 0, 64, Oc, Ic)
        pin(3, 1, 65, Od, Id)
        assert Ic[0] < Id[0] < Ob[0] - 2
    else:       # coarse: (is a right pin, rank of O, rank of I, bucket of the pinned partner)
        plan = [(True, 40, 64, 20), (False, 127, 158, 40), (False, 191, 215, 60), (True, 236, 256, 100)]
        if B >= 642:
            plan += [(True, 500, 512, 180), (False, 575, 600, 200)]
        for k, (right, ro, ri, bucket) in enumerate(plan):
            if right:
                O, I = pair_at(k, xi=xmin + 16 * bucket)
                anchors[ri + 1] = xmin + 16 * (bucket + 1)          # the next box starts in the next bucket
            else:
                O, I = pair_at(k, xo=xmin + 16 * bucket + 15)
                anchors[ro - 1] = xmin + 16 * bucket - 1            # the box before starts in the bucket before
            pin(k, ro, ri, O, I)
        wide = 5
    if family != 'flat':
        fixed = dict(anchors)
        fixed.update({r: p[0] for r, p in pins.items()})
        fixed.setdefault(0, xmin)
        fixed.setdefault(B - 1, xmax)
        rs = sorted(fixed)
        x1 = np.zeros(B)
        for ra, rb in zip(rs[:-1], rs[1:]):
            assert fixed[ra] < fixed[rb], (ra, rb)
            x1[ra] = fixed[ra]
            x1[ra + 1:rb] = _fill_x(ra, fixed[ra], rb, fixed[rb], g)
        x1[rs[-1]] = fixed[rs[-1]]
        assert np.all(np.diff(x1) >= 0) and x1[0] == xmin and x1[-1] == xmax
    m = len(pins) // 2
    fw = rng.randint(1, 31, B).astype(np.float64)
    if family == 'frac':
        fw = fw + rng.randint(0, 4, B) * 0.25
    if wide is not None:
        assert wide not in pins and wide not in anchors
        fw[wide] = 3 * W
    x2 = x1 + fw - 1
    y1 = np.zeros(B)
    hh = rng.randint(1, band, B).astype(np.float64)
    fillers = [r for r in range(B) if r not in pins]
    y1[fillers] = (m + rng.permutation(len(fillers))) * band
    rows_of = np.zeros((m, 2), np.int64)        # ranks of (O, I) per pair
    for r, (a, b, k, outer) in pins.items():
        assert a == x1[r] or family == 'flat'
        x1[r], x2[r], y1[r], hh[r] = a, b, k * band, heights[k]
        rows_of[k, 0 if outer else 1] = r
    if family != 'flat':        # a pinned box has its x1 to itself
        for r in pins:
            assert np.sum(x1 == x1[r]) == 1, (family, r)
    assert y1.max() + band <= 65536 and x2.max() <= 65535
    by_rank = np.stack([x1, y1, x2, y1 + hh - 1], 1).astype(F32)
    assert np.array_equal(by_rank.astype(np.float64), np.stack([x1, y1, x2, y1 + hh - 1], 1))
    pr = rows_of.copy()
    pr[1::2] = pr[1::2, ::-1]
    ranks = np.concatenate([pr.ravel(), rng.permutation(np.asarray(fillers))])
    pairs = np.arange(2 * m).reshape(m, 2)
    pairs[1::2] = pairs[1::2, ::-1]
    return by_rank[ranks], pairs


def xbucket(x, xmin, scale, top=255):
    """xbucket of csrc/nms_kernels.hpp in float32 (top: the clamp)."""
    t = (F32(x) - xmin) * scale
    return 0 if t <= 0 else (top if t >= top else int(t))


def window_index(boxes, mode='kernel'):
    """frame_index_kernel in numpy: (rank of every row in the x1 order, cum [257], xmin, scale, wmax), all float32."""
    boxes = np.asarray(boxes, F32)
    order = np.argsort(boxes[:, 0], kind='stable')
    rank = np.empty(boxes.shape[0], np.int64)
    rank[order] = np.arange(boxes.shape[0])
    xmin, xmax = boxes[:, 0].min(), boxes[:, 0].max()
    scale = F32(256.0) / (xmax - xmin) if xmax > xmin else F32(0)
    wd = boxes[:, 2] - boxes[:, 0]
    wmax = (wd if mode == 'wmax_no_plus1' else wd + F32(1)).max()
    bk = np.array([xbucket(x, xmin, scale) for x in boxes[:, 0]])
    cum = np.concatenate([[0], np.cumsum(np.bincount(bk, minlength=256))])
    return rank, cum, xmin, scale, wmax


def window_model(boxes, query, t, site, mode='kernel', index=None):
    """The rank range [r0, r1) of the frame's x1 order that a site reads for the box `query` (a row of the frame or a free
    box [4]), as the code is written -- 'adj': adj_build_kernel (float32, 1.001 relative + 2 px; also returns the range of
    64-rank words [w0, w1), the granularity it reads at), 'xwindow': xwindow() (float64, 1.001 + 1 px), 'link': the link
    scans (float32, omt = (1 - t) * 1.002 + 1e-6, inv_t = 1.002 / t, + 2 px, the current box truncated) -- or as one of the
    single-token mistakes of WINDOW_MUTANTS would write it.  Returns (r0, r1), for 'adj' (r0, r1, w0, w1)."""
    assert site in WINDOW_SITES and mode in WINDOW_MODES
    boxes = np.asarray(boxes, F32)
    rank, cum, xmin, scale, wmax = index if index is not None else window_index(boxes, mode)
    q = boxes[int(query)] if np.ndim(query) == 0 else np.asarray(query, F32)
    bare = mode in ('in1', 'nomargin')                      # no relative and no pixel margin
    shift = 1.0 if mode == 'in1' else 0.0                   # ... and both bounds one pixel inward
    own = mode == 'own_width_left'
    top = 254 if mode == 'clamp254' else 255
    if site == 'adj':
        omt = F32(max(0.0, 1.0 - float(t)))
        rel = F32(1.0) if bare else F32(1.001)
        px = F32(0.0 if bare else 2.0)
        wrow = (q[2] - q[0]) + F32(1)
        wleft = wrow if own else min(wmax, wrow / max(F32(1) - omt, F32(1e-6)) * rel)
        lo = F32(F32(q[0] - omt * wleft * rel) - px) + F32(shift)
        hi = F32(F32(q[0] + omt * wrow * rel) + px) - F32(shift)
    elif site == 'xwindow':
        t = float(t)
        rel = 1.0 if bare else 1.001
        px = 0.0 if bare else 1.0
        x1c, wc = float(q[0]), float((q[2] - q[0]) + F32(1))
        wj = wc if own else min(float(wmax), wc / t * rel)
        lo = F32(max(x1c - (1.0 - t) * wj * rel - px + shift, -3.0e38))
        hi = F32(min(x1c + (1.0 - t) * wc * rel + px - shift, 3.0e38))
    else:
        cur = np.trunc(q)
        omt = F32(1.0 - float(t)) if bare else F32(1.0 - float(t)) * F32(1.002) + F32(1.0e-6)
        inv_t = F32((1.0 if bare else 1.002) / max(float(t), 1.0e-6))
        px = F32(0.0 if bare or mode == 'no_trunc_slack' else 2.0)
        wc = (cur[2] - cur[0]) + F32(1)
        lo = F32(F32(cur[0] - omt * (wc if own else min(wmax, wc * inv_t))) - px) + F32(shift)
        hi = F32(F32(cur[0] + omt * wc) + px) - F32(shift)
    b0, b1 = xbucket(lo, xmin, scale, top), xbucket(hi, xmin, scale, top)
    r0, r1 = int(cum[b0]), int(cum[b1] if mode == 'cum_b1' else cum[b1 + 1])
    if site != 'adj':
        return r0, r1
    nw = (boxes.shape[0] + 63) >> 6
    w0 = (r0 + 63) >> 6 if mode == 'ceil_w0' else r0 >> 6
    w1 = min(nw, r1 >> 6 if mode == 'floor_w1' else (r1 + 63) >> 6)
    return r0, r1, w0, w1


def link_query(box):
    """The box of the frame before whose truncation is `box`: x1 and x2 moved right by 0.75 px where they are whole pixels
    (the link scans truncate the current box, so the window is taken 0.75 px to the left of where the box stands)."""
    q = np.array(box, F32)
    if q[0] == np.trunc(q[0]) and q[2] == np.trunc(q[2]):
        q[0] += F32(0.75); q[2] += F32(0.75)
    return q


def window_lost(boxes, pairs, t, site, mode, frac=False):
    """(directed pinned pairs that are true partners by the site's referee, how many of them the window of `mode` does not
    read).  Both directions of every pair: the window of O has to hold I (right side) and the window of I has to hold O
    (left side).  frac: at the link site the queries are link_query() of the pinned boxes."""
    boxes = np.asarray(boxes, F32)
    index = window_index(boxes, mode)
    rank = index[0]
    true = lost = 0
    for o, i in np.asarray(pairs):
        for qrow, prow in ((o, i), (i, o)):
            q = link_query(boxes[qrow]) if (site == 'link' and frac) else boxes[qrow]
            if not window_partner(q, boxes[prow], t, site):
                continue
            true += 1
            r = window_model(boxes, q, t, site, mode, index)
            p = int(rank[prow])
            lost += not (r[2] <= p >> 6 < r[3] if site == 'adj' else r[0] <= p < r[1])
    return true, lost
