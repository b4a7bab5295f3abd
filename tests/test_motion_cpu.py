"""No GPU: the rule of motion-guided propagation (tests/motion_spec.py) against numbers worked by hand, on planted movers and on
a detector that misses a frame; the C-ABI's prototypes, binding rows and limits rows (include/vdet_hip.h, vdetlib_amd/_lib.py).
  a. the motion field at P = 8, R = 1 by hand;  b. the range rule and the rounding by hand;  c. planted movers;
  d. recall and AP on the spec;  e. the binding."""
import inspect

import numpy as np
import pytest

import motion_cases as mc
import motion_spec as ms
import pixtrack_harness as ph
import pixtrack_spec as px


def gray(planes):
    """luma planes [F,H,W] -> images uint8 [F,H,W,3] whose luma they are (29 + 150 + 77 = 256)"""
    images = np.repeat(np.asarray(planes, np.uint8)[..., None], 3, axis=-1)
    assert np.array_equal(px.luma(images), planes)
    return images


# a. -------------------------------------------------------------------------------------------------------------------
RAMP = np.tile(10 * np.arange(16), (16, 1))                      # L[y, x] = 10 * x
RIGHT = RAMP[:, np.maximum(np.arange(16) - 1, 0)]                # the ramp moved one column to the right, the edge replicated
LEFT = RAMP[:, np.minimum(np.arange(16) + 1, 15)]


@pytest.mark.parametrize("edge", ("right", "left", "bottom", "top"))
def test_the_clamp_at_each_edge(edge):
    """the ramp moves by one pixel toward ``edge``.  The block away from that edge matches exactly.  In the block AT the edge the
    candidate reads one column (row) beyond the image, which is the last one again: that column differs by 10 on each of its 8
    rows: cost 80.  Zero motion would cost 10 on all 64 pixels: 640.  The other axis ties on every shift: zero wins.
    The way back (direction 1 of the moved frame) matches exactly in both blocks: the moved frame's replicated edge column is the
    ramp's own first (last) column, which the clamp reads again"""
    moved = RIGHT if edge in ("right", "bottom") else LEFT
    pair = np.stack([RAMP, moved])
    sign = 1 if edge in ("right", "bottom") else -1
    if edge in ("bottom", "top"):
        pair = pair.transpose(0, 2, 1)
    field, cost, fsum = ms.motion_field(gray(pair), 8, 1)
    assert field.shape == (2, 2, 2, 2, 2) and field.dtype == np.int16 and cost.shape == (2, 2, 2, 2) and cost.dtype == np.int32
    vec = [sign, 0] if edge in ("right", "left") else [0, sign]
    assert (field[0, 0] == vec).all() and (field[1, 1] == [-v for v in vec]).all()
    at_edge = np.zeros((2, 2), bool)
    if edge in ("right", "left"):
        at_edge[:, 1 if edge == "right" else 0] = True
    else:
        at_edge[1 if edge == "bottom" else 0, :] = True
    assert np.array_equal(cost[0, 0], np.where(at_edge, 80, 0)) and (cost[1, 1] == 0).all()
    # the frames without a partner
    assert not field[0, 1].any() and not field[1, 0].any() and not cost[0, 1].any() and not cost[1, 0].any()
    assert not fsum[0, 1].any() and not fsum[1, 0].any()
    assert fsum.shape == (2, 2, 3, 3, 2) and fsum.dtype == np.int32 and fsum[0, 0, 2, 2].tolist() == [4 * v for v in vec]


def test_a_partial_block():
    """16 columns x 12 rows, L[y, x] = 10 * y moved one row down.  Block row 1 holds rows 8..11 and row 11 four more times:
    80 90 100 110 110 110 110 110.  At dy = +1 its rows 8..10 match exactly, and rows 11..15 all read the moved frame's row 11,
    which is 100: 5 rows x 8 columns x 10 = 400.  dy = 0: 8 rows x 8 x 10 = 640.  dy = -1: rows 8..11 differ by 20, 12..15 by
    20: 1280.  The way back: the moved frame's block row 1 is 70 80 90 100 100 100 100 100; at dy = -1 its rows 8..11 match, and
    rows 12..15 read the ramp's row 11, which is 110: 4 rows x 8 x 10 = 320 (dy = 0 costs 640)"""
    ramp = np.tile(10 * np.arange(12)[:, None], (1, 16))
    down = ramp[np.maximum(np.arange(12) - 1, 0)]
    field, cost, _ = ms.motion_field(gray(np.stack([ramp, down])), 8, 1)
    assert field.shape == (2, 2, 2, 2, 2)
    assert (field[0, 0] == [0, 1]).all() and cost[0, 0].tolist() == [[0, 0], [400, 400]]
    assert (field[1, 1] == [0, -1]).all() and cost[1, 1].tolist() == [[0, 0], [320, 320]]


def test_a_flat_frame_ties_on_zero_motion():
    field, cost, fsum = ms.motion_field(np.full((3, 16, 16, 3), 77, np.uint8), 8, 1)
    assert not field.any() and not cost.any() and not fsum.any()
    # one brighter pixel in the middle frame: the blocks that hold it, or see it in the neighbour, still prefer the smallest
    # shift among equal SADs
    images = np.full((3, 16, 16, 3), 77, np.uint8)
    images[1, 3, 3] = 200
    field, cost, _ = ms.motion_field(images, 8, 1)
    assert not field.any()                       # every shift of block (0,0) costs the same: the pixel is in or out once
    assert cost[0, 1, 0, 0] == cost[1, 1, 0, 0] == cost[0, 0, 0, 0] == cost[1, 2, 0, 0] == 123 and cost.sum() == 4 * 123


def test_fsum_against_a_double_loop():
    rng = np.random.RandomState(9001)
    field = rng.randint(-16, 17, size=(2, 3, 4, 5, 2)).astype(np.int16)
    got = ms.summed(field)
    assert got.shape == (2, 3, 5, 6, 2) and got.dtype == np.int32
    for d in range(2):
        for f in range(3):
            for y in range(5):
                for x in range(6):
                    want = [sum(int(field[d, f, r, c, k]) for r in range(y) for c in range(x)) for k in range(2)]
                    assert got[d, f, y, x].tolist() == want


def test_motion_field_of_noise_equals_a_scalar_restatement():
    """one block of a random pair, every candidate by scalar loops"""
    rng = np.random.RandomState(9002)
    images = rng.randint(0, 256, size=(2, 13, 21, 3)).astype(np.uint8)
    L = px.luma(images).astype(int)
    field, cost, _ = ms.motion_field(images, 8, 2)
    H, W = 13, 21
    for by, bx in ((0, 0), (1, 2), (0, 2), (1, 0)):
        best = None
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                sad = sum(abs(L[0, min(max(by * 8 + i, 0), H - 1), min(max(bx * 8 + j, 0), W - 1)] -
                              L[1, min(max(by * 8 + i + dy, 0), H - 1), min(max(bx * 8 + j + dx, 0), W - 1)])
                          for i in range(8) for j in range(8))
                key = (sad, dy * dy + dx * dx, dy, dx)
                best = key if best is None or key < best else best
        assert field[0, 0, by, bx].tolist() == [best[3], best[2]] and cost[0, 0, by, bx] == best[0]


# b. -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("X1,X2,want", (
    (4, 12, (0, 1)),          # the centres 4 and 12 are the box's own ends
    (5, 11, (1, 1)),          # no centre inside: the block of the box's middle, (5 + 11) // 2 = 8
    (-10, 50, (0, 3)),        # wider than the image: every block
    (-20, -3, (0, 0)),        # left of the image: centres -20 and -12 lie inside, both clamp to block 0
    (40, 50, (3, 3)),         # right of the image
    (12, 9, (1, 1)),          # x2 < x1: no centre inside, (12 + 9) // 2 = 10
    (-3, -2, (0, 0)),         # no centre inside, a negative middle: (-5) // 2 = -3, -3 // 8 = -1, clamped
    (0, 31, (0, 3)),
    (13, 19, (2, 2)),         # no centre inside: middle 16
))
def test_the_range_rule_by_hand(X1, X2, want):
    """P = 8, four blocks on the axis: centre pixels 4, 12, 20, 28"""
    assert ms.block_range(X1, X2, 8, 4) == want


@pytest.mark.parametrize("s,n,want", ((1, 2, 1), (-1, 2, 0), (3, 2, 2), (-3, 2, -1), (5, 4, 1), (-5, 4, -1), (6, 4, 2), (-6, 4, -1),
                                      (0, 3, 0), (-7, 1, -7)))
def test_the_rounding_by_hand(s, n, want):
    """the mean s / n rounded half UP, for both signs: 0.5 -> 1, -0.5 -> 0, 1.5 -> 2, -1.5 -> -1, 1.25 -> 1, -1.25 -> -1"""
    field = np.zeros((1, 4, 2), np.int16)
    field[0, 0, 0] = s                     # n blocks in the range, the x components sum to s
    field[0, 0, 1] = -s
    fs = ms.summed(field)
    box = (4, 0, 4 + 8 * (n - 1), 7)        # the centres of blocks 0 .. n-1
    assert ms.block_range(box[0], box[2], 8, 4) == (0, n - 1)
    assert ms.box_shift(fs, 8, box) == (want, (2 * -s + n) // (2 * n))


def test_box_shift_reads_rows_like_columns():
    rng = np.random.RandomState(9003)
    field = rng.randint(-16, 17, size=(5, 4, 2)).astype(np.int16)
    fs = ms.summed(field)
    for box in ((5, 3, 30, 37), (-9, 20, 2, 21), (12, 9, 9, 12), (0, 0, 31, 39), (100, -50, 200, -40)):
        c0, c1 = ms.block_range(box[0], box[2], 8, 4)
        r0, r1 = ms.block_range(box[1], box[3], 8, 5)
        part = field[r0:r1 + 1, c0:c1 + 1].astype(int).reshape(-1, 2)
        n = len(part)
        want = tuple(int(np.floor((2 * part[:, k].sum() + n) / (2.0 * n))) for k in range(2))
        assert ms.box_shift(fs, 8, box) == want


# c. -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(mc.SCENES)))
def test_planted_movers(k):
    """From the planted box of frame MID, 1 to 3 frames in both directions.
    The margin, on the spec alone and FIRST: after m steps the accumulated shift is within m pixels of the planted motion on
    each axis -- one pixel a step, which covers the rounding of the mean and the blocks whose centre is in the box but whose
    pixels are partly background.  By geometry that keeps IoU >= (w-3)(h-3) / (2wh - (w-3)(h-3)) >= 0.59 on the smallest object
    here (24 x 20).  Then the evaluator's criterion, IoU >= 0.5 with the planted box of the frame, for every propagated box; and
    the box left where it was fails it at distance 3."""
    H, W, w, h, vx, vy, P, R = mc.SCENES[k]
    images, truth = mc.planted(k)
    fsum = mc.field_of(k)[2]
    st, ib = ms.source_state(truth[mc.MID])
    assert st == 1
    bound = (w - 3.0) * (h - 3.0) / (2.0 * w * h - (w - 3.0) * (h - 3.0))
    assert bound >= 0.59
    for direction, sign in enumerate((1, -1)):
        steps = ms.walk(fsum, P, H, W, mc.MID, ib, direction, mc.REACH)
        assert len(steps) == mc.REACH
        for m, (Sx, Sy) in enumerate(steps, 1):
            assert abs(Sx - sign * m * vx) <= m and abs(Sy - sign * m * vy) <= m, (direction, m, Sx, Sy)
    # the same through propagate: one box, one class
    boxes = np.tile(truth[:, None, :], (1, 1, 1))
    scores = np.full((mc.F, 1, 1), 0.5, np.float32)
    keep_idx = np.zeros((mc.F, 1, 1), np.int32)
    keep_cnt = np.zeros((mc.F, 1), np.int32)
    keep_cnt[mc.MID] = 1
    tracks, ntracks, score, src, bad = ms.propagate(fsum, P, H, W, boxes, scores, keep_idx, keep_cnt, top=1, reach=mc.REACH)
    assert not bad and ntracks.tolist() == [2 * mc.REACH]
    seen = 0
    for di, delta in enumerate(ms.deltas(mc.REACH)):
        g = mc.MID + delta
        live = np.flatnonzero(np.isfinite(tracks[0, di, :, 0]))
        assert live.tolist() == [g] and src[0, di, g] == 0 and score[0, di, g] == np.float32(0.5)
        ov = mc.iou(tracks[0, di, g, :4], truth[g])
        assert ov >= bound and ov >= 0.5, (delta, ov)
        seen += 1
    assert seen == 6
    for delta in (-3, 3):
        assert mc.iou(truth[mc.MID], truth[mc.MID + delta]) < 0.5


def test_chain_ends_and_bad_sources():
    """a box that leaves the image ends its chain; decay; the three kinds of bad data write NaN rows and flag the call"""
    H, W, P = 32, 32, 8
    F = 5
    field = np.zeros((2, F, 4, 4, 2), np.int16)
    field[0, :, :, :, 0] = 16                  # forward: everything moves 16 columns to the right
    fsum = ms.summed(field)
    boxes = np.array([[[5, 5, 12, 12], [np.nan, 1, 2, 3], [1, 1, 2.0 ** 20 + 1, 4]]] * F, np.float32)
    scores = np.full((F, 3, 1), 0.8, np.float32)
    keep_idx = np.zeros((F, 1, 2), np.int32)
    keep_cnt = np.zeros((F, 1), np.int32)
    keep_cnt[0] = 1
    tracks, nt, score, src, bad = ms.propagate(fsum, P, H, W, boxes, scores, keep_idx, keep_cnt, top=1, reach=3, decay=0.5)
    assert not bad and nt.tolist() == [6]
    # forward from frame 0: 16 columns (inside: x1 = 20), then 32 (x1 = 36 > 31: outside) -- slot of delta = +1 only
    assert tracks[0, 3, 1].tolist() == [21, 5, 28, 12, np.float32(0.4)] and np.isnan(tracks[0, 4]).all() and np.isnan(tracks[0, 5]).all()
    assert np.isnan(tracks[0, :3]).all() and (src[0, :3] == ms.INT32_MIN).all() and src[0, 3, 1] == 0
    for kind in range(4):
        ki, kc = keep_idx.copy(), keep_cnt.copy()
        kc[2] = 1
        if kind == 0:
            ki[2, 0, 0] = 1                    # a NaN coordinate
        elif kind == 1:
            ki[2, 0, 0] = 2                    # beyond 2^20
        elif kind == 2:
            ki[2, 0, 0] = 3                    # keep_idx = B
        else:
            kc[2] = 3                          # keep_cnt = kcap + 1
        t2, _, _, s2, bad = ms.propagate(fsum, P, H, W, boxes, scores, ki, kc, top=1, reach=3, decay=0.5)
        assert bad and ph.bits_equal(t2, tracks) and np.array_equal(s2, src)


# d. -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", (0, 2))
def test_recall_and_ap_on_the_spec(k):
    """the detector reports the object on every frame but MID.  After propagation + oracle.nms per frame the missed frame holds
    a detection of IoU >= 0.5; without propagation it holds none; the AP of the class rises strictly"""
    from vdetlib_amd import eval as ev
    truth = mc.planted(k)[1]
    still = mc.detector(k)
    assert still[3][:, 0].min() >= mc.TOP              # every list has its sources
    plain = ev.detections_from_keep_lists(mc.VIDEO, *still)
    assert mc.best_iou_on(mc.MID, plain, truth) < 0.5
    prop, out = mc.pipeline_spec(k)
    moved = ev.detections_from_tracks(mc.VIDEO, out['tracks'], out['ntracks'], out['score'])
    assert mc.best_iou_on(mc.MID, moved, truth) >= 0.5
    for f in range(mc.F):
        assert mc.best_iou_on(f, moved, truth) >= 0.5
    ap_plain, ap_moved = mc.host_aps(k)
    assert ap_moved > ap_plain and abs(ap_plain - 6.0 / 7.0) < 1e-12 and abs(ap_moved - 1.0) < 1e-12


# e. -------------------------------------------------------------------------------------------------------------------
PROTOS = {
    'vdet_motion_field': ['vdet_ctx *ctx', 'const uint8_t *d_images', 'int64_t F', 'int64_t H', 'int64_t W', 'int block', 'int radius',
                          'int16_t *d_field', 'int32_t *d_cost', 'int32_t *d_fsum'],
    'vdet_motion_table': ['vdet_ctx *ctx', 'const int16_t *d_field', 'int64_t F', 'int64_t Hb', 'int64_t Wb', 'int32_t *d_fsum'],
    'vdet_propagate_boxes': ['vdet_ctx *ctx', 'const int32_t *d_fsum', 'int64_t F', 'int64_t Hb', 'int64_t Wb', 'int block', 'int64_t H',
                             'int64_t W', 'int64_t B', 'int64_t C', 'const float *d_boxes', 'const float *d_scores',
                             'const int32_t *d_keep_idx', 'int64_t kcap', 'const int32_t *d_keep_cnt', 'int top', 'int reach',
                             'double decay', 'float *d_tracks', 'float *d_score', 'int32_t *d_src', 'int32_t *d_ntracks'],
}


@pytest.mark.parametrize("name", sorted(PROTOS))
def test_prototypes_and_binding_rows(name):
    import ctypes
    from vdetlib_amd import _lib
    args = ph.prototype(name)
    assert args == PROTOS[name]
    res, types = _lib.SYMBOLS[name]
    assert res is ctypes.c_int and types == [ph.ctype_of(a) for a in args]
    L = _lib.load_library()
    assert getattr(L, name)(*([None] + [0] * (len(args) - 1))) == _lib.VDET_EINVAL          # a NULL context: nothing touched


def test_limits_rows_and_the_status_bit():
    import os
    import re
    hdr = ph.header()
    top = hdr[:hdr.index('#ifndef VDET_HIP_H')]
    for words in ('(vdet_motion_field) block 8, 16 or 32, 1 <= radius <= 16, H, W <= 32767', '(vdet_motion_table) 1 <= Hb, Wb <= 4096',
                  '(vdet_propagate_boxes)', '1 <= top <= kcap, 1 <= reach <= 16, 2*reach*top <= 1024', 'decay finite and >= 0'):
        assert words in top, words
    src = open(os.path.join(ph.ROOT, 'vdetlib_amd', 'csrc', 'motion_kernels.hpp')).read()
    assert 'constexpr int kStBadPropagate = 8192;' in src
    bits = []
    for fn in os.listdir(os.path.join(ph.ROOT, 'vdetlib_amd', 'csrc')):
        if fn.endswith('.hpp'):
            bits += re.findall(r'constexpr int kSt\w+ = (\d+);', open(os.path.join(ph.ROOT, 'vdetlib_amd', 'csrc', fn)).read())
    assert len(bits) == len(set(bits))                  # no status bit is used twice


def test_ops_signatures():
    from vdetlib_amd import ops
    p = inspect.signature(ops.motion_field).parameters
    assert list(p) == ['images', 'block', 'radius', 'sync', 'ctx'] and (p['block'].default, p['radius'].default) == (16, 8)
    p = inspect.signature(ops.propagate_detections).parameters
    assert list(p) == ['motion', 'still', 'top', 'reach', 'decay', 'sync', 'ctx']
    assert (p['reach'].default, p['decay'].default, p['sync'].default) == (3, 1.0, True)
