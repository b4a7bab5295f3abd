"""Box-filter sampling for the pixel tracker in numpy: the specification of vdet_luma_integral, vdet_track_pixels_box and
vdet_track_volume_pixels_box (include/vdet_hip.h, csrc/pixtrack_kernels.hpp; ``sampling='box'`` of the four ops calls).
Integers only, except the confidence.  The device must match it bit for bit.  Only what differs from the point rule is
restated here: a cell's VALUE.  Columns and rows are 0-based, ``//`` is floor division.

  luma      tests/pixtrack_spec.py's: L = (29*c0 + 150*c1 + 77*c2 + 128) >> 8
  integral  I[f, y, x] = sum of L[f, r, c] over r < y, c < x: uint32 [F, H+1, W+1], row 0 and column 0 zero.  H*W <= 2^24, so
            the largest entry, 255 * 2^24, and every tot + (area >> 1) below fit in 32 bits
  edges     on one axis, from the box origin o, the extent e (w or h), the side S, the limit N (W or H), for ANY integer k:
            a = o + (k*e) // S, b = o + ((k+1)*e) // S; a' = clamp(a, 0, N-1), b' = min(max(b, a'+1), N).  A cell partly
            outside the image averages its inside part; a cell wholly outside, or narrower than a pixel (e < S), becomes the
            nearest single column or row (edge replication, as in the point rule)
  value     tot = I[rb', cb'] - I[ra', cb'] - I[rb', ca'] + I[ra', ca'], area = (rb'-ra') * (cb'-ca'),
            v = (tot + (area >> 1)) // area, a uint8: the rounded mean of the cell's pixels

Everything else is unchanged: the template is cells 0..S-1 of the anchor box on the anchor frame and the region cells
-R..S+R-1 (pixtrack_spec); SAD, key, tie order, f32 confidence, move, outside test, bad anchors, step and max_frames
(pixtrack_spec); levels, margins, penalty and key of the scale search (pixtrack_scale_spec; scales = 0 is the fixed-scale
chain); the greedy loop (greedy_pixel_spec).  The chain below is pixtrack_scale_spec.track_slot with ``sample`` in the place
of pixtrack_spec.sample; the slot table and the greedy loop ARE pixtrack_scale_spec's functions, run with this chain as their
tracker (``_box_chain``).  With w == h == S every cell is one pixel and the rule is the point rule's, at the image's edges too.
"""
import contextlib

import numpy as np

import pixtrack_scale_spec as ps
import pixtrack_spec as px

AREA_MAX = 1 << 24


def integral(lumas):
    """uint8 [F,H,W] -> uint32 [F,H+1,W+1]"""
    lumas = np.asarray(lumas)
    F, H, W = lumas.shape
    assert H * W <= AREA_MAX
    out = np.zeros((F, H + 1, W + 1), np.uint32)
    out[:, 1:, 1:] = lumas.astype(np.uint64).cumsum(axis=1).cumsum(axis=2).astype(np.uint32)
    return out


def luma_integral(images):
    """uint8 [F,H,W,3] -> uint32 [F,H+1,W+1]: what vdet_luma_integral writes"""
    return integral(px.luma(np.asarray(images)))


def cell_edges(o, e, S, k, N):
    """(a', b') of cell k on one axis; k an int or an int array"""
    k = np.asarray(k, dtype=np.int64)
    a = o + (k * e) // S
    b = o + ((k + 1) * e) // S
    a = np.clip(a, 0, N - 1)
    b = np.minimum(np.maximum(b, a + 1), N)
    return a, b


def sample(I, box, S, k0, k1):
    """the cells k0..k1-1 (both axes) of ``box`` (0-based ints) from ONE frame's integral I [H+1,W+1] -> uint8 [k1-k0, k1-k0]"""
    x1, y1, x2, y2 = box
    H, W = I.shape[0] - 1, I.shape[1] - 1
    k = np.arange(k0, k1)
    ca, cb = cell_edges(x1, x2 - x1 + 1, S, k, W)
    ra, rb = cell_edges(y1, y2 - y1 + 1, S, k, H)
    J = I.astype(np.int64)
    tot = J[rb[:, None], cb[None, :]] - J[ra[:, None], cb[None, :]] - J[rb[:, None], ca[None, :]] + J[ra[:, None], ca[None, :]]
    area = (rb - ra)[:, None] * (cb - ca)[None, :]
    assert area.min() >= 1 and tot.min() >= 0 and (tot <= 255 * area).all()
    return ((tot + (area >> 1)) // area).astype(np.uint8)


def step_once(Tm, I, box, S, R, ns=0, p=5, q=0):
    """one step onto the frame whose integral is I: (moved box, conf, (level, dy, dx), raw SAD)"""
    tables = {}
    for l in range(-ns, ns + 1):
        bl = ps.level_box(box, l, p)
        if bl is not None:
            tables[l] = ps.sad_table(Tm, sample(I, bl, S, -R, S + R), R)
    sad, l, dy, dx = ps.pick(tables, R, q)
    x1, y1, x2, y2 = ps.level_box(box, l, p)
    wl, hl = x2 - x1 + 1, y2 - y1 + 1
    sx = (2 * dx * wl + S) // (2 * S)
    sy = (2 * dy * hl + S) // (2 * S)
    return (x1 + sx, y1 + sy, x2 + sx, y2 + sy), px.confidence(sad, S), (l, dy, dx), sad


def track_slot(integ, frame, box, S, R, min_conf=0.5, max_frames=0, step=1, scales=0, scale_step=5, scale_penalty=0):
    """rows [F,5] f32 of one live slot (``frame`` 1-based, ``box`` the 0-based integer anchor box) from integ [F,H+1,W+1]"""
    ps.check_settings(scales, scale_step, scale_penalty)
    F, H, W = integ.shape[0], integ.shape[1] - 1, integ.shape[2] - 1
    rows = np.full((F, 5), np.nan, np.float32)
    af = frame - 1
    rows[af] = px.row_of(box, np.float32(1.0))
    Tm = sample(integ[af], box, S, 0, S)
    thr = np.float32(min_conf)
    for d in (1, -1):
        cur = tuple(box)
        for n in range(1, px.reach_of(max_frames, F) + 1):
            g = af + d * n * step
            if g < 0 or g >= F:
                break
            cur, conf, _, _ = step_once(Tm, integ[g], cur, S, R, scales, scale_step, scale_penalty)
            if conf < thr or px.outside(cur, H, W):
                break
            rows[g] = px.row_of(cur, conf)
    return rows


@contextlib.contextmanager
def _box_chain(integ):
    """pixtrack_scale_spec's slot table and greedy loop call its module-level ``track_slot`` with the luma planes first: inside
    this block that name is the chain above on ``integ``, so the loops themselves are not restated"""
    saved = ps.track_slot
    ps.track_slot = lambda lumas, *args: track_slot(integ, *args)
    try:
        yield
    finally:
        ps.track_slot = saved


def track_pixels(images, anchor_frames, anchor_boxes, anchor_scores=None, grid=32, radius=8, min_conf=0.5, max_frames=0, step=1,
                 scales=0, scale_step=5, scale_penalty=0):
    """sampling='box' of ops.track_pixels (scales = 0) and ops.track_pixels_scaled -> (tracks [C,T,F,5] f32, anchors [C,T,3]
    f32, ntracks [C] int32, bad)"""
    with _box_chain(luma_integral(images)):
        return ps.track_pixels(images, anchor_frames, anchor_boxes, anchor_scores, grid, radius, min_conf, max_frames, step, scales,
                               scale_step, scale_penalty)


def track_volume_pixels(images, boxes, scores, nms_thres=0.3, thres=0.0, max_tracks=10, grid=32, radius=8, min_conf=0.5,
                        max_frames=0, step=1, scales=0, scale_step=5, scale_penalty=0):
    """sampling='box' of ops.track_volume_pixels (scales = 0) and ops.track_volume_pixels_scaled -> (tracks
    [C,max_tracks,F,5] f32, anchors [C,max_tracks,3] f32, ntracks [C] int32, bad)"""
    with _box_chain(luma_integral(images)):
        return ps.track_volume_pixels(images, boxes, scores, nms_thres, thres, max_tracks, grid, radius, min_conf, max_frames, step,
                                      scales, scale_step, scale_penalty)
