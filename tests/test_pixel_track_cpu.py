"""CPU-only: the numpy statement of the pixel tracker (tests/pixtrack_spec.py) against numbers worked out by hand and against
planted objects whose positions are known, and the C-ABI surface of the device form (vdet_track_pixels)."""
import ctypes
import inspect
import re

import numpy as np
import pytest

import pixtrack_cases as pc
import pixtrack_spec as px
from pixtrack_harness import ctype_of, header, prototype


def grey(plane):
    """a luma plane as an image: c0 = c1 = c2 = v has luma (256*v + 128) >> 8 = v"""
    return np.repeat(np.asarray(plane, dtype=np.uint8)[..., None], 3, axis=-1)


# ---- a. by hand: S = 4, R = 1, 8 x 8 ---------------------------------------------------------------------------------------

def test_luma_constants():
    # (29*255 + 128) >> 8 = 7523 >> 8 = 29; (150*255 + 128) >> 8 = 38378 >> 8 = 149; (77*255 + 128) >> 8 = 19763 >> 8 = 77
    # 29 + 150 + 77 = 256: white is (256*255 + 128) >> 8 = 255; (10,20,30): 290 + 3000 + 2310 + 128 = 5728 >> 8 = 22
    img = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 255], [0, 0, 0], [10, 20, 30], [30, 20, 10]], np.uint8)
    # (30,20,10): 870 + 3000 + 770 + 128 = 4768 >> 8 = 18: the channel order matters and is never swapped
    assert px.luma(img).tolist() == [29, 149, 77, 255, 0, 22, 18]
    assert px.luma(img).dtype == np.uint8
    v = np.arange(256, dtype=np.uint8)
    assert np.array_equal(px.luma(grey(v)), v)


def test_grid_floor_division_and_clamp():
    k = np.arange(-2, 6)
    # w = 6, S = 4: (2k+1)*6 // 8 for k = -2..5: -18//8 = -3 (truncation would give -2), -6//8 = -1 (truncation: 0), 0, 2, 3, 5, 6, 8
    assert ((2 * k + 1) * 6 // 8).tolist() == [-3, -1, 0, 2, 3, 5, 6, 8]
    assert px.grid_index(10, 6, 4, k, 100).tolist() == [7, 9, 10, 12, 13, 15, 16, 18]
    # w = 2 < S: cells share pixels: 2//8, 6//8, 10//8, 14//8 = 0, 0, 1, 1; k = -1: -2//8 = -1; k = 4: 18//8 = 2
    assert px.grid_index(3, 2, 4, np.arange(-1, 5), 100).tolist() == [2, 3, 3, 4, 4, 5]
    # the clamp at each edge, 8 x 8 image, box (-1,5,4,10) 0-based (w = h = 6): columns -1 + [-1,0,2,3,5,6] = [-2,-1,1,2,4,5]
    # -> [0,0,1,2,4,5]; rows 5 + [-1,0,2,3,5,6] = [4,5,7,8,10,11] -> [4,5,7,7,7,7]
    r = np.arange(-1, 5)
    assert px.grid_index(-1, 6, 4, r, 8).tolist() == [0, 0, 1, 2, 4, 5]
    assert px.grid_index(5, 6, 4, r, 8).tolist() == [4, 5, 7, 7, 7, 7]
    L = (10 * np.arange(8)[:, None] + np.arange(8)[None, :]).astype(np.uint8)
    want = np.array([[10 * y + x for x in (0, 0, 1, 2, 4, 5)] for y in (4, 5, 7, 7, 7, 7)], np.uint8)
    assert np.array_equal(px.sample(L, (-1, 5, 4, 10), 4, -1, 5), want)
    # right and top: box (5,-3,10,2): columns 5 + [-1,0,2,3,5,6] = [4,5,7,8,10,11] -> [4,5,7,7,7,7]; rows -> [0,0,0,0,2,3]
    assert px.grid_index(5, 6, 4, r, 8).tolist() == [4, 5, 7, 7, 7, 7] and px.grid_index(-3, 6, 4, r, 8).tolist() == [0, 0, 0, 0, 2, 3]


def test_tie_order():
    # Tm has 100 at (1,1) and (1,2); row 2 of the 6 x 6 region is [0,100,100,100,100,0].  dx = -1 sees [0,100,100,100] against
    # [0,100,100,0]: SAD 100; dx = +1 sees [100,100,100,0]: 100; dx = 0 sees four 100s: 200; dy = +-1 puts Tm's row on zeros
    # (200) and the region's row on a zero row of Tm (>= 300 more).  (100, 1, 0, -1) < (100, 1, 0, +1): dx = -1 wins
    Tm = np.zeros((4, 4), np.uint8)
    Tm[1, 1] = Tm[1, 2] = 100
    Rg = np.zeros((6, 6), np.uint8)
    Rg[2, 1:5] = 100
    assert px.best_shift(Tm, Rg, 1) == (100, 0, -1)
    # dy before dx: Tm is 100 on its four centre cells, the region on the 12-cell plus (rows 1..4 x columns 2..3 and rows 2..3 x
    # columns 1..4): both are symmetric under the two flips and the transposition, so (-1,0), (0,-1), (0,1), (1,0) tie.  (-1,0):
    # the window (rows 0..3, columns 1..4) matches the block and sees (3,2), (3,3) and rows 2..3 of columns 1 and 4: 600.  (-1,-1):
    # the window (rows 0..3, columns 0..3) misses (1,1) and sees 8 - 3 others: 600, but dy^2+dx^2 = 2.  (0,0) sees 8 others: 800.
    # (600, 1, -1, 0) is the smallest key
    Tm = np.zeros((4, 4), np.uint8)
    Tm[1:3, 1:3] = 100
    Rg = np.zeros((6, 6), np.uint8)
    Rg[1:5, 2:4] = 100
    Rg[2:4, 1:5] = 100
    assert px.best_shift(Tm, Rg, 1) == (600, -1, 0)
    # the distance before the offsets: a flat pair ties everywhere, (0, 0) wins
    assert px.best_shift(np.full((4, 4), 7, np.uint8), np.full((6, 6), 7, np.uint8), 1) == (0, 0, 0)


def test_shift_rounding():
    def shift(d, w, S):
        return (2 * d * w + S) // (2 * S)
    # S = 4: w = 6: +1 -> 16//8 = 2 (1.5 rounds up), -1 -> -8//8 = -1 (-1.5 rounds up); w = 2 < S: -1 -> 0//8 = 0, +1 -> 8//8 = 1;
    # w = 3: -1 -> -2//8 = -1 (a negative numerator: truncation would give 0), +1 -> 10//8 = 1; w = 8: +-1 -> 20//8 = 2, -12//8 = -2
    assert [shift(1, 6, 4), shift(-1, 6, 4), shift(-1, 2, 4), shift(1, 2, 4), shift(-1, 3, 4), shift(1, 3, 4), shift(1, 8, 4),
            shift(-1, 8, 4)] == [2, -1, 0, 1, -1, 1, 2, -2]
    # step_once applies it: a 2 x 3 box (w < S) on a ramp.  The grid doubles pixels: columns 3 + [-1,0,0,1,1,2], rows
    # 2 + [-1,0,1,1,2,3] ((2k+1)*3 // 8 = -1,0,1,1,2,3), so only the step's own arithmetic is pinned here, on x
    L = (np.arange(8)[None, :] * 20 + np.zeros((8, 1))).astype(np.uint8)      # L[y][x] = 20 x
    Tm = px.sample(L, (3, 2, 4, 4), 4, 0, 4)                                  # columns 3,3,4,4
    assert Tm[0].tolist() == [60, 60, 80, 80]
    Lm = np.roll(L, -1, axis=1)                                               # the content moved LEFT by one pixel: Lm[y][x] = 20 (x+1)
    # region columns 2,3,3,4,4,5 -> 60,80,80,100,100,120; dx = -1: [60,80,80,100] vs [60,60,80,80] -> 40 a row; dx = 0:
    # [80,80,100,100] -> 80; dx = +1: [80,100,100,120] -> 120.  Half a cell cannot be matched: dx = -1, SAD 160, and the box moves
    # (2*(-1)*2 + 4) // 8 = 0
    box, conf, (l, dy, dx), sad = px.step_once(Tm, Lm, (3, 2, 4, 4), 4, 1)
    assert (l, dy, dx, sad) == (0, 0, -1, 160) and box == (3, 2, 4, 4)
    assert conf == np.float32(1.0) - np.float32(160) / np.float32(4080)


def ramp(shift, bump=None):
    """8 x 8 plane 10 y + (x - shift) + 30: the content of ramp(0) moved right by ``shift`` pixels"""
    L = (10 * np.arange(8)[:, None] + (np.arange(8)[None, :] - shift) + 30).astype(np.int64)
    if bump is not None:
        L[bump[0], bump[1]] += bump[2]
    return L.astype(np.uint8)


def test_chain_by_hand():
    """Box (3,3,6,6) 1-based = (2,2,5,5) 0-based, w = h = S = 4: pitch 1, cell k is pixel 2 + k (36//8 = 4 and -4//8 = -1 at the
    ends), the region columns and rows 1..6, no clamp.  On a ramp 10 y + x a candidate (dy,dx) on content moved by m has
    SAD 16 * |10 dy + dx - m|: both signs of dx are found exactly; dx = -1 moves the box by (-8 + 4) // 8 = -1."""
    frames = np.stack([grey(ramp(-1)), grey(ramp(0)), grey(ramp(1)), grey(ramp(2, bump=(3, 5, 51)))], 0)
    L = px.luma(frames)
    Tm = px.sample(L[1], (2, 2, 5, 5), 4, 0, 4)
    assert Tm.tolist() == [[52, 53, 54, 55], [62, 63, 64, 65], [72, 73, 74, 75], [82, 83, 84, 85]]
    Rg = px.sample(L[2], (2, 2, 5, 5), 4, -1, 5)
    sads = {(dy, dx): int(np.abs(Tm.astype(int) - Rg[1 + dy:5 + dy, 1 + dx:5 + dx].astype(int)).sum()) for dy in (-1, 0, 1) for dx in (-1, 0, 1)}
    assert sads == {(dy, dx): 16 * abs(10 * dy + dx - 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)}
    assert px.step_once(Tm, L[2], (2, 2, 5, 5), 4, 1)[:3] == ((3, 2, 6, 5), np.float32(1.0), (0, 0, 1))
    assert px.step_once(Tm, L[0], (2, 2, 5, 5), 4, 1)[:3] == ((1, 2, 4, 5), np.float32(1.0), (0, 0, -1))
    # frame 3: moved once more, and pixel (row 3, column 5) -- inside the moved box (4,2,7,5) -- is 51 brighter: the right
    # candidate has SAD 51; every other one has 15 or 16 pixels off by >= 1 and the bumped one off by >= 50: >= 65
    box, conf, d, sad = px.step_once(Tm, L[3], (3, 2, 6, 5), 4, 1)
    c51 = np.float32(1.0) - np.float32(51) / np.float32(4080)
    assert (box, d, sad) == ((4, 2, 7, 5), (0, 0, 1), 51) and conf == c51
    one = np.float32(1.0)
    want = np.array([[2, 3, 5, 6, one], [3, 3, 6, 6, one], [4, 3, 7, 6, one], [5, 3, 8, 6, c51]], np.float32)
    fr, bx = np.array([[2]], np.int32), np.array([[[3.9, 3.2, 6.99, 6.5]]], np.float32)      # fractional: truncated to (3,3,6,6)
    tracks, anchors, nt, bad = px.track_pixels(frames, fr, bx, None, 4, 1, min_conf=float(c51))
    assert not bad and nt.tolist() == [1] and anchors.tolist() == [[[2.0, -1.0, 0.0]]]
    assert np.array_equal(tracks[0, 0], want)                  # conf == min_conf: the chain goes on
    tracks = px.track_pixels(frames, fr, bx, None, 4, 1, min_conf=float(np.nextafter(c51, one)))[0]
    assert np.array_equal(tracks[0, 0, :3], want[:3]) and np.isnan(tracks[0, 0, 3]).all()
    # max_frames = 3: ceil(4/2) - 1 = 1 step each way; = 2: ceil(3/2) - 1 = 1; = 1: none
    for mf, live in ((3, [0, 1, 2]), (2, [0, 1, 2]), (1, [1]), (5, [0, 1, 2, 3])):
        tr = px.track_pixels(frames, fr, bx, None, 4, 1, min_conf=0.5, max_frames=mf)[0][0, 0]
        assert np.flatnonzero(~np.isnan(tr[:, 0])).tolist() == live, mf


def test_bad_anchor_data():
    img = np.zeros((3, 8, 8, 3), np.uint8)
    ok = [3, 3, 6, 6]
    cases = [(4, ok), (-1, ok), (1, [np.nan, 3, 6, 6]), (1, [3, 3, np.inf, 6]), (1, [3, 3, 2 ** 20 + 1, 6]), (1, [3, 3, 2.9, 6]),
             (1, [3, 5, 6, 4.5]), (1, [9, 3, 12, 6]), (1, [3, -4, 6, 0.5]), (1, [-7, 3, 0, 6]), (1, [3, 9, 6, 12])]
    for frame, box in cases:
        fr = np.array([[1, frame, 2]], np.int32)
        bx = np.array([[ok, box, ok]], np.float32)
        tracks, anchors, nt, bad = px.track_pixels(img, fr, bx, None, 4, 1)
        assert bad and np.isnan(tracks[0, 1]).all() and not np.isnan(tracks[0, 0]).any() and nt.tolist() == [3], (frame, box)
        assert anchors[0, 1, 0] == frame
    # legal edge cases: one pixel inside, a 1 x 1 box, the bound itself, an empty slot with a wild box
    for frame, box in ((1, [-5, -5, 1, 1]), (1, [8, 8, 20, 20]), (3, [4, 4, 4.9, 4.9]), (1, [-2.0 ** 20, 1, 2, 2]), (0, [np.nan] * 4)):
        tracks, anchors, nt, bad = px.track_pixels(img, np.array([[frame]], np.int32), np.array([[box]], np.float32), None, 4, 1)
        assert not bad and nt.tolist() == [int(frame > 0)], (frame, box)


# ---- b. planted objects -------------------------------------------------------------------------------------------------------

PLANTED = ((32, 8, 64, 96), (8, 2, 16, 8), (16, 4, 16, 32), (64, 16, 64, 64))


@pytest.mark.parametrize("S,R,w,h", PLANTED)
def test_planted_objects_are_followed_exactly(S, R, w, h):
    F, anchor = 10, 5
    H, W = h + 6 * (R - 1) * (h // S) + 7, w + 6 * (R - 1) * (w // S) + 5
    images, pos = pc.planted_video(1000 + S, F, H, W, w, h, S, R, anchor)
    moves = np.abs(np.diff(pos, axis=0)) // (w // S, h // S)
    assert moves.max() <= R - 1 and moves.max() >= 1
    x, y = pos[anchor]
    tracks, _, nt, bad = px.track_pixels(images, np.array([[anchor + 1]], np.int32),
                                         np.array([[[x + 1, y + 1, x + w, y + h]]], np.float32), None, S, R, min_conf=0.5)
    assert not bad and nt.tolist() == [1]
    assert np.array_equal(tracks[0, 0], pc.rows_from_positions(pos, w, h, range(F)))


# ---- c. the object vanishes ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("S,R,w,h", PLANTED[:3])
def test_chain_ends_where_the_object_vanishes(S, R, w, h):
    F, anchor, gone = 10, 3, 7
    H, W = h + 6 * (R - 1) * (h // S) + 7, w + 6 * (R - 1) * (w // S) + 5
    images, pos = pc.planted_video(2000 + S, F, H, W, w, h, S, R, anchor, vanish_from=gone)
    x, y = pos[anchor]
    fr, bx = np.array([[anchor + 1]], np.int32), np.array([[[x + 1, y + 1, x + w, y + h]]], np.float32)
    free = px.track_pixels(images, fr, bx, None, S, R, min_conf=0.0)[0][0, 0]
    print("confidence on the first empty frame: %.4f" % free[gone, 4])
    assert free[gone, 4] < 0.9                  # the precondition: noise does not look like the object
    assert not np.isnan(free[:, 0]).any()       # min_conf <= 0 never stops
    tracks = px.track_pixels(images, fr, bx, None, S, R, min_conf=0.9)[0][0, 0]
    assert np.array_equal(tracks, pc.rows_from_positions(pos, w, h, range(gone)), equal_nan=True)


# ---- d. a flat image ----------------------------------------------------------------------------------------------------------

def test_flat_image_stays_put():
    images = np.full((5, 40, 50, 3), 93, np.uint8)
    tracks = px.track_pixels(images, np.array([[3]], np.int32), np.array([[[11, 7, 30, 31]]], np.float32), None, 8, 2)[0][0, 0]
    assert np.array_equal(tracks, np.tile(np.array([11, 7, 30, 31, 1], np.float32), (5, 1)))


# ---- e. the binding --------------------------------------------------------------------------------------------------------

def test_header_prototype_and_symbol_row():
    from vdetlib_amd import _lib
    proto = prototype('vdet_track_pixels')
    assert proto[0] == 'vdet_ctx *ctx' and proto[1] == 'const uint8_t *d_images'
    assert [a.split()[-1].lstrip('*') for a in proto[2:]] == ['F', 'H', 'W', 'd_anchor_frames', 'd_anchor_boxes', 'd_anchor_scores', 'C', 'T',
                                                              'S', 'R', 'min_conf', 'max_frames', 'step', 'd_tracks', 'd_anchors',
                                                              'd_ntracks']
    res, args = _lib.SYMBOLS['vdet_track_pixels']
    assert res is ctypes.c_int and args == [ctype_of(a) for a in proto]


def test_null_context_refused():
    from vdetlib_amd import _lib
    L = _lib.load_library()
    z = None
    assert L.vdet_track_pixels(z, z, 1, 8, 8, z, z, z, 1, 1, 8, 2, 0.5, 0, 1, z, z, z) == _lib.VDET_EINVAL


def test_limits_table_row():
    head = header().split('#ifndef VDET_HIP_H')[0]
    m = re.search(r'\n \*   device pixel tracker(.*?)\n \*/', head, flags=re.S)
    assert m, "the limits table has no 'device pixel tracker' row"
    row = re.sub(r'\s*\n \*\s*', ' ', m.group(1))
    for part in ('multiple of 4 in 4 .. 64', '1 <= radius R <= 16', 'step >= 1', 'max_frames >= 0', 'min_conf finite', 'H, W <= 32767',
                 'C*T*F < 2^31 - 16', 'VDET_EINVAL', 'latched'):
        assert part in row, part


def test_python_surface():
    from vdetlib_amd import ops
    from vdetlib_amd.vdet import track
    assert list(inspect.signature(ops.track_pixels).parameters) == [
        'images', 'anchor_frames', 'anchor_boxes', 'anchor_scores', 'grid', 'radius', 'min_conf', 'max_frames', 'step', 'sync', 'ctx']
    d = {k: v.default for k, v in inspect.signature(ops.track_pixels).parameters.items()}
    assert (d['anchor_scores'], d['grid'], d['radius'], d['min_conf'], d['max_frames'], d['step'], d['sync'], d['ctx']) == \
        (None, 32, 8, 0.5, 0, 1, True, None)
    assert list(inspect.signature(track.pixel_tracker).parameters) == ['vid_proto', 'anchor_frame_id', 'bbox', 'opts']
    for name in ('fcn_tracker', 'tld_tracker'):                   # the external trackers keep raising
        with pytest.raises(RuntimeError):
            getattr(track, name)(None, 1, [1, 1, 2, 2], None)


def test_host_tensors_are_refused():
    import torch
    from vdetlib_amd import ops
    img = torch.zeros((2, 8, 8, 3), dtype=torch.uint8)
    fr, bx = torch.ones((1, 1), dtype=torch.int32), torch.tensor([[[2., 2., 5., 5.]]])
    with pytest.raises(ValueError):
        ops.track_pixels(img, fr, bx)
