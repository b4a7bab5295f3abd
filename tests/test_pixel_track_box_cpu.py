"""CPU: ``sampling='box'`` of the rule (tests/pixtrack_spec.py) against hand-written values, against the point rule where
the two must agree, and on the videos the point rule loses (tests/pixtrack_box_cases.py).  The device is compared with this
spec on bits in test_pixel_track_box_gpu.py."""
import math

import numpy as np
import pytest

import pixtrack_box_cases as bc
import pixtrack_spec as px

BOX = dict(sampling='box')


# a. -------------------------------------------------------------------------------------------------------------------
def test_integral_against_a_double_loop():
    rng = np.random.RandomState(7600)
    images = rng.randint(0, 256, size=(2, 5, 7, 3)).astype(np.uint8)
    L = px.luma(images)
    I = px.luma_integral(images)
    assert I.dtype == np.uint32 and I.shape == (2, 6, 8)
    for f in range(2):
        for y in range(6):
            for x in range(8):
                want = sum(int(L[f, r, c]) for r in range(y) for c in range(x))
                assert int(I[f, y, x]) == want, (f, y, x)
    assert not I[:, 0].any() and not I[:, :, 0].any()
    full = px.integral(np.full((1, 4096, 4096), 255, np.uint8))
    assert int(full[0, -1, -1]) == 255 << 24            # the largest entry the rule allows: it fits


def edges(o, e, S, k, N):
    a, b = px.cell_edges(o, e, S, k, N)
    return int(a), int(b)


def test_cell_edges_by_hand():
    # inside: a box of 20 columns from column 10 under side 8 on an image 100 wide: cell 3 is columns 17 .. 19
    assert edges(10, 20, 8, 3, 100) == (17, 20)
    assert edges(10, 20, 8, 0, 100) == (10, 12) and edges(10, 20, 8, 7, 100) == (27, 30)
    # e < S: 5 columns under side 8.  Cell 0 is floor(0/8) .. floor(5/8) = 0 .. 0: empty, so it becomes the single column 10;
    # cell 1 is floor(5/8) .. floor(10/8) = 0 .. 1: column 10; cell 3: floor(15/8) .. floor(20/8) = 1 .. 2: column 11
    assert edges(10, 5, 8, 0, 100) == (10, 11) and edges(10, 5, 8, 1, 100) == (10, 11) and edges(10, 5, 8, 3, 100) == (11, 12)
    # k < 0: floor division.  k = -1: floor(-20/8) = -3 .. 0: columns 7 .. 9;  k = -3: floor(-60/8) = -8 .. floor(-40/8) = -5
    assert edges(10, 20, 8, -1, 100) == (7, 10) and edges(10, 20, 8, -3, 100) == (2, 5)
    # straddling the left border: k = -4: floor(-80/8) = -10 .. floor(-60/8) = -8, from column 0: columns -0 .. 1, the inside part
    assert edges(10, 20, 8, -4, 100) == (0, 2)
    assert edges(3, 20, 8, -1, 100) == (0, 3)           # columns 0 .. 2 of 0 .. 2: exactly at the border
    assert edges(1, 20, 8, -1, 100) == (0, 1)           # columns -2 .. 0: only column 0 is inside
    # straddling the right border: a box from column 90, cell 3 = columns 97 .. 99, cell 4 = 100 .. 102 on an image 101 wide
    assert edges(90, 20, 8, 3, 101) == (97, 100) and edges(90, 20, 8, 4, 101) == (100, 101)
    assert edges(90, 20, 8, 3, 99) == (97, 99)          # columns 97 .. 98 of 97 .. 99
    # wholly outside on the left: the nearest column, 0; on the right: the nearest column, N - 1
    assert edges(10, 20, 8, -5, 100) == (0, 1) and edges(10, 20, 8, -9, 100) == (0, 1)
    assert edges(90, 20, 8, 4, 100) == (99, 100) and edges(90, 20, 8, 9, 100) == (99, 100)
    # the same function serves rows: limit H
    assert edges(-6, 16, 4, 0, 30) == (0, 1) and edges(-6, 16, 4, 1, 30) == (0, 2) and edges(20, 16, 4, 2, 30) == (28, 30)
    # arrays of k
    a, b = px.cell_edges(10, 20, 8, np.arange(-5, 3), 100)
    assert a.tolist() == [0, 0, 2, 5, 7, 10, 12, 15] and b.tolist() == [1, 2, 5, 7, 10, 12, 15, 17]


def test_cell_value_is_the_rounded_mean():
    rng = np.random.RandomState(7601)
    L = rng.randint(0, 256, size=(1, 30, 40)).astype(np.uint8)
    I = px.integral(L)[0]
    box = (-7, 4, 51, 28)              # 59 x 25 under side 4: cells of 14-15 x 6-7 pixels, over the left and the right border
    got = px.sample_box(I, box, 4, -1, 5)
    for i, k in enumerate(range(-1, 5)):
        ra, rb = edges(4, 25, 4, k, 30)
        for j, m in enumerate(range(-1, 5)):
            ca, cb = edges(-7, 59, 4, m, 40)
            cell = L[0, ra:rb, ca:cb].astype(np.int64)
            assert cell.size >= 1 and int(got[i, j]) == (int(cell.sum()) + cell.size // 2) // cell.size, (k, m)


# b. -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", bc.SIZES)
@pytest.mark.parametrize("seed", bc.SEEDS)
def test_sub_cell_motion(seed, w, h):
    """The box rule stays within half a pitch of the planted position on every frame; the point rule, on the same video,
    strays further than one pitch: the videos are ones the point rule loses."""
    images, pos = bc.sub_cell_video(seed, w, h)
    fr, bx = bc.anchor_of(pos, w, h)
    moves = np.diff(pos, axis=0)
    assert np.abs(moves).max() <= 3 and np.abs(moves).min() >= 1 and w / float(bc.S) > 3 and h / float(bc.S) > 3
    box = px.track_pixels(images, fr, bx, None, **BOX, **bc.KW)[0][0, 0]
    point = px.track_pixels(images, fr, bx, None, **bc.KW)[0][0, 0]
    ex, ey = bc.errors(box, pos)
    print("seed %d %dx%d box: max |dx| %g |dy| %g conf >= %.4f" % (seed, w, h, ex.max(), ey.max(), box[:, 4].min()))
    assert np.isfinite(box).all()                       # a row on every frame
    assert ex.max() <= math.ceil(w / float(bc.S) / 2) and ey.max() <= math.ceil(h / float(bc.S) / 2)
    px_, py_ = bc.errors(point, pos)
    print("seed %d %dx%d point: max |dx| %g |dy| %g conf >= %.4f" % (seed, w, h, np.nanmax(px_), np.nanmax(py_), np.nanmin(point[:, 4])))
    assert np.nanmax(px_) > w / float(bc.S) or np.nanmax(py_) > h / float(bc.S)


# c. -------------------------------------------------------------------------------------------------------------------
def test_one_pixel_cells_are_the_point_rule():
    """w == h == S: a cell is a pixel, so the box sampler gives the point sampler's bits -- on chains that touch every image edge:
    the anchors sit in the four corners and on the four sides, partly outside, and the region (R cells around the box) reads
    beyond each edge from the first step on."""
    rng = np.random.RandomState(7602)
    S, R, F, H, W = 8, 3, 6, 20, 24
    images = rng.randint(0, 256, size=(F, H, W, 3)).astype(np.uint8)
    xs, ys = (-3, 8, W - 5), (-3, 6, H - 5)             # 0-based x1 / y1: over the low edge, inside, over the high edge
    boxes = [[x + 1, y + 1, x + S, y + S] for y in ys for x in xs]
    fr = np.array([[1 + k % F for k in range(len(boxes))]], np.int32)
    bx = np.array([boxes], np.float32)
    for kw in (dict(min_conf=0.0), dict(min_conf=0.0, step=2), dict()):
        want = px.track_pixels(images, fr, bx, None, S, R, **kw)
        got = px.track_pixels(images, fr, bx, None, S, R, **BOX, **kw)
        assert not want[3] and not got[3]
        for a, b in zip(got[:3], want[:3]):
            assert a.dtype == b.dtype and np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a,
                                                         b.view(np.uint32) if b.dtype == np.float32 else b)
    live = np.isfinite(want[0][0, :, :, 0])
    assert live.sum(axis=1).min() >= 2                  # every chain walks
    # the sample itself, cell by cell, far outside included
    I = px.luma_integral(images)
    L = px.luma(images)
    for b in ((-3, -3, 4, 4), (W - 5, H - 5, W + 2, H + 2), (-40, 5, -33, 12), (W + 9, H + 9, W + 16, H + 16)):
        assert np.array_equal(px.sample_box(I[0], b, S, -R, S + R), px.sample(L[0], b, S, -R, S + R))


def test_scale_search_and_greedy_loop_run_the_box_chain():
    """scales > 0 and the greedy form run the one walk on the integral; a point walk after it is a point walk still (the
    sampling is the call's, not the module's); with one-pixel cells and scales = 0 the greedy loop is the point loop on bits"""
    import greedy_pixel_cases as gc
    images, pos = bc.sub_cell_video(bc.SEEDS[0], 40, 40)
    fr, bx = bc.anchor_of(pos, 40, 40)
    lumas = px.luma(images)
    rows = px.track_pixels(images, fr, bx, None, scales=1, scale_step=5, **BOX, **bc.KW)[0][0, 0]
    assert np.isfinite(rows).all() and px.track_slot(lumas, 1, (0, 0, 7, 7), 8, 3).shape == rows.shape
    (images, boxes, scores, _, _), _ = gc.main_case()
    sq = boxes.copy()                                   # every proposal made 8 x 8: one pixel per cell
    sq[..., 2], sq[..., 3] = sq[..., 0] + 7, sq[..., 1] + 7
    want = px.track_volume_pixels(images, sq, scores, **gc.MAIN)
    got = px.track_volume_pixels(images, sq, scores, **BOX, **gc.MAIN)
    for a, b in zip(got[:3], want[:3]):
        assert np.array_equal(a, b, equal_nan=True)
    assert int(want[2].sum()) >= 2
