"""CPU-only: the scale search of the pixel tracker's numpy statement (tests/pixtrack_spec.py): scales = 0 against the
defaults and against a walk on ``best_shift``, the step's second, independent winner; numbers worked out by hand; constructed
SAD tables; a planted scene whose object really grows and shrinks; the design of the greedy case; and the C-ABI / python
surface of the device forms (vdet_track_pixels_scaled, vdet_track_volume_pixels_scaled)."""
import ctypes
import inspect
import re

import numpy as np
import pytest

import pixtrack_scale_cases as sc
import pixtrack_spec as px
from pixtrack_harness import ctype_of, header, prototype


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a,
                                                                        b.view(np.uint32) if b.dtype == np.float32 else b)


# ---- a. scales = 0 is the fixed-scale rule ------------------------------------------------------------------------------------

@pytest.mark.parametrize("kw", (dict(min_conf=0.0), dict(), dict(min_conf=0.0, step=3, max_frames=5)))
def test_no_levels_is_the_fixed_scale_rule_on_bits(kw):
    images, fr, bx, scr, _ = sc.mixed_case(8, 2)
    fr, bx = fr.copy(), bx.copy()
    fr[2, 3], bx[2, 3] = 4, [10, 10, 9.5, 30]                  # a bad slot (empty after truncation) ...
    fr[2, 4] = sc.F + 1                                        # ... and a frame outside the video, among the live and the empty ones
    want = px.track_pixels(images, fr, bx, scr, 8, 2, **kw)
    got = px.track_pixels(images, fr, bx, scr, 8, 2, scales=0, scale_step=7, scale_penalty=99, **kw)
    assert want[3] and got[3]
    for a, b in zip(got[:3], want[:3]):
        assert same_bits(a, b)
    # the rule's step is sad_table + pick; the witness walks every live slot with best_shift and holds the two winners
    # against each other on every step it takes
    lumas = px.luma(images)
    steps = []
    for c in range(fr.shape[0]):
        for t in range(fr.shape[1]):
            state, ib = px.anchor_state(fr[c, t], bx[c, t], sc.F, sc.H, sc.W)
            rows = np.full((sc.F, 5), np.nan, np.float32)
            if state == 1:
                rows = best_shift_walk(lumas, int(fr[c, t]), ib, 8, 2, steps=steps, **kw)
            assert same_bits(want[0][c, t], rows), (c, t)
    walked = np.isfinite(want[0][..., 0]).sum()
    assert walked > 30                                          # (the table is not idle: most chains walk)
    assert len(steps) >= walked - (fr > 0).sum()                # every row but the anchors' came from a step held against pick


def best_shift_walk(lumas, frame, box, S, R, min_conf=0.5, max_frames=0, step=1, steps=None):
    """The fixed-scale point chain written out with ``px.best_shift`` as the step's winner: this test's independent witness,
    not a second rule.  On every step taken, best_shift == pick over level 0's sad_table, reduced to (SAD, dy, dx)"""
    F, H, W = lumas.shape
    rows = np.full((F, 5), np.nan, np.float32)
    af = frame - 1
    rows[af] = px.row_of(box, np.float32(1.0))
    Tm = px.sample(lumas[af], box, S, 0, S)
    for d in (1, -1):
        x1, y1, x2, y2 = box
        for n in range(1, px.reach_of(max_frames, F) + 1):
            g = af + d * n * step
            if g < 0 or g >= F:
                break
            Rg = px.sample(lumas[g], (x1, y1, x2, y2), S, -R, S + R)
            sad, dy, dx = px.best_shift(Tm, Rg, R)
            psad, l, pdy, pdx = px.pick({0: px.sad_table(Tm, Rg, R)}, R, 99)
            assert (sad, dy, dx) == (psad, pdy, pdx) and l == 0, (frame, box, g)
            steps.append(g)
            sx, sy = (2 * dx * (x2 - x1 + 1) + S) // (2 * S), (2 * dy * (y2 - y1 + 1) + S) // (2 * S)
            x1, y1, x2, y2 = x1 + sx, y1 + sy, x2 + sx, y2 + sy
            conf = px.confidence(sad, S)
            if conf < np.float32(min_conf) or px.outside((x1, y1, x2, y2), H, W):
                break
            rows[g] = px.row_of((x1, y1, x2, y2), conf)
    return rows


# ---- b. level_box by hand -----------------------------------------------------------------------------------------------------

def widths(w, p, levels, h=None):
    out = []
    for l in levels:
        b = px.level_box((100, 200, 100 + w - 1, 200 + (h or w) - 1), l, p)
        out.append(None if b is None else (b[2] - b[0] + 1, b[3] - b[1] + 1))
    return out


def test_level_box_by_hand():
    # w = 64, p = 5: |l| = 1: (1*5*64 + 100) // 200 = 420 // 200 = 2 a side: 68 / 60; |l| = 2: (640 + 100) // 200 = 3: 70 / 58
    assert widths(64, 5, (1, -1, 2, -2)) == [(68, 68), (60, 60), (70, 70), (58, 58)]
    assert px.level_box((100, 200, 163, 263), 1, 5) == (98, 198, 165, 265)             # about the centre: the same margin each side
    assert px.level_box((100, 200, 163, 263), -2, 5) == (103, 203, 160, 260)
    assert px.level_box((100, 200, 163, 263), 0, 5) == (100, 200, 163, 263)
    # w = 16, p = 5: (80 + 100) // 200 = 0: levels +-1 are the box itself; l = 2: (160 + 100) // 200 = 1: 18
    assert widths(16, 5, (1, -1, 2)) == [(16, 16), (16, 16), (18, 18)]
    # w = 2, p = 25: |l| = 1: (50 + 100) // 200 = 0: the box itself; |l| = 2: (100 + 100) // 200 = 1: l = -2 would be 0 wide: the
    # level is skipped, l = +2 is 4 wide; |l| = 3: (150 + 100) // 200 = 1 likewise
    assert widths(2, 25, (-1, 1, -2, 2, -3, 3)) == [(2, 2), (2, 2), None, (4, 4), None, (4, 4)]
    # w = 5, p = 25, l = -3: (375 + 100) // 200 = 2 a side: width 1; w = 4: (300 + 100) // 200 = 2: width 0: skipped
    assert widths(5, 25, (-3,)) == [(1, 1)] and widths(4, 25, (-3,)) == [None]
    # the 2^21 cap: w = 2^21 - 2 at p = 1: (2097150 + 100) // 200 = 10486 a side: 2^21 + 20970 wide: skipped; the shrunk level is
    # fine.  w = 2^21 - 20972: (2076180 + 100) // 200 = 10381 a side: 2^21 - 210 wide: admissible
    big = 1 << 21
    assert widths(big - 2, 1, (1, -1)) == [None, (big - 2 - 2 * 10486, big - 2 - 2 * 10486)]
    assert widths(big - 20972, 1, (1,)) == [(big - 20972 + 2 * 10381, big - 20972 + 2 * 10381)]
    assert big - 20972 + 2 * 10381 <= big
    # level 0 is admissible whatever the size
    assert px.level_box((0, 0, big + 5, 3), 0, 25) == (0, 0, big + 5, 3)
    # unequal sides, w = 64, h = 16, p = 5: ex = 2, ey = 0 at |l| = 1; ex = 3, ey = 1 at |l| = 2; one side below 1 skips the level:
    # w = 64, h = 2, p = 25, l = -2: ey = (100 + 100) // 200 = 1 -> h_l = 0
    assert widths(64, 5, (1, -1, 2, -2), h=16) == [(68, 16), (60, 16), (70, 18), (58, 14)]
    assert widths(64, 25, (-2, -1), h=2) == [None, (64 - 2 * 8, 2)]


# ---- c. the key's order -------------------------------------------------------------------------------------------------------

def table(R, fill, **cells):
    t = np.full((2 * R + 1, 2 * R + 1), fill, np.int64)
    for k, v in cells.items():
        dy, dx = (int(x) for x in k.replace('m', '-').split('_')[1:])
        t[dy + R, dx + R] = v
    return t


def test_key_order_on_constructed_tables():
    R = 2
    # equal SAD at l = 0 and l = 1 (and at a smaller shift on level 1): level 0 wins -- |l| comes before the shift
    t = {0: table(R, 900, d_1_1=500), 1: table(R, 900, d_0_0=500), -1: table(R, 900)}
    assert px.pick(t, R, 0) == (500, 0, 1, 1)
    # equal at l = -1 and l = +1, same shift: -1 wins (the last field)
    t = {0: table(R, 900), 1: table(R, 900, d_0_1=400), -1: table(R, 900, d_0_1=400)}
    assert px.pick(t, R, 0) == (400, -1, 0, 1)
    # ... but the smaller shift before the level's sign
    t = {0: table(R, 900), 1: table(R, 900, d_0_1=400), -1: table(R, 900, d_1_1=400)}
    assert px.pick(t, R, 0) == (400, 1, 0, 1)
    # among equal |l| and d^2: dy, then dx
    t = {0: table(R, 900, d_1_0=400, d_0_m1=400, d_0_1=400, d_m1_0=400)}
    assert px.pick(t, R, 0) == (400, 0, -1, 0)
    # a penalty that flips a winner: level 2 is 100 better; q = 49: 2*49 = 98 < 100, level 2 still wins; q = 50 ties the
    # penalised SADs and |l| decides for level 0; q = 51 level 0 wins outright.  The SAD returned is the RAW one
    t = {0: table(R, 900, d_0_0=600), 2: table(R, 900, d_1_0=500), -2: table(R, 900)}
    assert px.pick(t, R, 0) == (500, 2, 1, 0)
    assert px.pick(t, R, 49) == (500, 2, 1, 0)
    assert px.pick(t, R, 50) == (600, 0, 0, 0)
    assert px.pick(t, R, 51) == (600, 0, 0, 0)
    # a level that was skipped is not in the tables at all
    assert px.pick({0: table(R, 7)}, R, 65535) == (7, 0, 0, 0)


def test_confidence_is_the_raw_sad_s():
    """A flat frame against a template that differs by 3 on every cell: every shift of every level has SAD 3 * 16 = 48.  Level 0
    wins; the step reports SAD 48 and conf 1 - 48/4080 whatever the penalty.  Where a penalised level wins (constructed tables:
    300 + 150 < 500), the SAD handed to the confidence is the raw 300."""
    S, R = 4, 1
    L = np.full((40, 40), 90, np.uint8)
    Tm = np.full((S, S), 93, np.uint8)
    for q in (0, 1000, 65535):
        box, conf, won, sad = px.step_once(Tm, L, (10, 10, 29, 29), S, R, 2, 10, q)
        assert (box, won, sad) == ((10, 10, 29, 29), (0, 0, 0), 48) and conf == np.float32(1.0) - np.float32(48) / np.float32(4080)
    t = {0: np.full((3, 3), 500, np.int64), 1: np.full((3, 3), 300, np.int64)}
    raw, l, dy, dx = px.pick(t, R, 150)
    assert (raw, l, dy, dx) == (300, 1, 0, 0)
    assert px.confidence(raw, S) == np.float32(1.0) - np.float32(300) / np.float32(4080)


def test_step_moves_the_level_box():
    """The move is applied to the winner's level box with ITS size: w = 20, p = 10, level +1 -> (9,9,30,30), w_l = 22, S = 4:
    dx = +1 moves by (2*22 + 4) // 8 = 6, dy = -1 by (-44 + 4) // 8 = -5."""
    S, R = 4, 1
    rng = np.random.RandomState(5)
    L = rng.randint(0, 256, size=(60, 60)).astype(np.uint8)
    Tm = px.sample(L, (9, 9, 30, 30), S, -1, S + 1)[0:4, 2:6]   # the level-1 grid one cell up and one to the right: rows k = -1..2, columns k = 1..4
    box, conf, won, sad = px.step_once(Tm, L, (10, 10, 29, 29), S, R, 1, 10, 0)
    assert won == (1, -1, 1) and sad == 0 and conf == np.float32(1.0)
    assert box == (9 + 6, 9 - 5, 30 + 6, 30 - 5)


# ---- d. the planted scene -----------------------------------------------------------------------------------------------------

def scene_runs(kind):
    images, truth = sc.scene(kind)
    fr, bx = sc.anchor_of(truth)
    fixed = px.track_pixels(images, fr, bx, None, sc.S, sc.R, 0.0)[0][0, 0]
    trace = {}
    rows = px.track_slot(px.luma(images), 1, tuple(int(v) for v in truth[0]), sc.S, sc.R, 0.0, 0, 1, 1, 5, 0, trace=trace)
    assert np.isfinite(fixed).all() and np.isfinite(rows).all()            # min_conf = 0: both chains reach the last frame
    return truth, fixed, rows, trace


@pytest.mark.parametrize("kind", ("grow", "shrink"))
def test_planted_object_that_changes_size(kind):
    """Grid 32, radius 8, scales = 1, scale_step = 5, min_conf = 0, anchored on the first frame.  Measured here, largest
    coordinate error against the true boxes: growing 21 px fixed-scale / 1 px scaled; shrinking 58 px / 2 px."""
    truth, fixed, rows, trace = scene_runs(kind)
    e_fixed, e_scaled = sc.largest_error(fixed, truth), sc.largest_error(rows, truth)
    print("%s: fixed-scale %g px, scaled %g px, levels %s" % (kind, e_fixed, e_scaled, [trace[g][0] for g in sorted(trace)]))
    assert e_fixed >= 15                     # the ground: without the search the box is wrong
    assert e_scaled <= 4
    sign = 1 if kind == 'grow' else -1
    assert all(sign * trace[g][0] >= 0 for g in trace) and sum(trace[g][0] != 0 for g in trace) >= 8


def test_constant_size_mover_stays_on_level_zero():
    """Measured: 1 px with and without the search; level 0 on every step, so the two rules give the same rows."""
    truth, fixed, rows, trace = scene_runs('const')
    assert sorted(trace) == list(range(1, sc.F)) and all(trace[g][0] == 0 for g in trace)
    assert same_bits(rows, fixed) and sc.largest_error(rows, truth) <= 4


# ---- e. the greedy case is what it says ---------------------------------------------------------------------------------------

def test_greedy_case_design():
    images, boxes, scores, truth = sc.greedy_case()
    assert images.shape == (sc.F, sc.H, sc.W, 3) and boxes.shape == (sc.F, sc.GB, 4) and scores.shape == (sc.F, sc.GB, sc.GC)
    (tracks, anchors, nt, bad), (ftracks, fanchors, fnt, fbad) = sc.greedy_specs()
    assert not bad and not fbad and nt.tolist() == [3, 1] and fnt.tolist() == [3, 1]
    # both loops start from A's true box on frame 1, then B's on frame 6
    for a in (anchors, fanchors):
        assert a[0, 0].tolist() == [1, sc.GIA, np.float32(0.99)] and a[0, 1].tolist() == [6, sc.GIB, np.float32(0.95)]
    late = range(sc.F - 4, sc.F)
    A = (sc.GIA,) + sc.GIJA
    # with the search, A's tubelet covers the true-size proposals on the late frames (IoU >= nms_thres): all suppressed, and
    # the third anchor is a distractor
    for f in late:
        for i in A:
            assert sc._iou(tracks[0, 0, f, :4], boxes[f, i]) >= sc.GREEDY['nms_thres'], (f, i)
    assert int(anchors[0, 2, 1]) in sc.GIDIS and anchors[0, 2, 2] < 0.5
    # without it the anchor frame's box misses A's true box on the last frame, and one of A's late proposals is the third anchor
    assert sc._iou(ftracks[0, 0, sc.F - 1, :4], boxes[sc.F - 1, sc.GIA]) < sc.GREEDY['nms_thres']
    assert int(fanchors[0, 2, 1]) in A and fanchors[0, 2, 0] - 1 in late and fanchors[0, 2, 2] > 0.5
    # B keeps its size: its tubelet is the same under both rules
    assert same_bits(tracks[0, 1], ftracks[0, 1]) and same_bits(tracks[1, 0], ftracks[1, 0])


# ---- f. the binding -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ("vdet_track_pixels", "vdet_track_volume_pixels"))
def test_header_prototypes_and_symbol_rows(name):
    from vdetlib_amd import _lib
    parent, proto = prototype(name), prototype(name + '_scaled')
    k = [a.split()[-1] for a in parent].index('step') + 1
    assert proto == parent[:k] + ['int scales', 'int scale_step', 'int scale_penalty'] + parent[k:]
    res, args = _lib.SYMBOLS[name + '_scaled']
    assert res is ctypes.c_int and args == [ctype_of(a) for a in proto]
    pres, pargs = _lib.SYMBOLS[name]
    assert args == pargs[:k] + [ctypes.c_int] * 3 + pargs[k:]


def test_null_context_refused():
    from vdetlib_amd import _lib
    L = _lib.load_library()
    z = None
    assert L.vdet_track_pixels_scaled(z, z, 1, 8, 8, z, z, z, 1, 1, 8, 2, 0.5, 0, 1, 1, 5, 0, z, z, z) == _lib.VDET_EINVAL
    assert L.vdet_track_volume_pixels_scaled(z, z, 8, 8, z, z, 1, 1, 1, 0.3, 0.0, 1, 8, 2, 0.5, 0, 1, 1, 5, 0, z, z, z) == _lib.VDET_EINVAL


def test_limits_table_row():
    head = header().split('#ifndef VDET_HIP_H')[0]
    m = re.search(r'\n \*   pixel tracker with scale search(.*?)\n \*/', head, flags=re.S)
    assert m, "the limits table has no 'pixel tracker with scale search' row"
    row = re.sub(r'\s*\n \*\s*', ' ', m.group(1))
    for part in ('vdet_track_pixels_scaled', 'vdet_track_volume_pixels_scaled', '0 <= scales <= 3', '1 <= scale_step <= 25',
                 '0 <= scale_penalty <= 65535', 'VDET_EINVAL', '2^21', 'skipped'):
        assert part in row, part


def test_python_surface():
    from vdetlib_amd import ops
    sig = inspect.signature(ops.track_pixels_scaled).parameters
    assert list(sig) == ['images', 'anchor_frames', 'anchor_boxes', 'anchor_scores', 'grid', 'radius', 'min_conf', 'max_frames', 'step',
                         'scales', 'scale_step', 'scale_penalty', 'sync', 'ctx']
    assert [sig[k].default for k in list(sig)[3:]] == [None, 32, 8, 0.5, 0, 1, 1, 5, 0, True, None]
    sig = inspect.signature(ops.track_volume_pixels_scaled).parameters
    assert list(sig) == ['images', 'boxes', 'scores', 'nms_thres', 'thres', 'max_tracks', 'grid', 'radius', 'min_conf', 'max_frames',
                         'step', 'scales', 'scale_step', 'scale_penalty', 'sync', 'ctx']
    assert [sig[k].default for k in list(sig)[3:]] == [0.3, 0.0, 10, 32, 8, 0.5, 0, 1, 1, 5, 0, True, None]
    # the parents keep theirs
    assert 'scales' not in inspect.signature(ops.track_pixels).parameters
    assert 'scales' not in inspect.signature(ops.track_volume_pixels).parameters


def test_host_tensors_are_refused():
    import torch
    from vdetlib_amd import ops
    img = torch.zeros((2, 8, 8, 3), dtype=torch.uint8)
    fr, bx = torch.ones((1, 1), dtype=torch.int32), torch.tensor([[[2., 2., 5., 5.]]])
    with pytest.raises(ValueError):
        ops.track_pixels_scaled(img, fr, bx)
    with pytest.raises(ValueError):
        ops.track_volume_pixels_scaled(img, torch.zeros((2, 3, 4)), torch.zeros((2, 3, 1)))
