"""CPU-only: the numpy statement of the R-CNN window warp (tests/patch_spec.py) against numbers worked out by hand, and the
C-ABI / dict-level surface of the device form (vdet_rcnn_patches, vdet_tubelet_patches)."""
import ctypes
import os
import re

import numpy as np
import pytest

import patch_spec as ps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 37, 53          # image rows, columns
S, P = 8, 2            # crop_size, padding: scale = 8 / (8 - 4) is exactly 2


def _geom(box, mode='warp', s=S, p=P):
    g = ps.geometry(box, H, W, mode, s, p)
    return (g['ok'], g['x1'], g['y1'], g['src_w'], g['src_h'], g['crop_w'], g['crop_h'], g['pad_w'], g['pad_h'])


def test_round_half_away():
    assert [ps.round_half_away(v) for v in (2.5, -0.5, 0.5, -2.5, 1.5, -1.5, 3.49, -3.49, 0.0)] == [3, -1, 1, -3, 2, -2, 3, -3, 0]


def test_geometry_half_corners():
    """bbox = box - 1, half = (x2-x1+1)/2, corner = centre -+ 2*half, rounded half AWAY from zero."""
    # [3,3,5,5] -> [2,2,4,4], half 1.5, centre 3.5: corners 0.5 -> 1 and 6.5 -> 7 (half-to-even would give 0 and 6)
    assert _geom([3, 3, 5, 5]) == (1, 1, 1, 7, 7, 8, 8, 0, 0)
    # [2,2,4,4] -> [1,1,3,3], centre 2.5: corners -0.5 -> -1 and 5.5 -> 6; unclipped 8, pad 1, clipped 0..6 = 7, scale 1
    assert _geom([2, 2, 4, 4]) == (1, 0, 0, 7, 7, 7, 7, 1, 1)
    # [1,1,3,3] -> [0,0,2,2], centre 1.5: corners -1.5 -> -2 and 4.5 -> 5; unclipped 8, pad 2, clipped 0..5 = 6
    assert _geom([1, 1, 3, 3]) == (1, 0, 0, 6, 6, 6, 6, 2, 2)


def test_geometry_overhang_each_edge():
    # left: [-5,10,10,20] -> [-6,9,9,19]; hw 8, hh 5.5; centre (2, 14.5); x -14..18 (33), y 3.5 -> 4 .. 25.5 -> 26 (23)
    # pad_x1 14, clipped x 0..18 = 19: crop_w = round(19*8/33 = 4.61) = 5, pad_w = round(14*8/33 = 3.39) = 3; crop_h = 8
    assert _geom([-5, 10, 10, 20]) == (1, 0, 4, 19, 23, 5, 8, 3, 0)
    # top: [10,-4,20,9] -> [9,-5,19,8]; centre (14.5, 2); x 4..26 (23); y -12..16 (29), pad_y1 12, clipped 17:
    # crop_h = round(17*8/29 = 4.69) = 5, pad_h = round(12*8/29 = 3.31) = 3
    assert _geom([10, -4, 20, 9]) == (1, 4, 0, 23, 17, 8, 5, 0, 3)
    # right: [45,10,60,20] -> [44,9,59,19]; centre x 52: 36..68 (33), clipped 36..52 = 17: crop_w = round(4.12) = 4
    assert _geom([45, 10, 60, 20]) == (1, 36, 4, 17, 23, 4, 8, 0, 0)
    # bottom: [10,30,20,45] -> [9,29,19,44]; centre y 37: 21..53 (33), clipped 21..36 = 16: crop_h = round(3.88) = 4
    assert _geom([10, 30, 20, 45]) == (1, 4, 21, 23, 16, 8, 4, 0, 0)


def test_geometry_larger_than_image():
    # [-10,-10,70,50] -> [-11,-11,69,49]; hw 40.5, centre 29.5: -51.5 -> -52 .. 110.5 -> 111 (164); hh 30.5, centre 19.5:
    # -41.5 -> -42 .. 80.5 -> 81 (124).  clipped 53 x 37.  crop_w = round(53*8/164 = 2.59) = 3, crop_h = round(37*8/124 = 2.39) = 2,
    # pad_w = round(52*8/164 = 2.54) = 3, pad_h = round(42*8/124 = 2.71) = 3
    assert _geom([-10, -10, 70, 50]) == (1, 0, 0, 53, 37, 3, 2, 3, 3)


def test_geometry_clamp_fires():
    # [3.75,11,10.25,18] -> [2.75,10,9.25,17]; hw 3.75, centre 6.5: corners -1 and 14, unclipped 16, scale_x 0.5; pad_x1 1 ->
    # round(0.5) = 1; clipped 0..14 = 15 -> round(7.5) = 8; 1 + 8 > 8: crop_w = 7.  y: hh 4, centre 14: 6..22 (17), crop_h 8
    assert _geom([3.75, 11, 10.25, 18]) == (1, 0, 6, 15, 17, 7, 8, 1, 0)


def test_geometry_outside_and_degenerate():
    for box in ([100, 100, 120, 120], [-50, -50, -30, -30], [30, 25, 10, 8], [float('nan'), 1, 5, 5], [1, 1, float('inf'), 5],
                [-1e308, 1, 1e308, 5]):
        assert _geom(box)[0] == 0, box
    patch, ok = ps.rcnn_window(np.full((H, W, 3), 9, np.uint8), [100, 100, 120, 120], 'warp', S, P, None)
    assert ok == 0 and not patch.any()


def test_geometry_square():
    # [5,10,34,19] -> [4,9,33,18]: hw 15, hh 5 (3:1), centre (19, 14).  square: both halves 15: x -11..49, y -16..44 (61 each);
    # pad 11 / 16, clipped 50 x 37: crop_w = round(50*8/61 = 6.56) = 7, crop_h = round(37*8/61 = 4.85) = 5, pad_w = round(1.44)
    # = 1, pad_h = round(2.10) = 2
    assert _geom([5, 10, 34, 19], 'square') == (1, 0, 0, 50, 37, 7, 5, 1, 2)
    # warp keeps hh 5: y 4..24 (21), inside the image
    assert _geom([5, 10, 34, 19], 'warp') == (1, 0, 4, 50, 21, 7, 8, 1, 0)


def test_geometry_warp_without_padding():
    # corners truncated towards zero; a window that leaves the image is flagged, not sliced
    assert _geom([10.9, 8.2, 30.7, 25.5], 'warp', 12, 0) == (1, 9, 7, 21, 18, 12, 12, 0, 0)
    assert _geom([1, 1, 53, 37], 'warp', 12, 0) == (1, 0, 0, 53, 37, 12, 12, 0, 0)
    for box in ([0, 5, 10, 10], [5, 5, 54, 10], [5, 5, 10, 38], [-3, 5, 10, 10], [30, 5, 10, 10]):
        assert _geom(box, 'warp', 12, 0)[0] == 0, box
    assert _geom([0.5, 5, 10, 10], 'warp', 12, 0)[0] == 1          # -0.5 truncates to 0


def test_resize_identity_and_constant():
    rng = np.random.RandomState(0)
    win = rng.randint(0, 256, size=(5, 7, 3)).astype(np.uint8)
    assert np.array_equal(ps.resize_linear(win, 7, 5), win.astype(np.float64))
    img = np.full((H, W, 3), 200, np.uint8)
    mean = np.array([103.939, 116.779, 123.68])
    # [2,2,4,4]: the 7 x 7 window keeps its size and is placed at (1, 1) (see above): constant - mean there, exactly
    patch, ok = ps.rcnn_window(img, [2, 2, 4, 4], 'warp', S, P, mean)
    assert ok == 1 and patch.dtype == np.float32 and patch.shape == (S, S, 3)
    inside = np.zeros((S, S), bool)
    inside[1:8, 1:8] = True
    for k in range(3):
        assert np.array_equal(patch[..., k][inside], np.full(inside.sum(), np.float32(200.0 - mean[k])))
        assert not patch[..., k][~inside].any()
    # [-5,10,10,20]: 19 x 23 -> 5 x 8 at column 3 (see above).  The f32 weights 1.f - fx and fx sum to 1 within 2^-25 per pass,
    # so the blend of a constant is the constant within 2 * 200 * 2^-25 = 1.2e-5, plus half an f32 ulp at 96 (3.8e-6)
    patch, ok = ps.rcnn_window(img, [-5, 10, 10, 20], 'warp', S, P, mean)
    inside[:] = False
    inside[0:8, 3:8] = True
    for k in range(3):
        assert np.abs(patch[..., k][inside].astype(np.float64) - (200.0 - mean[k])).max() <= 1.6e-5
        assert not patch[..., k][~inside].any()
    assert np.array_equal(ps.rcnn_window(img, [-5, 10, 10, 20], 'warp', S, P, None)[0][..., 0][~inside], np.zeros((~inside).sum(), np.float32))


def test_resize_hand_values():
    # 2 -> 4: fx = (d + .5)*.5 - .5 = -.25, .25, .75, 1.25 -> S0, .75*S0 + .25*S1, .25*S0 + .75*S1, S1 (clamped at both ends)
    win = np.array([[0, 100], [200, 40]], dtype=np.uint8)[:, :, None]
    want = np.array([[0, 25, 75, 100], [50, 58.75, 76.25, 85], [150, 126.25, 78.75, 55], [200, 160, 80, 40]])
    assert np.array_equal(ps.resize_linear(win, 4, 4)[..., 0], want)
    # 5 -> 2: fx = .5*2.5 - .5 = .75 and 1.5*2.5 - .5 = 3.25: .25*S0 + .75*S1, .75*S3 + .25*S4 (two taps: no area averaging)
    row = np.array([[10, 20, 30, 40, 50]], dtype=np.uint8)[:, :, None]
    assert np.array_equal(ps.resize_linear(row, 2, 1)[0, :, 0], np.array([17.5, 42.5]))
    col = row.transpose(1, 0, 2)
    assert np.array_equal(ps.resize_linear(col, 1, 2)[:, 0, 0], np.array([17.5, 42.5]))


def test_resize_matches_opencv():
    """The spec's resize against cv2.resize(window.astype('float'), ..., INTER_LINEAR), exactly.  SKIPS wherever OpenCV is not
    installed -- which includes every machine this project is built and tested on -- and is evidence of nothing until someone
    runs it with OpenCV: parity of the fixed resize rule with OpenCV is unpinned."""
    cv2 = pytest.importorskip('cv2')
    rng = np.random.RandomState(1)
    for (h, w, dh, dw) in ((5, 7, 8, 8), (23, 19, 5, 8), (37, 53, 224, 192), (2, 2, 4, 4), (1, 5, 3, 2), (17, 15, 8, 7)):
        win = rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8)
        got = cv2.resize(win.astype('float'), (dw, dh), interpolation=cv2.INTER_LINEAR).astype('float')
        assert np.array_equal(ps.resize_linear(win, dw, dh), got), (h, w, dh, dw)


def test_sampling_and_slots_spec():
    b = np.array([[10., 20., 30., 60.]])
    off = np.array([[[0.05, -0.05, 0.0, 0.01]]])
    assert np.array_equal(ps.sampling_boxes(b, off), np.array([[[10, 20, 30, 60], [10 + 0.05 * 20, 20 - 0.05 * 40, 30, 60 + 0.01 * 40]]]))
    tr = np.zeros((2, 2, 3, 5), np.float32)
    tr[0, 1, 1, 0] = np.nan
    assert ps.tubelet_slots(tr, [2, 1], 0, 3).tolist() == [[0, 0, 0], [0, 1, 0], [1, 0, 0], [0, 0, 1], [1, 0, 1], [0, 0, 2], [0, 1, 2],
                                                           [1, 0, 2]]


# ---- the C-ABI and the dict level ------------------------------------------------------------------------------------------

def _prototype(name):
    src = open(os.path.join(ROOT, 'include', 'vdet_hip.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    m = re.search(r'\bint\s+%s\s*\(([^;]*?)\)\s*;' % name, src, flags=re.S)
    assert m, "%s is not declared in include/vdet_hip.h" % name
    return [re.sub(r'\s+', ' ', a).strip() for a in m.group(1).split(',')]


def _ctype_of(arg):
    if '*' in arg:
        return ctypes.c_void_p
    return {'int': ctypes.c_int, 'int64_t': ctypes.c_int64, 'double': ctypes.c_double, 'float': ctypes.c_float}[arg.split()[-2]]


def test_header_prototypes_and_symbol_rows():
    from vdetlib_amd import _lib
    rp = _prototype('vdet_rcnn_patches')
    assert rp[0] == 'vdet_ctx *ctx' and rp[1] == 'const uint8_t *d_images'
    assert [a.split()[-1].lstrip('*') for a in rp[2:]] == ['Fi', 'H', 'W', 'd_boxes', 'boxes_f64', 'N', 'd_image_idx', 'd_offsets', 'num',
                                                           'd_mean', 'S', 'padding', 'mode', 'out_dtype', 'd_patches', 'd_ok', 'd_sboxes']
    tp = _prototype('vdet_tubelet_patches')
    assert [a.split()[-1].lstrip('*') for a in tp] == ['ctx', 'd_images', 'Fi', 'H', 'W', 'd_tracks', 'tracks_f64', 'C', 'T', 'F', 'ld',
                                                       'd_ntracks', 'f0', 'f1', 'cap', 'd_mean', 'S', 'padding', 'mode', 'out_dtype',
                                                       'd_patches', 'd_ok', 'd_slot', 'd_count']
    for name, proto in (('vdet_rcnn_patches', rp), ('vdet_tubelet_patches', tp)):
        res, args = _lib.SYMBOLS[name]
        assert res is ctypes.c_int
        assert args == [_ctype_of(a) for a in proto], name


def test_null_context_refused():
    from vdetlib_amd import _lib
    L = _lib.load_library()
    z = None
    assert L.vdet_rcnn_patches(z, z, 1, 4, 4, z, 0, 1, z, z, 0, z, 8, 2, 0, 0, z, z, z) == _lib.VDET_EINVAL
    assert L.vdet_tubelet_patches(z, z, 1, 4, 4, z, 0, 1, 1, 1, 5, z, 0, 1, 1, z, 8, 2, 0, 0, z, z, z, z) == _lib.VDET_EINVAL


def test_dict_level_needs_gpu():
    """Without a GPU the dict level raises -- there is no CPU fallback."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from vdetlib_amd.utils.common import rcnn_img_crop
    from vdetlib_amd.vdet.image_det import googlenet_features
    img = np.zeros((H, W, 3), np.uint8)
    with pytest.raises(RuntimeError):
        rcnn_img_crop(img, np.array([3., 3., 9., 9.]), 'warp', S, P, None)
    with pytest.raises(RuntimeError):
        googlenet_features(img, np.array([[3., 3., 9., 9.]]), object(), 'pool5')


def test_im_transform():
    from vdetlib_amd.utils.common import im_transform
    a = np.arange(24, dtype=np.float32).reshape(2, 4, 3)
    got = im_transform(a, mean_values=[1., 2., 3.])
    assert got.shape == (3, 2, 4) and np.array_equal(got, (a - np.array([1., 2., 3.])).transpose(2, 0, 1))
