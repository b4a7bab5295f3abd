"""CPU: the template update with an anchor guard of the pixel tracker's rule (tests/pixtrack_adapt_spec.py) against
tests/pixtrack_spec.py where the two must agree, against numbers worked out by hand, and on the videos a fixed template loses
and an unguarded update loses (tests/pixtrack_adapt_cases.py); then the binding.  The device is compared with this spec on bits
in test_pixel_track_adapt_gpu.py.
  a. the restated loops against pixtrack_spec;  b. the update formula by hand;  c. the morph and the passenger video;
  d. the backward chain;  e. the binding."""
import ctypes
import inspect
import re

import numpy as np
import pytest

import pixtrack_adapt_cases as ac
import pixtrack_adapt_spec as pa
import pixtrack_cases as pc
import pixtrack_spec as px
from pixtrack_harness import bits_equal, ctype_of, header, prototype

OFF = (dict(update=0), dict(update=128, update_conf=2.0), dict(update=128, drift_conf=2.0))


def same(got, want):
    assert got[3] == want[3]
    for k, name in enumerate(('tracks', 'anchors', 'ntracks')):
        assert bits_equal(got[k], want[k]), name


def greedy_volume(S, R):
    """proposals on mixed_case(S, R)'s frames, B = 3: the planted mover's true box, the 37 x 53 object's, one of the boxes over
    an edge; seeded scores for two classes"""
    images, fr, bx, _, pos, (w, h) = pc.mixed_case(S, R)
    F = images.shape[0]
    boxes = np.zeros((F, 3, 4), np.float32)
    for f in range(F):
        boxes[f, 0] = [pos[f, 0] + 1, pos[f, 1] + 1, pos[f, 0] + w, pos[f, 1] + h]
        boxes[f, 1] = [5 + 3 * f + 1, 10 + 2 * f + 1, 5 + 3 * f + 37, 10 + 2 * f + 53]
        boxes[f, 2] = bx[1, f % 5]
    scores = np.random.RandomState(8300 + S).uniform(0.05, 0.95, size=(F, 3, 2)).astype(np.float32)
    return images, boxes, scores


# a. -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sampling", ("point", "box"))
@pytest.mark.parametrize("scales", (0, 1))
def test_no_update_is_the_fixed_template_rule_on_bits(sampling, scales):
    """pins track_slot, step_regions and the greedy loop, which restate pixtrack_spec's: with update = 0, and with an
    update_conf or a drift_conf that no step reaches, every bit is the fixed-template rule's"""
    S, R = 8, 2
    images, fr, bx, scr, _, _ = pc.mixed_case(S, R)
    kw = dict(grid=S, radius=R, scales=scales, scale_step=10, sampling=sampling)
    want = px.track_pixels(images, fr, bx, scr, **kw)
    assert np.isfinite(want[0][..., 0]).sum() >= 30
    gimages, gboxes, gscores = greedy_volume(S, R)
    gkw = dict(kw, nms_thres=0.3, thres=0.3, max_tracks=3, min_conf=0.3)
    gwant = px.track_volume_pixels(gimages, gboxes, gscores, **gkw)
    assert int(gwant[2].sum()) >= 4
    for off in OFF:
        same(pa.track_pixels(images, fr, bx, scr, **dict(kw, **off)), want)
        same(pa.track_volume_pixels(gimages, gboxes, gscores, **dict(gkw, **off)), gwant)
    same(pa.track_pixels(images, fr, bx, scr, step=3, max_frames=5, **kw), px.track_pixels(images, fr, bx, scr, step=3, max_frames=5, **kw))
    # and an update that is accepted changes the rows: the keywords reach the walk
    moved = pa.track_pixels(images, fr, bx, scr, update=256, update_conf=0.0, drift_conf=0.0, **kw)
    assert not bits_equal(moved[0], want[0])


# b. -------------------------------------------------------------------------------------------------------------------
def test_update_formula_by_hand():
    S = 4
    tm0 = np.zeros((S, S), np.uint8)
    tm0[0] = (0, 255, 100, 101)
    A = pa.initial_state(tm0)
    assert A[0].tolist() == [0, 65280, 25600, 25856] and np.array_equal(pa.template_of(A), tm0)
    P = np.zeros((S, S), np.uint8)
    P[0] = (255, 0, 101, 100)
    # a = 1: (255 * A + 1 * (P << 8) + 128) >> 8
    #   cell 0: (0 + 65280 + 128) >> 8 = 255;  cell 1: (255 * 65280 + 0 + 128) >> 8 = 16646528 >> 8 = 65025
    #   cell 2: (255 * 25600 + 25856 + 128) >> 8 = 6553984 >> 8 = 25601;  cell 3: (255 * 25856 + 25600 + 128) >> 8 = 6619008 >> 8 = 25855
    assert pa.updated(A, P, 1)[0].tolist() == [255, 65025, 25601, 25855]
    assert pa.template_of(pa.updated(A, P, 1))[0].tolist() == [1, 254, 100, 101]
    # a = 128: the mean of A and P << 8, rounded: (128 * 0 + 128 * 65280 + 128) >> 8 = 32640 (+ 0.5 truncated)
    assert pa.updated(A, P, 128)[0].tolist() == [32640, 32640, 25728, 25728]
    assert pa.template_of(pa.updated(A, P, 128))[0].tolist() == [128, 128, 101, 101]        # (32640 + 128) >> 8 = 128; 25856 >> 8 = 101
    # a = 255: (1 * A + 255 * (P << 8) + 128) >> 8: cell 0: 16646528 >> 8 = 65025, cell 1: (65280 + 128) >> 8 = 255
    #   cell 2: (25600 + 255 * 25856 + 128) >> 8 = 6619008 >> 8 = 25855;  cell 3: (25856 + 255 * 25600 + 128) >> 8 = 25601
    assert pa.updated(A, P, 255)[0].tolist() == [65025, 255, 25855, 25601]
    # a = 256: A = P << 8 exactly, the largest intermediate 256 * 65280 + 128 included
    assert np.array_equal(pa.updated(A, P, 256), P.astype(np.int64) << 8)
    full = np.full((S, S), 255, np.uint8)
    assert np.array_equal(pa.updated(pa.initial_state(full), full, 256), np.full((S, S), 65280)) and 256 * 65280 + 128 < 2 ** 32
    for a in (1, 128, 255, 256):             # a fixed point: P == Tm leaves the state alone at both ends of the range
        for v in (0, 255):
            c = np.full((S, S), v, np.uint8)
            assert np.array_equal(pa.updated(pa.initial_state(c), c, a), pa.initial_state(c))


def test_the_8_8_state_moves_where_a_uint8_state_stalls():
    """a = 16 towards a patch 7 grey levels up: a uint8 state would add (16 * 7 + 128) >> 8 = 0 on every step, for ever; the
    8.8 state adds 16 * 7 = 112 / 256 of a level a step and the template it shows moves after two steps"""
    S, a = 4, 16
    tm = np.full((S, S), 100, np.uint8)
    P = np.full((S, S), 107, np.uint8)
    stalled = ((256 - a) * tm.astype(np.int64) + a * P.astype(np.int64) + 128) >> 8
    assert np.array_equal(stalled, tm)
    A = pa.initial_state(tm)
    seen = []
    for _ in range(40):
        A = pa.updated(A, P, a)
        seen.append(int(pa.template_of(A)[0, 0]))
    # by hand: A = 25600 -> (240 * 25600 + 16 * 27392 + 128) >> 8 = 25712 -> 25817: Tm = (25712 + 128) >> 8 = 100, (25817 + 128) >> 8 = 101
    assert seen[:2] == [100, 101] and seen == sorted(seen) and seen[-1] >= 106


# c. -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,R,obj", ac.SIZES)
def test_morph_video(S, R, obj):
    """the object's texture changes into another: the fixed template does NOT reach the last frame on the planted position,
    the updated one does, with zero error on every row"""
    images, pos = ac.morph_video(S, R, obj)
    fr, bx = ac.anchor_of(pos, obj)
    kw = dict(grid=S, radius=R, min_conf=0.8)
    fixed = px.track_pixels(images, fr, bx, None, **kw)[0][0, 0]
    err = ac.errors(fixed, pos)
    print("grid %d fixed: rows %d, last error %s" % (S, np.isfinite(err).sum(), err[-1]))
    assert not err[-1] == 0                              # no row there, or a row off the planted position
    for a in (64, 128):
        rows = pa.track_pixels(images, fr, bx, None, update=a, update_conf=0.8, drift_conf=0.0, **kw)[0][0, 0]
        print("grid %d update %d: conf %.4f .. %.4f" % (S, a, rows[1:, 4].min(), rows[1:, 4].max()))
        assert np.isfinite(rows).all() and ac.errors(rows, pos).max() == 0
        assert rows[1:, 4].min() > 0.9


@pytest.mark.parametrize("S,R,obj", ac.SIZES)
def test_passenger_video(S, R, obj):
    """a foreign patch rides on the object's right half, then stays behind: the unguarded update ends off the object, the
    guarded one is on it on every row, as the fixed template is.  The guard's value comes from the spec's own trace: half way
    between the largest c0 of a window the passenger sits on and the smallest c0 before it came"""
    images, pos = ac.passenger_video(S, R, obj)
    fr, bx = ac.anchor_of(pos, obj)
    kw = dict(grid=S, radius=R, min_conf=0.7)
    fixed = pa.track_pixels(images, fr, bx, None, **kw)[0][0, 0]
    assert np.isfinite(fixed).all() and ac.errors(fixed, pos).max() == 0
    guard = ac.passenger_guard(S, R, obj)
    _, ridden, before = ac._cache[('guard', S, R, obj, 0.7)]
    print("grid %d: c0 under the passenger <= %.4f, before it >= %.4f: drift_conf = %.4f" % (S, ridden, before, guard))
    assert ridden < guard < before
    up = dict(update=128, update_conf=0.7)
    loose = pa.track_pixels(images, fr, bx, None, drift_conf=-1.0, **dict(kw, **up))[0][0, 0]
    err = ac.errors(loose, pos)
    print("grid %d unguarded: error per frame %s" % (S, err.tolist()))
    assert np.isfinite(loose).all() and err[:ac.RIDE_FROM + ac.RIDE].max() == 0 and err[-1] >= obj // 2       # it stayed with the patch
    traces = {}
    held = pa.track_pixels(images, fr, bx, None, drift_conf=guard, traces=traces, **dict(kw, **up))[0][0, 0]
    assert np.isfinite(held).all() and ac.errors(held, pos).max() == 0
    acc = [traces[(0, 0)][f][5] for f in range(1, ac.F)]
    assert not any(acc[ac.RIDE_FROM - 1:ac.RIDE_FROM + ac.RIDE - 1]) and all(acc[:ac.RIDE_FROM - 1])


# d. -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sampling", ("point", "box"))
def test_backward_chain_starts_from_the_anchor_s_template(sampling):
    """a slot anchored mid-video: its backward rows are the forward rows of the same anchor on the reversed video, so the
    backward chain cannot have started from what the forward chain made of the template"""
    S, R, obj = ac.SIZES[1]
    images, pos = ac.morph_video(S, R, obj)
    mid = 12
    fr, bx = ac.anchor_of(pos, obj, mid)
    kw = dict(grid=S, radius=R, min_conf=0.5, update=128, update_conf=0.5, drift_conf=0.0, sampling=sampling)
    rows = pa.track_pixels(images, fr, bx, None, **kw)[0][0, 0]
    rfr = np.array([[ac.F - mid]], np.int32)
    rev = pa.track_pixels(images[::-1], rfr, bx, None, **kw)[0][0, 0]
    assert np.isfinite(rows).all() and bits_equal(rows, rev[::-1])
    # and it matters: a backward chain started from the forward chain's last template gives other rows
    fwd_only = pa.track_pixels(images[mid:], np.array([[1]], np.int32), bx, None, **kw)[0][0, 0]
    assert bits_equal(fwd_only, rows[mid:])
    fixed = px.track_pixels(images, fr, bx, None, grid=S, radius=R, min_conf=0.5, sampling=sampling)[0][0, 0]
    assert not bits_equal(fixed[:mid], rows[:mid])       # (the backward rows do depend on the update)


# e. the binding ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("vdet_track_pixels", "vdet_track_volume_pixels"))
def test_header_prototypes_and_symbol_rows(name):
    from vdetlib_amd import _lib
    sibling, proto = prototype(name + '_box'), prototype(name + '_adaptive')
    assert sibling[1] == 'const uint32_t *d_integral'
    k = [a.split()[-1] for a in sibling].index('scale_penalty') + 1
    assert proto == sibling[:1] + ['const void *d_planes', 'int box'] + sibling[2:k] + \
        ['int update', 'double update_conf', 'double drift_conf'] + sibling[k:]
    res, args = _lib.SYMBOLS[name + '_adaptive']
    assert res is ctypes.c_int and args == [ctype_of(a) for a in proto]


def test_null_context_refused():
    from vdetlib_amd import _lib
    L = _lib.load_library()
    z = None
    assert L.vdet_track_pixels_adaptive(z, z, 0, 1, 8, 8, z, z, z, 1, 1, 8, 2, 0.5, 0, 1, 0, 5, 0, 64, 0.8, 0.7, z, z, z) == _lib.VDET_EINVAL
    assert L.vdet_track_volume_pixels_adaptive(z, z, 0, 8, 8, z, z, 1, 1, 1, 0.3, 0.0, 1, 8, 2, 0.5, 0, 1, 0, 5, 0, 64, 0.8, 0.7,
                                               z, z, z) == _lib.VDET_EINVAL


def test_limits_table_row():
    head = header().split('#ifndef VDET_HIP_H')[0]
    m = re.search(r'\n \*   pixel tracker with template update(.*?)\n \*/', head, flags=re.S)
    assert m, "the limits table has no 'pixel tracker with template update' row"
    row = re.sub(r'\s*\n \*\s*', ' ', m.group(1))
    for part in ('vdet_track_pixels_adaptive', 'vdet_track_volume_pixels_adaptive', '0 <= update <= 256', 'box 0 or 1', 'finite',
                 'VDET_EINVAL'):
        assert part in row, part


def test_header_states_the_rule():
    text = re.sub(r'\s*\n \*\s*', ' ', header())
    for part in ('A = ((256 - a) * A + a * (P << 8) + 128) >> 8', 'Tm = (A + 128) >> 8', 'SAD0 = sum |Tm0 - P|',
                 'c0 = 1.0f - (float)SAD0 / (float)(255*S*S)', 'conf >= (float)update_conf and c0 >= (float)drift_conf',
                 'per slot AND direction', 'tests/pixtrack_adapt_spec.py'):
        assert part in text, part


SIGNATURES = {
    'track_pixels': ['images', 'anchor_frames', 'anchor_boxes', 'anchor_scores', 'grid', 'radius', 'min_conf', 'max_frames', 'step',
                     'sync', 'ctx'],
    'track_pixels_scaled': ['images', 'anchor_frames', 'anchor_boxes', 'anchor_scores', 'grid', 'radius', 'min_conf', 'max_frames',
                            'step', 'scales', 'scale_step', 'scale_penalty', 'sync', 'ctx'],
    'track_volume_pixels': ['images', 'boxes', 'scores', 'nms_thres', 'thres', 'max_tracks', 'grid', 'radius', 'min_conf',
                            'max_frames', 'step', 'sync', 'ctx'],
    'track_volume_pixels_scaled': ['images', 'boxes', 'scores', 'nms_thres', 'thres', 'max_tracks', 'grid', 'radius', 'min_conf',
                                   'max_frames', 'step', 'scales', 'scale_step', 'scale_penalty', 'sync', 'ctx'],
}


@pytest.mark.parametrize("name", sorted(SIGNATURES))
def test_python_surface(name):
    """the visible signature is the call's own; the three keywords are accepted (a host tensor is refused as a host tensor, not
    as an unknown keyword) and checked; the docstring states the rule and says that the defaults are untuned"""
    import torch
    from vdetlib_amd import ops
    fn = getattr(ops, name)
    assert list(inspect.signature(fn).parameters) == SIGNATURES[name]
    doc = re.sub(r'\s+', ' ', fn.__doc__)
    for part in ('update', 'update_conf', 'drift_conf', 'nobody has tuned'):
        assert part in doc, part
    assert 'A = ((256 - a) * A + a * (P << 8) + 128) >> 8' in re.sub(r'\s+', ' ', ops.track_pixels.__doc__)
    img = torch.zeros((2, 8, 8, 3), dtype=torch.uint8)
    if 'volume' in name:
        args = (img, torch.zeros((2, 3, 4)), torch.zeros((2, 3, 1)))
    else:
        args = (img, torch.ones((1, 1), dtype=torch.int32), torch.tensor([[[2., 2., 5., 5.]]]))
    for kw in (dict(), dict(update=0), dict(update=64), dict(update=64, update_conf=0.9, drift_conf=0.6), dict(update=256, sampling='box')):
        with pytest.raises(ValueError, match='GPU|cuda|device'):
            fn(*args, **kw)
    for kw in (dict(update=-1), dict(update=257), dict(update=64, update_conf=float('nan')), dict(update=64, drift_conf=float('inf')),
               dict(update=0, update_conf=float('-inf'))):
        with pytest.raises(ValueError, match='update|drift_conf'):
            fn(*args, **kw)
    with pytest.raises(TypeError):
        fn(*args, updates=3)


def test_update_settings_reader():
    from vdetlib_amd import ops
    assert ops._update_settings(0, 0.8, 0.7) == (0, 0.8, 0.7) and ops._update_settings(256.0, 1, 2) == (256, 1.0, 2.0)
    for bad in ((-1, 0.8, 0.7), (257, 0.8, 0.7), (64, float('nan'), 0.7), (64, 0.8, float('nan')), (64, float('inf'), 0.7),
                (64, 0.8, float('-inf'))):
        with pytest.raises(ValueError):
            ops._update_settings(*bad)
