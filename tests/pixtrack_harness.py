"""What the pixel tracker family's test files share (test_pixel_track*_{cpu,gpu}.py, test_greedy_pixels_{cpu,gpu}.py): the
device calls against the one rule (tests/pixtrack_spec.py) ON BITS, the latched-anchor case, and the header readers of the CPU
files.  torch is imported where a function needs the GPU, never at import."""
import ctypes
import os
import re

import numpy as np
import pytest

import pixtrack_spec as px

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def g(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(out):
    return tuple(x.cpu().numpy() for x in out)


def bits_equal(got, want):
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    if got.dtype.kind != 'f':
        return np.array_equal(got, want)
    nan = np.isnan(want)
    u = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    return np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(u)[~nan], want.view(u)[~nan])


def assert_same(got, want):
    for k, name in enumerate(('tracks', 'anchors', 'ntracks')):
        assert bits_equal(got[k], want[k]), name


# ---- the slot-table form: ops.track_pixels without ``scales`` in the keywords, ops.track_pixels_scaled with ----------------------

def device(images, fr, bx, sc=None, **kw):
    from vdetlib_amd import ops
    fn = ops.track_pixels_scaled if 'scales' in kw else ops.track_pixels
    return host(fn(g(images), g(fr), g(bx), None if sc is None else g(sc), **kw))


def assert_spec(images, fr, bx, sc=None, **kw):
    """device == spec on bits, both with the same keywords (``sampling`` among them); returns the spec's outputs"""
    want = px.track_pixels(images, fr, bx, sc, **kw)
    assert not want[3]
    assert_same(device(images, fr, bx, sc, **kw), want)
    return want


# ---- the greedy form: ops.track_volume_pixels / ops.track_volume_pixels_scaled by the same choice ------------------------------

def greedy_device(images, boxes, scores, **kw):
    from vdetlib_amd import ops
    fn = ops.track_volume_pixels_scaled if 'scales' in kw else ops.track_volume_pixels
    return host(fn(g(images), g(boxes), g(scores), **kw))


def assert_greedy_spec(images, boxes, scores, ctx=None, **kw):
    """device == spec on bits; returns the spec's outputs"""
    want = px.track_volume_pixels(images, boxes, scores, **kw)
    assert not want[3]
    assert_same(greedy_device(images, boxes, scores, ctx=ctx, **kw), want)
    return want


# ---- invalid anchor data ---------------------------------------------------------------------------------------------------------
FI = 6
BAD_SLOTS = ((FI + 1, [10, 10, 30, 30]), (-1, [10, 10, 30, 30]), (2, [np.nan, 10, 30, 30]), (2, [10, 10, np.inf, 30]),
             (2, [10, 10, 9.5, 30]), (2, [10, 30, 30, 29]), (2, [70, 10, 90, 30]), (2, [10, -30, 30, 0.5]), (2, [10, 10, 2.0 ** 21, 30]))


def invalid_anchor_data_is_latched(call, k, seed, **kw):
    """BAD_SLOTS[k] between two good anchors on FI frames of noise from ``seed``, through ``call`` (the name of the ops call
    under test) with the settings ``kw``, which the spec takes too: the call raises, the slot is written as an empty one, its
    neighbours are what they are without it, the latch is cleared by the wait that reports it and the context works after it"""
    from vdetlib_amd import _lib, ops
    call = getattr(ops, call)
    frame, box = BAD_SLOTS[k]
    images = np.random.RandomState(seed).randint(0, 256, size=(FI, 48, 64, 3)).astype(np.uint8)
    ok = [20, 12, 43, 35]
    fr = np.array([[3, frame, 4]], np.int32)
    bx = np.array([[ok, box, ok]], np.float32)
    want = px.track_pixels(images, fr, bx, None, **kw)
    assert want[3] and np.isnan(want[0][0, 1]).all() and want[2].tolist() == [3]
    good = px.track_pixels(images, fr[:, ::2], bx[:, ::2], None, **kw)
    assert not good[3] and bits_equal(want[0][0, ::2], good[0][0])           # the neighbours are what they are without it
    ti, tf, tb = g(images), g(fr), g(bx)
    cx = _lib.Context()
    try:
        with pytest.raises(ValueError):
            call(ti, tf, tb, ctx=cx, **kw)
        out = call(ti, tf, tb, sync=False, ctx=cx, **kw)
        with pytest.raises(ValueError):
            cx.sync()
        assert_same(host(out), want)
        cx.sync()                                                             # the latch is cleared ...
        out = call(ti, g(fr[:, ::2]), g(bx[:, ::2]), ctx=cx, **kw)            # ... and the context works
        assert_same(host(out), good)
    finally:
        cx.close()


# ---- include/vdet_hip.h, for the CPU files ---------------------------------------------------------------------------------------

def header():
    return open(os.path.join(ROOT, 'include', 'vdet_hip.h')).read()


def prototype(name):
    src = re.sub(r'/\*.*?\*/', '', header(), flags=re.S)
    m = re.search(r'\bint\s+%s\s*\(([^;]*?)\)\s*;' % name, src, flags=re.S)
    assert m, "%s is not declared in include/vdet_hip.h" % name
    return [re.sub(r'\s+', ' ', a).strip() for a in m.group(1).split(',')]


def ctype_of(arg):
    if '*' in arg:
        return ctypes.c_void_p
    return {'int': ctypes.c_int, 'int64_t': ctypes.c_int64, 'double': ctypes.c_double, 'float': ctypes.c_float}[arg.split()[-2]]
