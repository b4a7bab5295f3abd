"""CPU-only: the numpy rule of multi-context suppression (tests/context_spec.py) against numbers worked by hand, the case list's
own aims, and the binding: prototypes, symbol rows, and the argument errors that are raised before a device is needed."""
import os
import re

import numpy as np
import pytest

import context_cases as cc
import context_spec as spec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
NAN, INF = np.nan, np.inf


def same_bits(a, b):
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# the hand-worked volume: F = 2, B = 3, C = 4; 22 candidates (two NaN)
HAND = np.array([[[0.9, 0.1, 0.2, NAN],
                  [0.3, 0.8, 0.1, 0.0],
                  [0.2, 0.1, 0.7, -INF]],
                 [[0.95, 0.2, 0.1, 0.1],
                  [0.1, 0.3, 0.2, 0.2],
                  [0.4, 0.85, 0.3, NAN]]], F32)


def test_hand_worked_volume():
    # descending: 0.95 (c0), 0.9 (c0), 0.85 (c1), 0.8 (c1), 0.7 (c2), ...
    t, n, hits, high = spec.context_classes(HAND, top=4)
    assert n == 22 and t == F32(0.8) and t.dtype == F32
    assert hits.tolist() == [2, 2, 0, 0] and hits.dtype == np.int32
    assert high.tolist() == [True, True, False, False]
    out = spec.suppress_context(HAND, high, penalty=0.5)
    p = F32(0.5)
    want = np.array([[[0.9, 0.1, F32(0.2) - p, NAN],
                      [0.3, 0.8, F32(0.1) - p, F32(0.0) - p],
                      [0.2, 0.1, F32(0.7) - p, -INF]],
                     [[0.95, 0.2, F32(0.1) - p, F32(0.1) - p],
                      [0.1, 0.3, F32(0.2) - p, F32(0.2) - p],
                      [0.4, 0.85, F32(0.3) - p, NAN]]], F32)
    assert same_bits(out, want)
    # the default ratio on 22 candidates: floor(0.0066) = 0 -> k = 1
    t, n, hits, high = spec.context_classes(HAND)
    assert t == F32(0.95) and hits.tolist() == [1, 0, 0, 0]
    # top = 5 reaches class 2
    assert spec.context_classes(HAND, top=5)[3].tolist() == [True, True, True, False]


def test_rank_roundings():
    assert 0.0003 * 10000 == 2.9999999999999996 and spec.rank(10000) == 2
    assert 0.0003 * 30000 == 9.0 and spec.rank(30000) == 9
    assert spec.rank(600000000) == 179999
    assert spec.rank(5) == 1 and spec.rank(0) == 0 and spec.rank(7, ratio=1.0) == 7
    assert spec.rank(7, top=3) == 3 and spec.rank(7, top=100) == 7


def test_ties_at_the_threshold_over_two_classes():
    s = np.array([[[0.5, 0.7, 0.1], [0.7, 0.2, 0.7], [0.9, 0.1, 0.1]]], F32)
    t, n, hits, high = spec.context_classes(s, top=2)         # 0.9, then three 0.7 tied at rank 2
    assert t == F32(0.7) and hits.tolist() == [2, 1, 1] and high.tolist() == [True, True, True]


def test_zero_signs():
    s = np.array([[[-0.0, -1.0], [0.0, -2.0]]], F32)
    t, n, hits, high = spec.context_classes(s, top=1)
    assert same_bits(t, F32(0.0)) and hits.tolist() == [2, 0]
    s = np.array([[[-0.0, -1.0], [-0.0, -2.0]]], F32)        # only -0.0: still returned as +0.0
    assert same_bits(spec.context_classes(s, top=2)[0], F32(0.0))


def test_video_of_nan_and_top_beyond_n():
    s = np.full((2, 2, 3), NAN, F32)
    t, n, hits, high = spec.context_classes(s, top=3)
    assert t == INF and n == 0 and not hits.any() and not high.any()
    out = spec.suppress_context(s, high)
    assert same_bits(out, s)
    s[1, 0] = [1.0, 2.0, 3.0]
    t, n, hits, high = spec.context_classes(s, top=50)
    assert t == F32(1.0) and n == 3 and hits.tolist() == [1, 1, 1]
    t, n, hits, high = spec.context_classes(s, top=1, frame_off=[0, 1, 2])
    assert t.tolist() == [INF, 3.0] and n.tolist() == [0, 3] and high.tolist() == [[False] * 3, [False, False, True]]
    assert n.dtype == np.int64 and t.dtype == F32 and high.dtype == bool


def test_min_hits():
    s = np.array([[[0.9, 0.8, 0.1], [0.7, 0.2, 0.1]]], F32)
    t, n, hits, high = spec.context_classes(s, top=3, min_hits=2)
    assert hits.tolist() == [2, 1, 0] and high.tolist() == [True, False, False]


def test_score_thresh_drops_padding():
    s = np.array([[[0.9, 0.1], [-INF, -INF], [0.5, -INF]]], F32)
    assert spec.context_classes(s, ratio=1.0)[1] == 6
    t, n, hits, high = spec.context_classes(s, ratio=1.0, score_thresh=-INF)
    assert n == 3 and t == F32(0.1) and hits.tolist() == [2, 1]
    assert spec.context_classes(s, ratio=1.0)[0] == -INF


def test_nan_payload_and_inf_through_suppression():
    s = np.array([[[1.0, -INF, 0.0, INF]]], F32)
    s.view(np.uint32)[0, 0, 2] = 0x7FC01234
    out = spec.suppress_context(s, np.zeros(4, bool), penalty=1e30)
    assert out.view(np.uint32)[0, 0, 2] == 0x7FC01234 and out[0, 0, 1] == -INF and out[0, 0, 3] == INF
    assert out[0, 0, 0] == F32(1.0) - F32(1e30)
    assert same_bits(spec.suppress_context(s, np.ones(4, bool)), s)
    assert same_bits(spec.suppress_context(s, np.zeros(4, bool), penalty=0.0), s)


@pytest.mark.parametrize("case", cc.cases(), ids=lambda c: c["name"])
def test_cases_stand_where_they_aim(case):
    t, n, hits, high = spec.context_classes(case["scores"], **case["kw"])
    ex = case.get("expect", {})
    if "thresh" in ex:
        assert same_bits(t, np.array(ex["thresh"], F32))
    if "n" in ex:
        assert n == ex["n"]
    if "k" in ex:
        assert spec.rank(n, case["kw"].get("ratio", 0.0003), case["kw"].get("top")) == ex["k"]
    if "hits_total" in ex:
        assert int(hits.sum()) == ex["hits_total"]
    if "seams" in case:
        assert cc.seams_ok(case)
    if case["name"].startswith("knife") and ex["k"] < ex["n"]:
        # the next lower value is the threshold's neighbour: one rank further the threshold moves by one float
        t2 = spec.context_classes(case["scores"], top=int(hits.sum()) + 1)[0]
        assert same_bits(t2, cc.down(t if t != 0 else F32(-0.0)))


def test_digit_boundary_cases_straddle_the_digits():
    def key(x):
        b = int(np.array(x, F32).view(np.uint32))
        return (~b & 0xFFFFFFFF) if b & 0x80000000 else b | 0x80000000
    for b in cc.DIGIT_BITS:
        for sign in ("pos", "neg"):
            t = cc.case("knife_digit%d_%s" % (b, sign))["expect"]["thresh"]
            assert key(t) & ((1 << b) - 1) == 0 and key(cc.down(t)) & ((1 << b) - 1) == (1 << b) - 1
            assert key(t) - key(cc.down(t)) == 1


def test_batch_cases_have_differing_high_sets():
    c = cc.case("batch_v3_high_sets_differ")
    high = spec.context_classes(c["scores"], **c["kw"])[3]
    assert len({tuple(h) for h in high.tolist()}) == 3 and all(0 < h.sum() < h.size for h in high)


# ---- the binding
def _prototype(name):
    src = open(os.path.join(ROOT, 'include', 'vdet_hip.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    m = re.search(r'\bint\s+%s\s*\(([^)]*)\)\s*;' % name, src)
    assert m, name
    return [a.strip() for a in m.group(1).split(',')]


def test_prototypes_and_symbol_rows():
    import ctypes
    from vdetlib_amd import _lib
    for name in ("vdet_context_classes", "vdet_suppress_context"):
        args = _prototype(name)
        res, row = _lib.SYMBOLS[name]
        assert res is ctypes.c_int and len(row) == len(args), name
        for a, t in zip(args, row):
            want = (ctypes.c_void_p if '*' in a else ctypes.c_int64 if a.startswith('int64_t') else
                    ctypes.c_double if a.startswith('double') else ctypes.c_int)
            assert t is want, (name, a)
    src = open(os.path.join(ROOT, 'include', 'vdet_hip.h')).read()
    assert 'VDET_CTX_RECORDS=0' in src


def test_argument_errors_need_no_device():
    import torch
    from vdetlib_amd import ops
    s = torch.zeros((2, 3, 4))
    high = torch.zeros(4, dtype=torch.bool)
    bad = [dict(ratio=0.0), dict(ratio=1.5), dict(ratio=float('nan')), dict(ratio=-0.1), dict(top=0), dict(top=-3),
           dict(min_hits=0), dict(frame_off=[0, 1]), dict(frame_off=[0, 2, 2]), dict(frame_off=[1, 2])]
    for kw in bad:
        with pytest.raises(ValueError):
            ops.context_classes(s, **kw)
    for t in (s.double(), s[0], s[:, :, :0], torch.zeros((0, 3, 4))):
        with pytest.raises(ValueError):
            ops.context_classes(t)
        with pytest.raises(ValueError):
            ops.suppress_context(t, high)
    with pytest.raises(ValueError, match="same GPU"):
        ops.context_classes(s)                   # right layout, wrong memory: there is no CPU path
    with pytest.raises(ValueError, match="same GPU"):
        ops.suppress_context(s, high)
    for p in (-1.0, float('nan'), float('inf'), 1e39, -1e-9):
        with pytest.raises(ValueError, match="penalty"):
            ops.suppress_context(s, high, penalty=p)
    for h in (high.int(), torch.zeros(5, dtype=torch.bool), torch.zeros((1, 4), dtype=torch.bool)):
        with pytest.raises(ValueError, match="high"):
            ops.suppress_context(s, h)
    with pytest.raises(ValueError, match="high"):
        ops.suppress_context(s, high, frame_off=[0, 1, 2])           # [V,C] wanted
    with pytest.raises(ValueError, match="out"):
        ops.suppress_context(s, high, out=torch.zeros((2, 3, 5)))
    with pytest.raises(ValueError, match="out"):
        ops.suppress_context(s, high, out=torch.zeros((2, 3, 4), dtype=torch.float64))
