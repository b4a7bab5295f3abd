"""The case list the numpy rule (rpn_spec.py) and the device (test_rpn_gpu.py) share: ``cases()`` returns dicts
(name, scores [F,A,Hf,Wf] f32, deltas [F,4A,Hf,Wf] f32, anchors [A,4] f64, im_size, kw: the remaining arguments), built once and
never written to; ``want(name)`` is the rule's result, computed once.  A case with ``cls`` gives its scores as the strided
foreground half ``cls[:, A:]`` of a contiguous [F,2A,Hf,Wf] array."""
import functools

import numpy as np

import rpn_spec

F32, F64 = np.float32, np.float64
NAN, INF = np.nan, np.inf

ANCHORS9 = rpn_spec.generate_anchors()
# fractional corners: no coordinate is an integer, one anchor is not even square-ish
ANCHORS4 = np.array([[-10.25, -7.5, 25.75, 22.125], [-30.5, -30.5, 45.5, 45.5], [1.125, -50.75, 14.875, 66.25], [-3.3, -3.3, 19.3, 19.3]], F64)
KNIFE_NAMES = ('exact', 'ulp_less', 'border_exact', 'border_ulp_less')


def random_case(seed, F, A, Hf, Wf, spread=0.2):
    """scores N(0,1), deltas N(0, spread): the shape of an RPN head's output"""
    rng = np.random.RandomState(seed)
    return rng.standard_normal((F, A, Hf, Wf)).astype(F32), (rng.standard_normal((F, 4 * A, Hf, Wf)) * spread).astype(F32)


def _case(name, scores, deltas, anchors, im_size, cls=None, **kw):
    return dict(name=name, scores=scores, deltas=deltas, anchors=anchors, im_size=im_size, cls=cls, kw=kw)


def knife_case():
    """One cell, four anchors, zero deltas: the decoded box of (x1,y1,x2,y2) is (x1, y1, x2 + 1, y2 + 1) exactly (width term 1.0,
    E(0) = 1), so with min_size = 16 on a 40 x 24 image (x clipped to 23):
      exact            (8,8,22,22)           -> (8,8,23,23): (23 - 8) + 1 = 16, a candidate
      ulp_less         x2 = 22 - 2^-19       -> X2 = 23 - 2^-19, the f32 below 23: 16 - 2^-19 < 16, none
      border_exact     (8,8,30,22)           -> X2 = 31 clipped to 23: 16, a candidate
      border_ulp_less  x1 = 8 + 2^-20        -> X1 the f32 above 8, X2 clipped to 23: 16 - 2^-20 < 16, none"""
    anchors = np.array([[8, 8, 22, 22], [8, 8, 22 - 2.0 ** -19, 22], [8, 8, 30, 22], [8 + 2.0 ** -20, 8, 30, 22]], F64)
    scores = np.array([0.4, 0.9, 0.3, 0.8], F32).reshape(1, 4, 1, 1)
    return _case('knife_edge', scores, np.zeros((1, 16, 1, 1), F32), anchors, (40, 24), pre_nms_top_n=4, post_nms_top_n=4,
                 min_size=16, nms_thresh=0.7)


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    small = dict(pre_nms_top_n=100, post_nms_top_n=20)
    s, d = random_case(1, 3, 9, 5, 7)
    out.append(_case('random_small', s, d, ANCHORS9, (80, 112), **small))
    s, d = random_case(2, 2, 3, 9, 67)                           # a row of 67 cells: a full tile of 64 lanes and a tail of 3
    out.append(_case('lane_tail', s, d, ANCHORS9[[0, 4, 8]], (144, 1072), pre_nms_top_n=500, post_nms_top_n=50))
    s, d = random_case(3, 1, 1, 1, 1)
    out.append(_case('one_anchor', s, d, ANCHORS9[3:4], (80, 112), pre_nms_top_n=1, post_nms_top_n=1))
    s, d = random_case(4, 2, 9, 48, 80)                          # N = 34 560 > 32 767
    out.append(_case('big_6000', s, d, ANCHORS9, (768, 1280), pre_nms_top_n=6000, post_nms_top_n=300))
    out.append(_case('big_16384', s, d, ANCHORS9, (768, 1280), pre_nms_top_n=16384, post_nms_top_n=300))
    s, d = random_case(5, 2, 20, 3, 70)                          # more anchors than one LDS tile of the decode pass holds
    rng = np.random.RandomState(55)
    c, hw = rng.uniform(0, 16, (20, 2)), rng.uniform(8, 90, (20, 2))
    out.append(_case('many_anchors', s, d, np.concatenate([c - hw, c + hw], 1).astype(F64), (48, 1120), pre_nms_top_n=700,
                     post_nms_top_n=100))

    # ---- ties
    rng = np.random.RandomState(6)
    s, d = random_case(6, 2, 9, 5, 7)
    out.append(_case('tie_quant4', (rng.randint(0, 4, s.shape) / 4.0).astype(F32), d, ANCHORS9, (80, 112), **small))
    out.append(_case('tie_all_equal', np.full(s.shape, 0.5, F32), d, ANCHORS9, (80, 112), **small))
    out.append(_case('tie_pm_zero', np.where(rng.randint(0, 2, s.shape) == 1, F32(0.0), F32(-0.0)).astype(F32), d, ANCHORS9, (80, 112),
                     **small))
    odd = np.array([NAN, INF, -INF, 0.0, -0.0, 1.0, -1.0], F32)
    out.append(_case('nan_inf_scores', np.where(rng.randint(0, 3, s.shape) == 0, odd[rng.randint(0, len(odd), s.shape)], s).astype(F32), d,
                     ANCHORS9, (80, 112), **small))

    # ---- edges
    s, d = random_case(7, 3, 9, 5, 7)
    few = np.full(s.shape, NAN, F32)
    flat = rng.permutation(s[0].size)
    few[0].reshape(-1)[flat[:5]] = s[0].reshape(-1)[flat[:5]]          # frame 0: 5 candidates at most, fewer than post
    few[1].reshape(-1)[flat[:50]] = s[1].reshape(-1)[flat[:50]]        # frame 1: fewer than pre
    few[2] = s[2]
    out.append(_case('few_candidates', few, d, ANCHORS9, (80, 112), **small))
    empty = s.copy()
    empty[1] = NAN                                                    # a frame with no candidate between two full ones
    out.append(_case('empty_frame', empty, d, ANCHORS9, (80, 112), **small))
    out.append(_case('pre_beyond_n', s, d, ANCHORS9, (80, 112), pre_nms_top_n=1000, post_nms_top_n=300))
    out.append(_case('min_size_filter', s, d, ANCHORS9, (80, 112), min_size=75.5, **small))
    out.append(knife_case())
    bad = d.copy()
    hit = rng.randint(0, 6, bad.shape) == 0
    bad[hit] = np.array([NAN, INF, -INF, 3e38, -3e38], F32)[rng.randint(0, 5, int(hit.sum()))]
    out.append(_case('nonfinite_deltas', s, bad, ANCHORS9, (80, 112), **small))
    # a dw / dh of 10 on small anchors in a large image: unclamped sides grow by e^10 and are cut by the border, clamped by 62.5
    sw, wide = random_case(10, 2, 6, 5, 7)
    wide = wide.copy()
    dwdh = wide.reshape(2, 6, 4, 5, 7)[:, :, 2:]
    dwdh[rng.randint(0, 4, dwdh.shape) == 0] = 10.0
    tiny = rpn_spec.generate_anchors(base_size=4, scales=(1, 2))
    out.append(_case('dw10_clamped', sw, wide, tiny, (2000, 3000), dw_max=float(np.log(1000.0 / 16.0)), min_size=2, **small))
    out.append(_case('dw10_free', sw, wide, tiny, (2000, 3000), min_size=2, **small))
    out.append(_case('offset_eps', s, d, ANCHORS9, (80, 112), offset=1e-14, **small))
    s4, d4 = random_case(8, 2, 4, 6, 5)
    out.append(_case('fractional_anchors', s4, d4, ANCHORS4, (70, 61), stride=13, min_size=4.5, nms_thresh=0.5, **small))
    cls = np.random.RandomState(9).standard_normal((3, 18, 5, 7)).astype(F32)
    out.append(_case('strided_scores', cls[:, 9:], d, ANCHORS9, (80, 112), cls=cls, **small))
    for c in out:
        for k in ('scores', 'deltas', 'anchors', 'cls'):
            if c[k] is not None:
                c[k].setflags(write=False)
    return tuple(out)


def names():
    return tuple(c['name'] for c in cases())


def case(name):
    return cases()[names().index(name)]


@functools.lru_cache(maxsize=None)
def want(name):
    c = case(name)
    out = rpn_spec.proposals(c['scores'], c['deltas'], c['anchors'], c['im_size'], **c['kw'])
    for v in out.values():
        v.setflags(write=False)
    return out
