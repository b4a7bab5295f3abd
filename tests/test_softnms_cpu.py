"""CPU-only: ops.soft_nms_tracks / ops.soft_nms_tracks_batch (Soft-NMS of the per-frame detection lists) -- the C-ABI symbols and
prototypes, the ops signatures and every ValueError that starts no device work; the properties of the Gaussian weight's
exponential g of tests/softnms_spec.py and its measured distance from np.exp; hand-made lists that pin each clause of the rule
(pins(), which test_softnms_gpu.py runs on the device); two cross-checks against existing code; and the input condition of the
GPU cases: every list is reordered by the decay, tied scores are emitted, and rows fall below a floor by decay alone."""
import inspect
import math
import os

import numpy as np
import pytest

import knife_spec as K
import softnms_spec as S
from test_nms_tracks_cpu import (CASES, SRC_PAD, _host_args, _oracle, _prototype, _still_with, list_rows, make_case, same_bits,
                                 still_of)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = os.path.join(ROOT, 'tests', 'golden', 'knife_pairs.npz')
F32 = np.float32
INF = math.inf
LINEAR_THRESH = 0.3             # the generated cases' threshold (the issue's counts were taken there)
G_REL = 6e-7                    # g against np.exp over [-1 / SIGMA_MIN, 0]: measured 5.75e-7 (every float32 of the range), one digit up


def gpu_cases():
    """the generated cases of the GPU file: test_nms_tracks_cpu.CASES and case 2 with every box in its keep list"""
    from test_nms_tracks_gpu import unsuppressed
    return [make_case(*s) for s in CASES] + [unsuppressed(CASES[1])]


def case_lists(case, **kw):
    C, _, F = case['tracks'].shape[:3]
    for c in range(C):
        for f in range(F):
            yield list_rows(c, f, case['tracks'], case['ntracks'], case['score'], case['tboxes'], still_of(case), **kw)


def case_median(case):
    """the median f32 score over the rows of every list of the case, as a python float"""
    return float(np.median(np.concatenate([d[:, 4] for d, _, _ in case_lists(case)])))


# ---- symbols, prototypes, signatures -------------------------------------------------------------------------------------
def test_symbols_and_prototypes():
    from vdetlib_amd import _lib
    hard = _prototype('vdet_nms_tracks')[2:]
    common = hard[:16] + ['int method', 'double sigma', 'double min_score'] + hard[16:] + ['double *d_score0_out']
    assert hard[15] == 'int R' and len(common) == 25
    assert _prototype('vdet_soft_nms_tracks') == ['vdet_ctx *ctx', 'int64_t F'] + common
    assert _prototype('vdet_soft_nms_tracks_batch') == ['vdet_ctx *ctx', 'const int64_t *h_frame_off', 'int64_t V'] + common
    assert len(_lib.SYMBOLS['vdet_soft_nms_tracks'][1]) == 2 + len(common)
    assert len(_lib.SYMBOLS['vdet_soft_nms_tracks_batch'][1]) == 3 + len(common)
    L = _lib.load_library()
    assert hasattr(L, 'vdet_soft_nms_tracks') and hasattr(L, 'vdet_soft_nms_tracks_batch')
    hdr = open(os.path.join(ROOT, 'include', 'vdet_hip.h')).read()
    assert 'Soft-NMS of the per-frame lists' in hdr and 'ovr > thresh' in hdr and 'score0' in hdr


def test_ops_signatures():
    from vdetlib_amd import ops
    p = inspect.signature(ops.soft_nms_tracks).parameters
    assert list(p) == ['tracks', 'ntracks', 'score', 'tboxes', 'still', 'method', 'thresh', 'sigma', 'min_score', 'top_still', 'cap',
                       'sync', 'ctx']
    assert {k: v.default for k, v in p.items() if k != 'tracks'} == \
        dict(ntracks=None, score=None, tboxes=None, still=None, top_still=None, cap=None, sync=True, ctx=None, **S.DEFAULTS)
    q = inspect.signature(ops.soft_nms_tracks_batch).parameters
    assert list(q) == ['batch_out', 'score', 'still', 'method', 'thresh', 'sigma', 'min_score', 'top_still', 'cap', 'use_tboxes',
                       'sync', 'ctx']
    assert {k: v.default for k, v in q.items() if k != 'batch_out'} == \
        dict(score='pooled', still=None, top_still=None, cap=None, use_tboxes=True, sync=True, ctx=None, **S.DEFAULTS)
    assert 'could not be checked' in ops.soft_nms_tracks.__doc__
    assert ops._SN_METHODS == S.METHODS and ops._SN_SIGMA_MIN == S.SIGMA_MIN


SOFT_BAD = [dict(method='hard'), dict(method=0), dict(method=None), dict(sigma=0.0), dict(sigma=-1.0), dict(sigma=math.nan),
            dict(sigma=INF), dict(sigma=1.0 / 128), dict(sigma='wide'), dict(thresh=math.nan), dict(min_score=math.nan),
            dict(min_score=None)]


def test_value_errors_start_no_device_work():
    """host tensors throughout: whatever passes the checks ends at the device check, a ValueError as well"""
    import torch
    from vdetlib_amd import ops
    a = _host_args()
    z = torch.zeros
    bad = [
        dict(tracks=z(2, 3, 4, 4)), dict(tracks=z(2, 3, 4, 5, dtype=torch.float64)), dict(tracks=z(2, 3, 0, 5), score=z(2, 3, 0)),
        dict(ntracks=z(2, dtype=torch.int64)), dict(ntracks=z(3, dtype=torch.int32)), dict(ntracks=None),
        dict(score=z(2, 3, 5)), dict(score=z(2, 3, 4, dtype=torch.float16)), dict(score=None), dict(score=1),
        dict(tboxes=z(2, 3, 4, 5)), dict(tboxes=z(2, 3, 4, 4, dtype=torch.float64)),
        dict(still=a['still'][:3]), dict(still=_still_with(a, 0, z(4, 5, 5))), dict(still=_still_with(a, 0, z(3, 5, 4))),
        dict(still=_still_with(a, 0, z(4, 5, 4, dtype=torch.float64))), dict(still=_still_with(a, 1, z(4, 2, 5))),
        dict(still=_still_with(a, 2, z(4, 2, 5, dtype=torch.int64))), dict(still=_still_with(a, 2, z(4, 3, 5, dtype=torch.int32))),
        dict(still=_still_with(a, 3, z(4, 3, dtype=torch.int32))), dict(still=_still_with(a, 3, z(4, 2, dtype=torch.int64))),
        dict(still=None, top_still=2), dict(top_still=-1), dict(top_still=1022), dict(cap=0), dict(cap=1025),
        dict(still=(z(4, 40000, 4), z(4, 40000, 2), a['still'][2], a['still'][3])),
    ] + SOFT_BAD + [
        {}, dict(method='gauss', sigma=S.SIGMA_MIN, min_score=-INF, thresh=INF),      # every check passes: host tensors
    ]
    for kw in bad:
        args = dict(a, **kw)
        with pytest.raises(ValueError) as e:
            ops.soft_nms_tracks(args.pop('tracks'), args.pop('ntracks'), args.pop('score'), **args)
        assert ('same GPU' in str(e.value)) == (kw in bad[-2:]), (kw.keys(), str(e.value))
    d = dict(tracks=a['tracks'], ntracks=a['ntracks'], series=(a['score'],), tboxes=a['tboxes'])
    for kw in (dict(ntracks=a['ntracks']), dict(score=1), dict(score='pooled'), {}):
        with pytest.raises(ValueError):
            ops.soft_nms_tracks(d, **kw)
    with pytest.raises(ValueError):
        ops.soft_nms_tracks(dict(tracks=a['tracks']))
    with pytest.raises(ValueError, match="2\\^31"):
        ops.soft_nms_tracks(torch.empty(3000, 0, 1000, 5, device='meta'), torch.empty(3000, dtype=torch.int32, device='meta'),
                            torch.empty(3000, 0, 1000, device='meta'), cap=1000)


def test_batch_value_errors_start_no_device_work():
    import torch
    from vdetlib_amd import ops
    C, T = 2, 3
    off = np.array([0, 2, 5], np.int64)

    def views(per, dtype):
        flat = torch.zeros(C * T * 5 * per, dtype=dtype)
        return [flat[C * T * per * int(off[v]): C * T * per * int(off[v + 1])].view(*((C, T, int(off[v + 1] - off[v])) + ((per,) if per > 1 else ())))
                for v in range(2)]
    bo = dict(tracks=views(5, torch.float32), pooled=views(1, torch.float64), det=views(1, torch.float32), tboxes=views(4, torch.float32),
              ntracks=torch.zeros(2, C, dtype=torch.int32), frame_off=off)
    still = (torch.zeros(5, 7, 4), torch.zeros(5, 7, C), torch.zeros(5, C, 7, dtype=torch.int32), torch.zeros(5, C, dtype=torch.int32))
    bad = [
        (dict(bo, frame_off=np.array([0, 2, 2])), {}), ({k: v for k, v in bo.items() if k != 'ntracks'}, {}), (bo, dict(score='nope')),
        (dict(bo, pooled=bo['pooled'][:1]), {}), (dict(bo, tboxes=bo['tracks']), {}), (bo, dict(still=(still[0][:4],) + still[1:])),
        (bo, dict(top_still=3)), (bo, dict(still=still, top_still=1022)), (bo, dict(cap=0)),
    ] + [(bo, kw) for kw in SOFT_BAD] + [
        (bo, {}), (bo, dict(score='det', still=still, method='gauss')),                # every check passes: host tensors
    ]
    for i, (b, kw) in enumerate(bad):
        with pytest.raises(ValueError) as e:
            ops.soft_nms_tracks_batch(b, **kw)
        assert ('same GPU' in str(e.value)) == (i >= len(bad) - 2), (i, str(e.value))


# ---- the Gaussian weight's exponential ------------------------------------------------------------------------------------
def _g_arguments():
    """a dense grid of [-1 / SIGMA_MIN, 0], runs of neighbouring float32 at every place where the range reduction's k changes
    and below -1e-3, -1, the cut, and the values beyond"""
    lo = F32(-1.0 / S.SIGMA_MIN)
    grid = np.linspace(0.0, float(lo), 2000001).astype(F32)
    edges = [F32(-(k + 0.5) * math.log(2.0)) for k in range(0, 126)] + [F32(-1e-3), F32(-1.0), S.G_CUT]
    runs = [(np.uint32(F32(e).view(np.uint32)) + np.arange(-2000, 2001, dtype=np.int64)).astype(np.uint32).view(F32) for e in edges]
    return lo, np.sort(np.concatenate([grid] + runs))[::-1]


def test_g_properties_and_distance_from_exp():
    lo, x = _g_arguments()
    y = S.g(x)
    assert y.dtype == F32 and S.g(F32(0.0)).view(np.uint32) == 0x3F800000 and S.g(F32(-0.0)).view(np.uint32) == 0x3F800000
    assert (y >= 0).all() and (y <= 1).all() and not np.isnan(y).any()
    assert (np.diff(y) <= 0).all(), "g increases somewhere as its argument falls"          # x is in descending order
    for far in (np.nextafter(S.G_CUT, F32(-INF)), F32(-104.0), F32(-1e30), F32(-INF)):
        assert S.g(far).view(np.uint32) == 0                                                # +0.0, not -0.0
    assert S.g(S.G_CUT) >= np.finfo(F32).tiny                                               # a normal float down to the cut
    m = x >= lo
    ref = np.exp(x[m].astype(np.float64))
    rel = np.abs(y[m].astype(np.float64) - ref) / ref
    print("g: largest relative distance from exp over [%g, 0]: %.4g at %r" % (lo, rel.max(), float(x[m][rel.argmax()])))
    assert rel.max() <= G_REL
    assert rel.max() > 2.0 ** -22, "the stated distance is no longer the 2^-20 grid's: state the new one"


# ---- hand-made lists --------------------------------------------------------------------------------------------------------
def one_list(still_rows=(), tub_rows=()):
    """C = F = 1: rows (box, score) -> dict(tracks, ntracks, score, still) with every still-image row in the keep list"""
    T = len(tub_rows)
    tracks = np.zeros((1, T, 1, 5), F32)
    score = np.zeros((1, T, 1))
    for t, (box, s) in enumerate(tub_rows):
        tracks[0, t, 0, :4], score[0, t, 0] = box, s
    still = None
    if still_rows:
        B = len(still_rows)
        still = (np.array([[b for b, _ in still_rows]], F32), np.array([[[s] for _, s in still_rows]], F32),
                 np.arange(B, dtype=np.int32)[None, None], np.array([[B]], np.int32))
    return dict(tracks=tracks, ntracks=np.array([T], np.int32), score=score, still=still)


A, A2, FAR, FAR2 = [10, 10, 109, 109], [10, 10, 109, 59], [300, 300, 399, 399], [600, 50, 699, 149]      # IoU(A, A2) = 0.5 exactly
NANBOX = [10, np.nan, 109, 109]                  # (a NaN x1 would make a tubelet row absent)


def pins():
    """name -> (list, settings, emitted src in order, emitted f32 scores in order)"""
    h = F32(0.5)
    gh = S.g(-(h * h) / F32(0.5))                    # the Gaussian weight at ovr = 0.5, sigma = 0.5
    return {
        # equal scores at selection time, one still-image row and one tubelet row: the tubelet row (the higher index) goes first
        'tie_still_tubelet': (one_list([(A, 0.75)], [(FAR, 0.75)]), dict(), [-1, 0], [0.75, 0.75]),
        # ... and a tie that only the decay makes: 0.8 * (1 - 0.5) == 0.4
        'tie_made_by_decay': (one_list([(FAR, 0.4)], [(A, 0.9), (A2, 0.8)]), dict(), [-1, -2, 0], [0.9, F32(0.8) * h, 0.4]),
        'minus_zero_first': (one_list((), [(A, 0.0), (FAR, -0.0)]), dict(min_score=-INF), [-2, -1], [-0.0, 0.0]),
        'plus_zero_first': (one_list((), [(A, -0.0), (FAR, 0.0)]), dict(min_score=-INF), [-2, -1], [0.0, -0.0]),
        'identical_box_default_floor': (one_list((), [(A, 0.9), (A, 0.8)]), dict(), [-1], [0.9]),
        'identical_box_no_floor': (one_list((), [(A, 0.9), (A, 0.8)]), dict(min_score=-INF), [-1, -2], [0.9, 0.0]),
        'identical_box_negative': (one_list((), [(A, 0.9), (A, -0.8)]), dict(min_score=-INF), [-1, -2], [0.9, -0.0]),
        'inf_times_zero': (one_list((), [(A, INF), (A, INF), (FAR, INF)]), dict(min_score=-INF), [-3, -2], [INF, INF]),
        # a negative score RISES when decayed: -0.8 -> -0.4 overtakes -0.5
        'negative_rises': (one_list((), [(A, 0.9), (A2, -0.8), (FAR, -0.5)]), dict(min_score=-INF), [-1, -2, -3], [0.9, F32(-0.8) * h, -0.5]),
        'negative_rises_gauss': (one_list((), [(A, 0.9), (A2, -0.8), (FAR, -0.5)]), dict(method='gauss', min_score=-INF),
                                 [-1, -2, -3], [0.9, F32(-0.8) * gh, -0.5]),
        'gauss_decays_below_thresh': (one_list((), [(A, 0.9), (A2, 0.8), (FAR, 0.5)]), dict(method='gauss', thresh=0.9),
                                      [-1, -3, -2], [0.9, F32(0.5) * S.g(F32(-0.0)), F32(0.8) * gh]),
        'linear_keeps_below_thresh': (one_list((), [(A, 0.9), (A2, 0.8), (FAR, 0.5)]), dict(thresh=0.51), [-1, -2, -3], [0.9, 0.8, 0.5]),
        'nan_coordinates': (one_list((), [(A, 0.9), (NANBOX, 0.8), (NANBOX, 0.7)]), dict(), [-1, -2, -3], [0.9, 0.8, 0.7]),
        'nan_coordinates_gauss': (one_list((), [(NANBOX, 0.9), (A, 0.8), (NANBOX, 0.7)]), dict(method='gauss'), [-1, -2, -3],
                                  [0.9, 0.8, 0.7]),
        'floor_on_input': (one_list([(A, 0.0005)], [(FAR, 0.5), (FAR2, F32(0.001))]), dict(), [-1, -2], [0.5, 0.001]),
    }


ZERO_UNION = one_list((), [([50, 50, 49, 80], 0.9), ([50, 50, 49, 80], 0.8), ([200, 200, 260, 260], 0.5)])


def run_spec(lst, **kw):
    return S.expected(lst['tracks'], lst['ntracks'], lst['score'], None, lst['still'], **kw)


@pytest.mark.parametrize("name", sorted(pins()))
def test_hand_made_lists(name):
    lst, kw, src, scores = pins()[name]
    out = run_spec(lst, **kw)
    n = len(src)
    assert out['cnt'].tolist() == [[n]] and out['ntracks'].tolist() == [n]
    assert out['src'][0, :n, 0].tolist() == src and (out['src'][0, n:, 0] == SRC_PAD).all()
    assert same_bits(out['tracks'][0, :n, 0, 4], np.array(scores, F32)), out['tracks'][0, :n, 0, 4]
    assert same_bits(out['score'][0, :n, 0], np.array(scores, F32).astype(np.float64))
    assert np.isnan(out['tracks'][0, n:]).all() and np.isnan(out['score'][0, n:]).all() and np.isnan(out['score0'][0, n:]).all()
    rows = list_rows(0, 0, lst['tracks'], lst['ntracks'], lst['score'], None, lst['still'])
    by_src = {int(s): (d, s64) for d, s64, s in zip(*rows)}
    for r, s in enumerate(src):                     # the box and the source's own score of the emitted row
        assert same_bits(out['tracks'][0, r, 0, :4], by_src[s][0][:4]) and same_bits(out['score0'][0, r, 0], by_src[s][1])


def test_score0_is_the_unrounded_source_score():
    lst = one_list((), [(A, 0.9), (FAR, np.nextafter(0.75, 1.0))])
    out = run_spec(lst)
    assert out['score0'][0, :, 0].tolist() == [0.9, np.nextafter(0.75, 1.0)]
    assert out['score'][0, :, 0].tolist() == [float(F32(0.9)), 0.75]


def test_zero_union_raises():
    with pytest.raises(ZeroDivisionError):
        run_spec(ZERO_UNION)
    with pytest.raises(ZeroDivisionError):
        run_spec(ZERO_UNION, method='gauss', min_score=-INF)
    lst = dict(ZERO_UNION, score=np.array([[[0.9], [np.nan], [0.5]]]))       # the NaN-scored one is no row: nothing is evaluated
    assert run_spec(lst)['cnt'].tolist() == [[2]]
    lst = dict(ZERO_UNION, score=np.array([[[0.9], [0.0005], [0.5]]]))       # ... nor against a row below the floor
    assert run_spec(lst)['cnt'].tolist() == [[2]]


def knife_lists(t):
    """the knife-edge pairs of threshold t as two-row lists, one per frame: box a (0.9) is emitted, box b (0.5) is the pair's j"""
    P = K.load_pairs(PAIRS)
    a = np.concatenate([P[(form, t)][0] for form in ('int', 'frac')])
    b = np.concatenate([P[(form, t)][1] for form in ('int', 'frac')])
    n = len(a)
    tracks = np.zeros((1, 2, n, 5), F32)
    tracks[0, 0, :, :4], tracks[0, 1, :, :4] = b, a
    score = np.zeros((1, 2, n))
    score[0, 0], score[0, 1] = 0.5, 0.9
    return tracks, np.array([2], np.int32), score


@pytest.mark.parametrize("t", K.THRESHOLDS)
def test_overlap_exactly_at_the_threshold(t):
    """a pair decays under 'linear' iff the reference's nms suppresses it at that threshold"""
    o = _oracle()
    tracks, nt, score = knife_lists(t)
    out = S.expected(tracks, nt, score, method='linear', thresh=t, min_score=-INF)
    assert (out['cnt'] == 2).all() and (out['src'][0, 0] == -2).all()
    decayed = out['tracks'][0, 1, :, 4] != F32(0.5)
    hard = np.array([len(o.nms(np.concatenate([tracks[0, ::-1, f, :4], [[0.9], [0.5]]], 1).astype(F32), t)) == 1
                     for f in range(tracks.shape[2])])
    assert np.array_equal(decayed, hard) and decayed.any() and not decayed.all()
    _, _, q = K.quotient(tracks[0, 1, :, :4], tracks[0, 0, :, :4])
    assert same_bits(out['tracks'][0, 1, :, 4], np.where(decayed, F32(0.5) * (F32(1.0) - q), F32(0.5)).astype(F32))


# ---- cross-checks against existing code ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(4))
def test_nothing_decays_is_the_hard_nms_order(k):
    """'linear' with thresh = 1.5 and no floor: every row, in exactly oracle.nms(dets, 1.5)'s order, scores unchanged"""
    o = _oracle()
    n = 0
    for dets, _, _ in case_lists(gpu_cases()[k]):
        order, s = S.soft_nms(dets, 'linear', 1.5, 0.5, -INF)
        assert order.tolist() == list(o.nms(dets, 1.5)) and same_bits(s, dets[order, 4]) and len(order) == len(dets)
        n += len(dets) > 1
    assert n > 0


def test_cap_cut_short_still_reports_the_full_count():
    case = make_case(*CASES[0])
    args = (case['tracks'], case['ntracks'], case['score'], case['tboxes'], still_of(case))
    full = S.expected(*args, thresh=LINEAR_THRESH)
    cut = S.expected(*args, thresh=LINEAR_THRESH, R=5)
    assert np.array_equal(cut['cnt'], full['cnt']) and full['cnt'].max() > 5 and cut['ntracks'].tolist() == np.minimum(full['ntracks'], 5).tolist()
    for k in ('tracks', 'score', 'score0', 'src'):
        assert cut[k].shape[1] == 5 and same_bits(cut[k], full[k][:, :5])


# ---- the input condition of the GPU cases -------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(4))
def test_generated_cases_keep_the_decay_busy(k):
    o = _oracle()
    lists = reordered = tied = by_decay = 0
    for dets, _, _ in case_lists(gpu_cases()[k]):
        if not len(dets):
            continue
        lists += 1
        order, s = S.soft_nms(dets, 'linear', LINEAR_THRESH, 0.5, -INF)              # (raises ZeroDivisionError: "no zero union")
        assert len(order) == len(dets)
        reordered += order.tolist() != list(o.nms(dets, 1.5))                        # the plain descending sort, ties by index
        tied += len(np.unique(s)) < len(s)
        med = float(np.median(dets[:, 4]))
        kept, _ = S.soft_nms(dets, 'linear', LINEAR_THRESH, 0.5, med)
        by_decay += int((dets[:, 4] >= F32(med)).sum()) - len(kept)
        S.soft_nms(dets, 'gauss', LINEAR_THRESH, 0.5, 0.001)
    print("case %d: %d lists, %d reordered, %d emit tied scores, %d rows removed by decay alone" % (k, lists, reordered, tied, by_decay))
    assert lists > 0 and reordered == lists and tied >= 1 and by_decay >= 1
