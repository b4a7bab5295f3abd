"""-m gpu: ops.soft_nms_tracks / ops.soft_nms_tracks_batch (csrc/softnms_kernels.hpp) against tests/softnms_spec.py.  Every
comparison is by bit pattern (tracks, score, score0 and src with a NaN equal to a NaN; cnt and ntracks equal); the inputs are
bit-identical after every call.

The generated cases are test_nms_tracks_cpu.CASES and case 2 with every box in its keep list; their input condition (every list
reordered by the decay, tied scores emitted, rows removed by decay alone) is checked in test_softnms_cpu.py, whose hand-made
lists (pins) and knife-edge lists run here on the device."""
import math

import numpy as np
import pytest

import knife_spec as K
import softnms_spec as S
from listnms_harness import ListNms, guards_intact, wide_lists
from test_nms_tracks_cpu import CASES, SRC_PAD, make_case, same_bits, still_of
from test_nms_tracks_gpu import batch_cases, dev, longest, pack_batch, unsuppressed
from test_softnms_cpu import LINEAR_THRESH, SOFT_BAD, ZERO_UNION, case_lists, case_median, gpu_cases, knife_lists, pins

pytestmark = pytest.mark.gpu

H = ListNms('soft_nms_tracks', S.expected, own=(('score0', 1, np.float64),), case_thresh=LINEAR_THRESH)
host, outputs_equal, run, want_of, check, check_case = H.host, H.outputs_equal, H.run, H.want_of, H.check, H.check_case
c_buffers, video_of = H.c_buffers, H.video_of

INF = math.inf
F32 = np.float32


def decayed(got):
    """the emitted rows whose score is no longer the f32 rounding of their source score"""
    live = ~np.isnan(got['score'])
    return live & (got['score'] != got['score0'].astype(F32).astype(np.float64))


# ---- generated cases ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("floor", ['none', 'default', 'median'])
@pytest.mark.parametrize("method", S.METHODS)
@pytest.mark.parametrize("k", range(4))
def test_generated_cases(k, method, floor):
    case = gpu_cases()[k]
    got = check_case(case, method=method, min_score={'none': -INF, 'default': 0.001, 'median': case_median(case)}[floor])
    src = got['src'][got['src'] != SRC_PAD]
    assert (src < 0).any() and decayed(got).any()
    if floor != 'median':            # (case 3's still-image scores all lie below its median)
        assert (src >= 0).any()
    if floor == 'none':
        assert got['cnt'].sum() == sum(len(r[0]) for r in case_lists(case))


@pytest.mark.parametrize("method", S.METHODS)
@pytest.mark.parametrize("variant", ["no_tboxes", "no_still", "top_still_0", "no_tubelets"])
def test_source_variants(variant, method):
    seed, F, B, C, T = CASES[2]
    case = make_case(*CASES[2])
    for floor in (-INF, 0.001, case_median(case)):
        kw = dict(method=method, min_score=floor)
        if variant == "no_tboxes":
            check_case(case, tboxes=False, **kw)
        elif variant == "no_still":
            got = check_case(case, still=False, **kw)
            assert got['tracks'].shape[1] == case['tracks'].shape[1] and got['cnt'].max() > 0
        elif variant == "top_still_0":
            got = check_case(case, top_still=0, **kw)
            assert (got['src'][got['src'] != SRC_PAD] < 0).all() and got['cnt'].max() > 0
        else:
            got = check_case(make_case(seed, F, B, C, 0), **kw)
            assert (got['src'][got['src'] != SRC_PAD] >= 0).all() and got['cnt'].max() > 0


@pytest.mark.parametrize("n", [63, 64, 65, 128, 129])
def test_list_lengths_across_the_chunk_edge(n):
    case = make_case(*CASES[1]) if n < 100 else unsuppressed(CASES[1])
    top = next(t for t in range(0, 131) if longest(case, t) == n)
    for method in S.METHODS:
        got = check_case(case, top_still=top, method=method, min_score=-INF)
        assert got['cnt'].max() == n


@pytest.mark.parametrize("nmax,method", [(511, 'linear'), (512, 'gauss'), (1023, 'linear'), (1024, 'gauss')])
def test_waves_per_workgroup(nmax, method):
    """32 bytes of LDS per candidate, the workgroup below 64 KiB: 4 waves up to 511 candidates, 2 up to 1023, 1 at 1024"""
    tracks, nt, score, still = wide_lists(nmax)
    got = check(tracks, nt, score, None, still, method=method, thresh=LINEAR_THRESH, min_score=-INF)
    assert got['tracks'].shape[1] == nmax and (got['cnt'] == nmax).all()
    assert decayed(got).sum() > 0.5 * got['cnt'].sum()                       # the decay is busy


# ---- clause pins ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(pins()))
def test_hand_made_lists(name):
    lst, kw, src, scores = pins()[name]
    got = check(lst['tracks'], lst['ntracks'], lst['score'], None, lst['still'], **kw)
    assert got['src'][0, :len(src), 0].tolist() == src and same_bits(got['tracks'][0, :len(src), 0, 4], np.array(scores, F32))


@pytest.mark.parametrize("t", K.THRESHOLDS)
def test_overlap_exactly_at_the_threshold(t):
    tracks, nt, score = knife_lists(t)
    got = check(tracks, nt, score, method='linear', thresh=t, min_score=-INF)
    dec = got['tracks'][0, 1, :, 4] != F32(0.5)
    assert dec.any() and not dec.all()
    check(tracks, nt, score, method='gauss', thresh=t, min_score=-INF)


# ---- error and status paths -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("method", S.METHODS)
def test_score_series(dtype, method):
    case = make_case(*CASES[0])
    sc = case['score'].astype(dtype)
    got = check(case['tracks'], case['ntracks'], sc, case['tboxes'], still_of(case), method=method, thresh=LINEAR_THRESH)
    tub = (got['src'] < 0) & (got['src'] != SRC_PAD)
    assert tub.any() and got['score'].dtype == np.float64 and got['score0'].dtype == np.float64
    assert same_bits(got['score'], got['tracks'][..., 4].astype(np.float64))
    if dtype == np.float64:          # score0 comes back unrounded
        assert (got['score0'][tub] != got['score0'][tub].astype(F32).astype(np.float64)).any()


def c_tail(d, T, B, kcap, top, thresh, R, method, sigma, floor, o, f64=1):
    p = lambda x: None if x is None else (x if isinstance(x, int) else x.data_ptr())
    return (T, p(d['tracks']), p(d['ntracks']), p(d['score']), f64, p(d.get('tboxes')), p(d.get('boxes')), p(d.get('scores')), B,
            p(d.get('keep_idx')), p(d.get('keep_cnt')), kcap, top, thresh, R, method, sigma, floor, p(o['tracks']), p(o['score']),
            p(o['src']), p(o['cnt']), p(o['ntracks']), p(o['score0']))


def test_capacity_below_a_lists_count():
    import torch
    from vdetlib_amd import _lib, ops
    case = make_case(*CASES[0])
    C, T, F = case['tracks'].shape[:3]
    B = case['boxes'].shape[1]
    R, G = 45, 4096
    want = want_of(case['tracks'], case['ntracks'], case['score'], case['tboxes'], still_of(case), thresh=LINEAR_THRESH, cap=R)
    assert want['cnt'].max() > R and want['cnt'].min() < R
    d = {k: dev(case[k]) for k in ('tracks', 'ntracks', 'score', 'tboxes', 'boxes', 'scores', 'keep_idx', 'keep_cnt')}
    still = (d['boxes'], d['scores'], d['keep_idx'], d['keep_cnt'])
    with pytest.raises(ValueError, match="capacity"):
        ops.soft_nms_tracks(d['tracks'], d['ntracks'], d['score'], tboxes=d['tboxes'], still=still, thresh=LINEAR_THRESH, cap=R)
    # the C entry point on buffers with a guard pattern behind R rows
    ctx = _lib.get_context(torch.cuda.current_device())
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    o = c_buffers(C, R, F, 1, G)
    ctx.check(ctx.lib.vdet_soft_nms_tracks(ctx.h, F, C, *c_tail(d, T, B, B, B, LINEAR_THRESH, R, 0, 0.5, 0.001, o)))
    with pytest.raises(ValueError, match="capacity"):
        ctx.sync()
    torch.cuda.synchronize()
    N = C * R * F
    got = dict(tracks=o['tracks'][:N * 5].view(C, R, F, 5), score=o['score'][:N].view(C, R, F), score0=o['score0'][:N].view(C, R, F),
               src=o['src'][:N].view(C, R, F), cnt=o['cnt'][:C * F].view(C, F), ntracks=o['ntracks'][:C])
    assert outputs_equal(host(got), want)
    assert guards_intact(o, dict(tracks=N * 5, score=N, score0=N, src=N, cnt=C * F, ntracks=C), G)


def test_keep_entries_out_of_range():
    case = dict(make_case(*CASES[0]))
    F, B, C = case['scores'].shape
    ki = case['keep_idx'].copy()
    ki[2, 1, 0] = B
    with pytest.raises(ValueError, match="keep"):
        run(case['tracks'], case['ntracks'], case['score'], case['tboxes'], (case['boxes'], case['scores'], ki, case['keep_cnt']))
    kc = case['keep_cnt'].copy()
    kc[0, 0] = B + 1
    with pytest.raises(ValueError, match="keep"):
        run(case['tracks'], case['ntracks'], case['score'], case['tboxes'], (case['boxes'], case['scores'], case['keep_idx'], kc))
    check_case(case)                                  # the status word was cleared with the report
    # the bad entries are skipped, everything else is the spec's: the same lists without them
    import torch
    from vdetlib_amd import _lib, ops
    ctx = _lib.get_context(torch.cuda.current_device())
    d = [dev(x) for x in (case['tracks'], case['ntracks'], case['score'], case['tboxes'], case['boxes'], case['scores'], ki, kc)]
    out = ops.soft_nms_tracks(d[0], d[1], d[2], tboxes=d[3], still=tuple(d[4:]), thresh=LINEAR_THRESH, sync=False)
    with pytest.raises(ValueError, match="keep"):
        ctx.sync()
    sc = case['scores'].copy()
    sc[2, int(case['keep_idx'][2, 1, 0]), 1] = np.nan          # the skipped row as an absent one: same row indices
    kc2 = kc.copy()
    kc2[0, 0] = 0                                                 # a bad count: no still-image rows
    want = want_of(case['tracks'], case['ntracks'], case['score'], case['tboxes'], (case['boxes'], sc, case['keep_idx'], kc2),
                   thresh=LINEAR_THRESH)
    assert outputs_equal(host(out), want)


def test_zero_union_raises_at_the_wait():
    import torch
    from vdetlib_amd import _lib, ops
    z = ZERO_UNION
    for kw in (dict(), dict(method='gauss', min_score=-INF)):
        with pytest.raises(ZeroDivisionError):
            run(z['tracks'], z['ntracks'], z['score'], **kw)
    ctx = _lib.get_context(torch.cuda.current_device())
    ops.soft_nms_tracks(dev(z['tracks']), dev(z['ntracks']), dev(z['score']), sync=False)
    with pytest.raises(ZeroDivisionError):
        ctx.sync()
    ctx.sync()                                       # the status word was cleared with the report
    for s1 in (np.nan, 0.0005):                      # no row / removed on input: nothing is evaluated against it
        got = check(z['tracks'], z['ntracks'], np.array([[[0.9], [s1], [0.5]]]))
        assert got['cnt'][0, 0] == 2


# ---- batch form -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", S.METHODS)
def test_batch_equals_single_video_calls(method):
    import torch
    from vdetlib_amd import _lib, ops
    cases = batch_cases()
    bo, still = pack_batch(cases)
    kw = dict(method=method, thresh=LINEAR_THRESH, min_score=0.02)
    ctx = _lib.get_context(torch.cuda.current_device())
    ctx.set_timing(1)
    try:
        out = ops.soft_nms_tracks_batch(bo, 'pooled', still=still, **kw)
        assert sum(n for _, n in ctx.last_timing().values()) == 1        # ONE launch for the whole batch
    finally:
        ctx.set_timing(0)
    off = out['frame_off']
    assert np.array_equal(off, bo['frame_off']) and tuple(out['ntracks'].shape) == (len(cases), cases[0]['tracks'].shape[0])
    for k in ('tracks', 'score', 'score0', 'src'):  # views of ONE allocation per field, video after video
        ops._batch_flat(out[k], 1)
        assert len({x.untyped_storage().data_ptr() for x in out[k]}) == 1
    singles = []
    for v, case in enumerate(cases):
        one = check(case['tracks'], case['ntracks'], case['score'], case['tboxes'], still_of(case), **kw)
        assert outputs_equal(video_of(out, v, off), one), v
        singles.append(one)
    # sync=False on a side stream and a context of its own, then ctx.sync()
    cx = _lib.Context()
    try:
        side = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            late = ops.soft_nms_tracks_batch(bo, 'pooled', still=still, sync=False, ctx=cx, **kw)
            cx.sync()
        for v in range(len(cases)):
            assert outputs_equal(video_of(late, v, off), singles[v]), v
    finally:
        cx.close()
    # without tboxes the track rows are the boxes; without the still-image source R = T
    few = ops.soft_nms_tracks_batch(bo, 'pooled', use_tboxes=False, **kw)
    for v, case in enumerate(cases):
        assert same_bits(few['tracks'][v].cpu().numpy(), want_of(case['tracks'], case['ntracks'], case['score'], **kw)['tracks']), v


def _batch_c_args():
    cases = batch_cases()
    bo, still = pack_batch(cases)
    C, T = cases[0]['tracks'].shape[:2]
    B = cases[0]['boxes'].shape[1]
    d = dict(tracks=bo['tracks'][0], ntracks=bo['ntracks'], score=bo['pooled'][0], tboxes=bo['tboxes'][0], boxes=still[0],
             scores=still[1], keep_idx=still[2], keep_cnt=still[3])
    return cases, bo, still, d, C, T, B


def test_batch_outputs_behind_a_guard_pattern():
    import torch
    from vdetlib_amd import _lib
    cases, bo, still, d, C, T, B = _batch_c_args()
    off = bo['frame_off']
    V, Ft, R, G = len(cases), int(off[-1]), B + T, 4096
    ctx = _lib.get_context(torch.cuda.current_device())
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    o = c_buffers(C, R, Ft, V, G)
    ctx.check(ctx.lib.vdet_soft_nms_tracks_batch(ctx.h, off.ctypes.data, V, C, *c_tail(d, T, B, B, B, LINEAR_THRESH, R, 1, 0.5, 0.02, o)))
    ctx.sync()
    N = C * R * Ft
    assert guards_intact(o, dict(tracks=N * 5, score=N, score0=N, src=N, cnt=C * Ft, ntracks=V * C), G)
    for v, case in enumerate(cases):
        f0, f1 = int(off[v]), int(off[v + 1])
        Fv = f1 - f0
        want = want_of(case['tracks'], case['ntracks'], case['score'], case['tboxes'], still_of(case), method='gauss',
                       thresh=LINEAR_THRESH, min_score=0.02)
        got = dict(tracks=o['tracks'][C * R * f0 * 5:C * R * f1 * 5].view(C, R, Fv, 5), score=o['score'][C * R * f0:C * R * f1].view(C, R, Fv),
                   score0=o['score0'][C * R * f0:C * R * f1].view(C, R, Fv), src=o['src'][C * R * f0:C * R * f1].view(C, R, Fv),
                   cnt=o['cnt'][:C * Ft].view(C, Ft)[:, f0:f1], ntracks=o['ntracks'][v * C:(v + 1) * C])
        assert outputs_equal(host(got), want), v


def test_every_einval_launches_and_writes_nothing():
    import torch
    from vdetlib_amd import _lib, ops
    cases, bo, still, d, C, T, B = _batch_c_args()
    off = bo['frame_off']
    V, Ft, R, G = len(cases), int(off[-1]), B + T, 16
    ctx = _lib.get_context(torch.cuda.current_device())
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    ctx.set_timing(2)
    try:
        ctx.last_timing()
        for kw in SOFT_BAD + [dict(top_still=1025 - T), dict(cap=1025), dict(cap=0), dict(top_still=-1)]:
            with pytest.raises(ValueError):
                ops.soft_nms_tracks_batch(bo, 'pooled', still=still, **kw)
        o = c_buffers(C, R, Ft, V, G)
        ok = dict(d=d, T=T, B=B, kcap=B, top=B, thresh=0.3, R=R, method=0, sigma=0.5, floor=0.001, o=o)
        bad = [dict(method=2), dict(method=-1), dict(sigma=0.0), dict(sigma=-0.5), dict(sigma=1.0 / 128), dict(sigma=INF),
               dict(sigma=math.nan), dict(thresh=math.nan), dict(floor=math.nan), dict(o=dict(o, score0=0)), dict(o=dict(o, cnt=0)),
               dict(top=1025 - T), dict(R=1025), dict(R=0), dict(top=-1), dict(B=32768), dict(kcap=0), dict(d=dict(d, boxes=0)),
               dict(d=dict(d, score=0))]
        for kw in bad:
            with pytest.raises(ValueError):
                ctx.check(ctx.lib.vdet_soft_nms_tracks_batch(ctx.h, off.ctypes.data, V, C, *c_tail(**dict(ok, **kw))))
        with pytest.raises(ValueError):
            ctx.check(ctx.lib.vdet_soft_nms_tracks_batch(ctx.h, np.array([0, 2, 2, 13], np.int64).ctypes.data, V, C, *c_tail(**ok)))
        with pytest.raises(ValueError):
            ctx.check(ctx.lib.vdet_soft_nms_tracks(ctx.h, 0, C, *c_tail(**ok)))
        assert sum(n for _, n in ctx.last_timing().values()) == 0, "a refused call launched something"
        torch.cuda.synchronize()
        assert all(bool((o[k] == (7.25 if o[k].dtype.is_floating_point else 12345)).all()) for k in o), "a refused call wrote something"
    finally:
        ctx.set_timing(0)


# ---- end to end -------------------------------------------------------------------------------------------------------------
def test_end_to_end_average_precision(capsys):
    """nms_volume -> soft_nms_tracks -> DetEvaluator.add_detections == eval.evaluate on the spec's lists (AP per class and mAP
    within the evaluator's stated 1e-12, identical tp sequences: test_eval_gpu._check).  The mAP is printed beside nms_tracks'
    on the same inputs; no gain is asserted."""
    from test_eval_gpu import _check
    from vdetlib_amd import eval as vev, ops
    one = batch_cases()[2]
    annots = [one['annot']]
    video = annots[0]['video']
    d = {k: dev(one[k]) for k in ('tracks', 'ntracks', 'score', 'tboxes', 'boxes', 'scores')}
    keep_idx, keep_cnt = ops.nms_volume(d['boxes'], d['scores'], 0.3)
    assert np.array_equal(keep_cnt.cpu().numpy(), one['keep_cnt']) and np.array_equal(keep_idx.cpu().numpy(), one['keep_idx'])
    still = (d['boxes'], d['scores'], keep_idx, keep_cnt)
    maps = {}
    for method in S.METHODS:
        out = ops.soft_nms_tracks(d['tracks'], d['ntracks'], d['score'], tboxes=d['tboxes'], still=still, method=method)
        want = want_of(one['tracks'], one['ntracks'], one['score'], one['tboxes'], still_of(one), method=method)
        assert outputs_equal(host(out), want)
        ev = ops.DetEvaluator(vev.gt_table_from_annots(annots))
        assert ev.add_detections(video, out) == int(want['cnt'].sum()) > 0
        _, maps[method] = _check(ev, vev.detections_from_tracks(video, want['tracks'], want['ntracks'], want['score']), annots, 'voc')
    ev = ops.DetEvaluator(vev.gt_table_from_annots(annots))
    ev.add_detections(video, ops.nms_tracks(d['tracks'], d['ntracks'], d['score'], tboxes=d['tboxes'], still=still, thresh=0.3))
    maps['nms_tracks(0.3)'] = ev.compute()[1]
    with capsys.disabled():
        print("\nmAP on one synthetic video: " + ", ".join("%s %.4f" % kv for kv in maps.items()))
    # the other consumers take tracks / ntracks / score
    again = ops.nms_tracks(out['tracks'], out['ntracks'], out['score'], thresh=0.3)
    assert int(again['cnt'].sum()) > 0
    sq = ops.seq_nms(out)
    assert int(sq['nseq'].sum()) > 0
