"""-m gpu: ops.vote_nms_tracks / ops.vote_nms_tracks_batch (csrc/votenms_kernels.hpp) against tests/votenms_spec.py.  Every
comparison is by bit pattern (tracks, score, src, box0 and votes with a NaN equal to a NaN; cnt and ntracks equal); the inputs
are bit-identical after every call.

The generated cases are test_votenms_cpu.gpu_cases(), whose input condition (boxes move, a list keeps more than 64 rows) is
checked in test_votenms_cpu.py; its hand-made lists (pins) and the knife-edge lists run here on the device."""
import functools
import math

import numpy as np
import pytest

import knife_spec as K
import votenms_spec as V
from listnms_harness import ListNms, guards_intact
from test_nms_tracks_cpu import CASES, SRC_PAD, expected as hard_expected, make_case, same_bits, still_of
from test_nms_tracks_gpu import batch_cases, dev, pack_batch, unsuppressed
from test_softnms_cpu import ZERO_UNION, knife_lists
from test_votenms_cpu import (CASE_THRESH, CASE_VOTE, KEYS, VOTE_BAD, case_args, case_spec, gpu_cases, moved_rows, outputs_equal,
                              pin_matches, pins)

pytestmark = pytest.mark.gpu

H = ListNms('vote_nms_tracks', V.expected, own=(('box0', 4, np.float32), ('votes', 1, np.int32)), case_thresh=CASE_THRESH,
            equal=outputs_equal)
host, run, want_of, check, check_case = H.host, H.run, H.want_of, H.check, H.check_case
c_buffers, sizes_of, video_of = H.c_buffers, H.sizes_of, H.video_of

F32 = np.float32
SETTINGS = ((0.3, 0.5), (0.5, 0.5), (0.5, 0.7), (1.5, 0.5), (0.3, 1.5))          # (thresh, vote_thresh)


# ---- generated cases ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("thresh,vote_thresh", SETTINGS)
@pytest.mark.parametrize("weights", V.WEIGHTS)
@pytest.mark.parametrize("k", range(6))
def test_generated_cases(k, weights, thresh, vote_thresh):
    want = case_spec(k, thresh, vote_thresh, weights)
    got = run(*case_args(gpu_cases()[k]), thresh=thresh, vote_thresh=vote_thresh, weights=weights)
    assert outputs_equal(got, want)
    live = got['src'] != SRC_PAD
    if vote_thresh > 1:         # nothing votes but the row itself: nms_tracks' result, bit for bit
        hard = hard_expected(*case_args(gpu_cases()[k]), thresh=thresh)
        assert all(same_bits(got[key], hard[key]) for key in ('tracks', 'score', 'src')) and np.array_equal(got['cnt'], hard['cnt'])
        assert not moved_rows(got).any() and (got['votes'][live] == 1).all()
    elif (thresh, vote_thresh) == (CASE_THRESH, CASE_VOTE):      # the input condition test_votenms_cpu.py states
        assert moved_rows(got).sum() >= 30
    if thresh > 1:             # every row is kept
        assert got['cnt'].sum() == sum(len(V.list_rows(c, f, *case_args(gpu_cases()[k]))[0]) for c in range(got['cnt'].shape[0])
                                       for f in range(got['cnt'].shape[1]))


@pytest.mark.parametrize("weights", V.WEIGHTS)
@pytest.mark.parametrize("variant", ["no_tboxes", "no_still", "top_still_0", "no_tubelets"])
def test_source_variants(variant, weights):
    seed, F, B, C, T = CASES[2]
    case = gpu_cases()[5]                     # unsuppressed(CASES[2]): the still-image rows vote too
    kw = dict(weights=weights, vote_thresh=CASE_VOTE)
    if variant == "no_tboxes":
        got = check_case(case, tboxes=False, **kw)
    elif variant == "no_still":
        got = check_case(case, still=False, **kw)
        assert got['tracks'].shape[1] == case['tracks'].shape[1]
    elif variant == "top_still_0":
        got = check_case(case, top_still=0, **kw)
        assert (got['src'][got['src'] != SRC_PAD] < 0).all()
    else:                                     # (the survivors of an NMS at 0.3 alone would have no voters at 0.5)
        got = check_case(unsuppressed((seed, F, B, C, 0)), **kw)
        assert (got['src'][got['src'] != SRC_PAD] >= 0).all()
    assert got['cnt'].max() > 0 and moved_rows(got).any()


@functools.lru_cache(maxsize=None)
def jittered_lists(n_still, T):
    """C = 1, F = 2: n_still still-image rows and T tubelet rows that are all jittered copies (+-8 px a coordinate) of ONE
    160 x 120 box, so that every row overlaps every other (IoU at least about 0.6, mostly above 0.8) -- tie-free scores, the
    still-image rows in descending score order as a keep list has them"""
    rng = np.random.RandomState(1000 * n_still + T)
    base = np.array([200, 150, 359, 269], F32)
    n = n_still + T
    still = None
    if n_still:
        boxes = (base + rng.randint(-8, 9, (2, n_still, 4))).astype(F32)
        scores = (0.05 + 0.9 * np.stack([np.sort(rng.permutation(4096)[:n_still])[::-1] for _ in range(2)]) / 4096.0).astype(F32)
        ki = np.tile(np.arange(n_still, dtype=np.int32), (2, 1, 1))
        still = (boxes, np.ascontiguousarray(scores[:, :, None]), ki, np.full((2, 1), n_still, np.int32))
    tracks = np.zeros((1, T, 2, 5), F32)
    tracks[0, :, :, :4] = base + rng.randint(-8, 9, (T, 2, 4))
    score = 0.05 + 0.9 * rng.rand(1, T, 2)
    return tracks, np.array([T], np.int32), score, still


@pytest.mark.parametrize("thresh", [0.9, 1.5])
@pytest.mark.parametrize("n_still,T", [(40, 23), (40, 24), (40, 25), (100, 29), (500, 11), (501, 11), (1012, 11), (1013, 11)])
def test_mutually_overlapping_rows(n_still, T, thresh):
    """63 / 64 / 65 / 129 rows (voters and, with thresh 1.5, kept rows on both sides of the 64-lane edge: the second rank pass
    runs) and 511 / 512 / 1 023 / 1 024 candidates (4, 2, 2 and 1 waves per workgroup).  At vote_thresh 0.85 a row has between a
    tenth and nine tenths of the list as its voters."""
    tracks, nt, score, still = jittered_lists(n_still, T)
    n = n_still + T
    for weights in V.WEIGHTS if n < 200 else (V.WEIGHTS[n % 2],):
        got = check(tracks, nt, score, None, still, thresh=thresh, vote_thresh=0.85, weights=weights)
        live = got['src'] != SRC_PAD
        assert got['tracks'].shape[1] == n and n // 10 < got['votes'][live].min() < got['votes'][live].max() < n
        assert moved_rows(got).sum() > 0.9 * live.sum()
        if thresh > 1:
            assert (got['cnt'] == n).all()
            # a symmetric neighbourhood count: row i counts row j iff row j counts row i, so the device's votes of a row are
            # also the number of rows that count IT
            for f in range(2):
                dets, _, src = V.list_rows(0, f, tracks, nt, score, None, still)
                nb = np.zeros((n, n), bool)
                for i in range(n):
                    nb[i, V.voters(dets, i, 0.85)] = True
                assert np.array_equal(nb, nb.T)
                counted_by = dict(zip(src.tolist(), nb.sum(0).tolist()))
                assert got['votes'][0, :, f].tolist() == [counted_by[s] for s in got['src'][0, :, f].tolist()]
        else:
            assert 8 < got['cnt'].max() < n


# ---- clause pins ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(pins()))
def test_hand_made_lists(name):
    lst, kw, want = pins()[name]
    if 'cap' in kw:             # fewer rows than the list keeps: ValueError at the wait (the rows: test_capacity_below_a_lists_count)
        with pytest.raises(ValueError, match="capacity"):
            run(lst['tracks'], lst['ntracks'], lst['score'], None, lst['still'], **kw)
        return
    got = check(lst['tracks'], lst['ntracks'], lst['score'], None, lst['still'], **kw)
    assert pin_matches(got, want)


@pytest.mark.parametrize("t", K.THRESHOLDS)
def test_overlap_exactly_at_the_vote_threshold(t):
    tracks, nt, score = knife_lists(t)
    for weights in V.WEIGHTS:
        got = check(tracks, nt, score, thresh=1.5, vote_thresh=t, weights=weights)
        two = got['votes'][0, 0] == 2
        assert two.any() and not two.all() and np.array_equal(two, got['votes'][0, 1] == 2)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("weights", V.WEIGHTS)
def test_score_series(dtype, weights):
    case = gpu_cases()[4]
    sc = case['score'].astype(dtype)
    got = check(case['tracks'], case['ntracks'], sc, case['tboxes'], still_of(case), thresh=CASE_THRESH, weights=weights)
    tub = (got['src'] < 0) & (got['src'] != SRC_PAD)
    assert tub.any() and got['score'].dtype == np.float64 and moved_rows(got).any()
    if dtype == np.float64:          # score comes back unrounded; the weight is its f32 rounding
        assert (got['score'][tub] != got['tracks'][..., 4][tub].astype(np.float64)).any()


# ---- error and status paths -------------------------------------------------------------------------------------------------
def c_tail(d, T, B, kcap, top, thresh, R, vote_thresh, weights, o, f64=1):
    p = lambda x: None if x is None else (x if isinstance(x, int) else x.data_ptr())
    return (T, p(d['tracks']), p(d['ntracks']), p(d['score']), f64, p(d.get('tboxes')), p(d.get('boxes')), p(d.get('scores')), B,
            p(d.get('keep_idx')), p(d.get('keep_cnt')), kcap, top, thresh, R, vote_thresh, weights, p(o['tracks']), p(o['score']),
            p(o['src']), p(o['cnt']), p(o['ntracks']), p(o['box0']), p(o['votes']))


def test_capacity_below_a_lists_count():
    import torch
    from vdetlib_amd import _lib, ops
    case = gpu_cases()[4]
    C, T, F = case['tracks'].shape[:3]
    B = case['boxes'].shape[1]
    R, G = 45, 4096
    want = want_of(*case_args(case), thresh=CASE_THRESH, cap=R)
    assert want['cnt'].max() > R and want['cnt'].min() < R
    d = {k: dev(case[k]) for k in ('tracks', 'ntracks', 'score', 'tboxes', 'boxes', 'scores', 'keep_idx', 'keep_cnt')}
    still = (d['boxes'], d['scores'], d['keep_idx'], d['keep_cnt'])
    with pytest.raises(ValueError, match="capacity"):
        ops.vote_nms_tracks(d['tracks'], d['ntracks'], d['score'], tboxes=d['tboxes'], still=still, thresh=CASE_THRESH, cap=R)
    # the C entry point on buffers with a guard pattern behind R rows, all seven outputs
    ctx = _lib.get_context(torch.cuda.current_device())
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    o = c_buffers(C, R, F, 1, G)
    ctx.check(ctx.lib.vdet_vote_nms_tracks(ctx.h, F, C, *c_tail(d, T, B, B, B, CASE_THRESH, R, CASE_VOTE, 0, o)))
    with pytest.raises(ValueError, match="capacity"):
        ctx.sync()
    torch.cuda.synchronize()
    N = C * R * F
    got = dict(tracks=o['tracks'][:N * 5].view(C, R, F, 5), score=o['score'][:N].view(C, R, F), src=o['src'][:N].view(C, R, F),
               cnt=o['cnt'][:C * F].view(C, F), ntracks=o['ntracks'][:C], box0=o['box0'][:N * 4].view(C, R, F, 4),
               votes=o['votes'][:N].view(C, R, F))
    assert outputs_equal(host(got), want)
    assert guards_intact(o, sizes_of(C, R, F, 1), G)


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
    out = ops.vote_nms_tracks(d[0], d[1], d[2], tboxes=d[3], still=tuple(d[4:]), thresh=CASE_THRESH, sync=False)
    with pytest.raises(ValueError, match="keep"):
        ctx.sync()
    sc = case['scores'].copy()
    sc[2, int(case['keep_idx'][2, 1, 0]), 1] = np.nan          # the skipped row as an absent one: same row indices
    kc2 = kc.copy()
    kc2[0, 0] = 0                                                 # a bad count: no still-image rows
    want = want_of(case['tracks'], case['ntracks'], case['score'], case['tboxes'], (case['boxes'], sc, case['keep_idx'], kc2),
                   thresh=CASE_THRESH)
    assert outputs_equal(host(out), want)


def test_zero_union_of_the_nms_raises_at_the_wait():
    import torch
    from vdetlib_amd import _lib, ops
    z = ZERO_UNION
    for kw in (dict(), dict(vote_thresh=1.5, weights='uniform')):
        with pytest.raises(ZeroDivisionError):
            run(z['tracks'], z['ntracks'], z['score'], **kw)
    ctx = _lib.get_context(torch.cuda.current_device())
    ops.vote_nms_tracks(dev(z['tracks']), dev(z['ntracks']), dev(z['score']), sync=False)
    with pytest.raises(ZeroDivisionError):
        ctx.sync()
    ctx.sync()                                       # the status word was cleared with the report
    got = check(z['tracks'], z['ntracks'], np.array([[[0.9], [np.nan], [0.5]]]))      # no row: nothing is evaluated against it
    assert got['cnt'][0, 0] == 2
    # ... and a zero union that only the voting pass meets raises nothing, with sync=False either
    lst = pins()['zero_union_met_by_the_voting_pass_only'][0]
    ops.vote_nms_tracks(dev(lst['tracks']), dev(lst['ntracks']), dev(lst['score']), sync=False)
    ctx.sync()


# ---- batch form -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weights", V.WEIGHTS)
def test_batch_equals_single_video_calls(weights):
    import torch
    from vdetlib_amd import _lib, ops
    cases = batch_cases()                            # ragged: 1, 5 and 7 frames
    bo, still = pack_batch(cases)
    kw = dict(thresh=CASE_THRESH, vote_thresh=CASE_VOTE, weights=weights)
    ctx = _lib.get_context(torch.cuda.current_device())
    ctx.set_timing(1)
    try:
        out = ops.vote_nms_tracks_batch(bo, 'pooled', still=still, **kw)
        assert sum(n for _, n in ctx.last_timing().values()) == 1        # ONE launch for the whole batch
    finally:
        ctx.set_timing(0)
    off = out['frame_off']
    assert np.array_equal(off, bo['frame_off']) and tuple(out['ntracks'].shape) == (len(cases), cases[0]['tracks'].shape[0])
    for k in KEYS:                                   # views of ONE allocation per field, video after video
        ops._batch_flat(out[k], 1)
        assert len({x.untyped_storage().data_ptr() for x in out[k]}) == 1
    singles = []
    for v, case in enumerate(cases):
        one = check(*case_args(case), **kw)
        assert outputs_equal(video_of(out, v, off), one), v
        singles.append(one)
    assert sum(int(moved_rows(s).sum()) for s in singles) > 0
    # sync=False on a side stream and a context of its own, then ctx.sync()
    cx = _lib.Context()
    try:
        side = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            late = ops.vote_nms_tracks_batch(bo, 'pooled', still=still, sync=False, ctx=cx, **kw)
            cx.sync()
        for v in range(len(cases)):
            assert outputs_equal(video_of(late, v, off), singles[v]), v
    finally:
        cx.close()
    # without tboxes the track rows are the boxes; without the still-image source R = T
    few = ops.vote_nms_tracks_batch(bo, 'pooled', use_tboxes=False, **kw)
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
    V_, Ft, R, G = len(cases), int(off[-1]), B + T, 4096
    ctx = _lib.get_context(torch.cuda.current_device())
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    o = c_buffers(C, R, Ft, V_, G)
    ctx.check(ctx.lib.vdet_vote_nms_tracks_batch(ctx.h, off.ctypes.data, V_, C, *c_tail(d, T, B, B, B, CASE_THRESH, R, CASE_VOTE, 1, o)))
    ctx.sync()
    assert guards_intact(o, sizes_of(C, R, Ft, V_), G)
    for v, case in enumerate(cases):
        f0, f1 = int(off[v]), int(off[v + 1])
        Fv = f1 - f0
        want = want_of(*case_args(case), thresh=CASE_THRESH, vote_thresh=CASE_VOTE, weights='uniform')
        cut = lambda key, per: o[key][C * R * f0 * per:C * R * f1 * per].view(*((C, R, Fv) + ((per,) if per > 1 else ())))
        got = dict(tracks=cut('tracks', 5), score=cut('score', 1), src=cut('src', 1), box0=cut('box0', 4), votes=cut('votes', 1),
                   cnt=o['cnt'][:C * Ft].view(C, Ft)[:, f0:f1], ntracks=o['ntracks'][v * C:(v + 1) * C])
        assert outputs_equal(host(got), want), v


def test_every_einval_launches_and_writes_nothing():
    import torch
    from vdetlib_amd import _lib, ops
    cases, bo, still, d, C, T, B = _batch_c_args()
    off = bo['frame_off']
    V_, Ft, R, G = len(cases), int(off[-1]), B + T, 16
    ctx = _lib.get_context(torch.cuda.current_device())
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    ctx.set_timing(2)
    try:
        ctx.last_timing()
        for kw in VOTE_BAD + [dict(top_still=1025 - T), dict(cap=1025), dict(cap=0), dict(top_still=-1)]:
            with pytest.raises(ValueError):
                ops.vote_nms_tracks_batch(bo, 'pooled', still=still, **kw)
        o = c_buffers(C, R, Ft, V_, G)
        ok = dict(d=d, T=T, B=B, kcap=B, top=B, thresh=0.3, R=R, vote_thresh=0.5, weights=0, o=o)
        bad = [dict(weights=2), dict(weights=-1), dict(vote_thresh=math.nan), dict(o=dict(o, box0=0)), dict(o=dict(o, votes=0)),
               dict(o=dict(o, cnt=0)), dict(top=1025 - T), dict(R=1025), dict(R=0), dict(top=-1), dict(B=32768), dict(kcap=0),
               dict(d=dict(d, boxes=0)), dict(d=dict(d, score=0))]
        for kw in bad:
            with pytest.raises(ValueError):
                ctx.check(ctx.lib.vdet_vote_nms_tracks_batch(ctx.h, off.ctypes.data, V_, C, *c_tail(**dict(ok, **kw))))
        with pytest.raises(ValueError):
            ctx.check(ctx.lib.vdet_vote_nms_tracks_batch(ctx.h, np.array([0, 2, 2, 13], np.int64).ctypes.data, V_, C, *c_tail(**ok)))
        with pytest.raises(ValueError):
            ctx.check(ctx.lib.vdet_vote_nms_tracks(ctx.h, 0, C, *c_tail(**ok)))
        assert sum(n for _, n in ctx.last_timing().values()) == 0, "a refused call launched something"
        torch.cuda.synchronize()
        assert all(bool((o[k] == (7.25 if o[k].dtype.is_floating_point else 12345)).all()) for k in o), "a refused call wrote something"
    finally:
        ctx.set_timing(0)


# ---- downstream -------------------------------------------------------------------------------------------------------------
def test_end_to_end_average_precision(capsys):
    """nms_volume -> vote_nms_tracks -> DetEvaluator(iou_thr 0.5 and 0.75).add_detections == eval.evaluate on the spec's lists (AP
    per class and mAP within the evaluator's stated 1e-12, identical tp sequences: test_eval_gpu._check).  The mAP is printed
    beside nms_tracks' on the same inputs; no gain is asserted.  seq_nms, soft_nms_tracks and the batch consumers take the result."""
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
    for weights in V.WEIGHTS:
        out = ops.vote_nms_tracks(d['tracks'], d['ntracks'], d['score'], tboxes=d['tboxes'], still=still, thresh=CASE_THRESH, weights=weights)
        want = want_of(*case_args(one), thresh=CASE_THRESH, weights=weights)
        assert outputs_equal(host(out), want)
        for iou_thr in (0.5, 0.75):
            ev = ops.DetEvaluator(vev.gt_table_from_annots(annots), iou_thr=iou_thr)
            assert ev.add_detections(video, out) == int(want['cnt'].sum()) > 0
            _, maps['%s@%.2f' % (weights, iou_thr)] = _check(
                ev, vev.detections_from_tracks(video, want['tracks'], want['ntracks'], want['score']), annots, 'voc', iou_thr=iou_thr)
    hard = ops.nms_tracks(d['tracks'], d['ntracks'], d['score'], tboxes=d['tboxes'], still=still, thresh=CASE_THRESH)
    for iou_thr in (0.5, 0.75):
        ev = ops.DetEvaluator(vev.gt_table_from_annots(annots), iou_thr=iou_thr)
        ev.add_detections(video, hard)
        maps['nms_tracks@%.2f' % iou_thr] = ev.compute()[1]
    with capsys.disabled():
        print("\nmAP on one synthetic video: " + ", ".join("%s %.4f" % kv for kv in sorted(maps.items())))
    # the other consumers take tracks / ntracks / score
    again = ops.nms_tracks(out['tracks'], out['ntracks'], out['score'], thresh=0.3)
    assert int(again['cnt'].sum()) > 0
    assert int(ops.seq_nms(out)['nseq'].sum()) > 0
    soft = ops.soft_nms_tracks(out['tracks'], out['ntracks'], out['score'])
    assert int(soft['cnt'].sum()) > 0
    # the batch dict goes on as it is; box0 and votes ride along
    cases = batch_cases()
    bo, bstill = pack_batch(cases)
    bout = ops.vote_nms_tracks_batch(bo, 'pooled', still=bstill, thresh=CASE_THRESH)
    evb = ops.DetEvaluator(vev.gt_table_from_annots([c['annot'] for c in cases]))
    assert evb.add_detections([c['annot']['video'] for c in cases], bout) == int(bout['cnt'].sum()) > 0
    assert int(ops.nms_tracks_batch(bout, 'score')['cnt'].sum()) > 0
    assert int(ops.soft_nms_tracks_batch(bout, 'score')['cnt'].sum()) > 0
    assert int(ops.seq_nms_batch(bout, 'score')['nseq'].sum()) > 0
