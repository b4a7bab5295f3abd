"""-m gpu: ops.nms_tracks / ops.nms_tracks_batch (csrc/tracknms_kernels.hpp) against `expected` of test_nms_tracks_cpu.py
(the rows of every (class, frame) list in the header's order, then oracle.nms).  Every comparison is exact: tracks, score and
src by bit pattern with a NaN equal to a NaN, cnt and ntracks equal; the inputs are bit-identical after every call.

The generated cases (seed, F, B, C, T) are the CPU file's, whose input condition is checked there.  Their longest list has 105
candidates, so the chunk-edge lengths 63 / 64 / 65 come from a `top_still` cut of case 12's NMS keep lists, and 128 / 129 from
the same case with every box of a frame in its keep list (descending score, no suppression: B = 130 of them)."""
import functools

import numpy as np
import pytest

import synth
from listnms_harness import ListNms, dev, wide_lists
from test_nms_tracks_cpu import CASES, SRC_PAD, THRESH, _oracle, expected, list_rows, make_case, outputs_equal, same_bits, still_of

pytestmark = pytest.mark.gpu

H = ListNms('nms_tracks', expected, case_thresh=THRESH, op_kw=dict(thresh=THRESH), equal=outputs_equal)
host, run, check, check_case = H.host, H.run, H.check, H.check_case


def longest(case, top_still):
    C, _, F = case['tracks'].shape[:3]
    return max(len(list_rows(c, f, case['tracks'], case['ntracks'], case['score'], case['tboxes'], still_of(case), top_still)[0])
               for c in range(C) for f in range(F))


@functools.lru_cache(maxsize=None)
def unsuppressed(shape):
    """the case with EVERY box of a frame in its keep list, in descending score order (ties by descending index)"""
    case = dict(make_case(*shape))
    o = _oracle()
    F, B, C = case['scores'].shape
    ki = np.empty((F, C, B), np.int32)
    for f in range(F):
        for c in range(C):
            ki[f, c] = o.argsort_desc(case['scores'][f, :, c])
    case['keep_idx'], case['keep_cnt'] = ki, np.full((F, C), B, np.int32)
    return case


@pytest.mark.parametrize("shape", CASES)
def test_generated_cases(shape):
    got = check_case(make_case(*shape))
    src = got['src'][got['src'] != SRC_PAD]
    assert (src >= 0).any() and (src < 0).any() and got['tracks'].shape[1] == shape[2] + 2 * shape[4]


@pytest.mark.parametrize("n", [63, 64, 65, 128, 129])
def test_list_lengths_across_the_chunk_edge(n):
    case = make_case(*CASES[1]) if n < 100 else unsuppressed(CASES[1])
    top = next(t for t in range(0, 131) if longest(case, t) == n)
    got = check_case(case, top_still=top)
    assert got['cnt'].max() > 32


@pytest.mark.parametrize("variant", ["top_still_0", "no_still", "no_tubelets", "wide_lds", "wide_lds_682", "wide_lds_683"])
def test_source_variants(variant):
    case = make_case(*CASES[2])
    if variant == "top_still_0":
        got = check_case(case, top_still=0)
        assert (got['src'][got['src'] != SRC_PAD] < 0).all() and got['cnt'].max() > 0
        assert outputs_equal(got, run(case['tracks'], case['ntracks'], case['score'], case['tboxes'], None))
    elif variant == "no_still":
        got = check_case(case, still=False)
        assert got['tracks'].shape[1] == case['tracks'].shape[1]
    elif variant == "no_tubelets":
        seed, F, B, C, _ = CASES[2]
        got = check_case(make_case(seed, F, B, C, 0))
        assert (got['src'][got['src'] != SRC_PAD] >= 0).all() and np.array_equal(got['cnt'], make_case(seed, F, B, C, 0)['keep_cnt'].T)
    elif variant == "wide_lds":     # top_still + T = 766 candidates of LDS per wave: two waves per workgroup instead of four, nine lists
        check_case(case, top_still=700)
    else:           # the break itself: 4 x 682 x 24 bytes stay below 64 KiB (four waves), 4 x 683 x 24 do not (two)
        nmax = int(variant[-3:])
        tracks, nt, score, still = wide_lists(nmax)
        got = check(tracks, nt, score, None, still, top_still=nmax - 11)
        assert got['tracks'].shape[1] == nmax and (0 < got['cnt']).all() and (got['cnt'] < nmax).all()
        live = got['src'] != SRC_PAD
        assert all((got['src'][0, :, f][live[0, :, f]] < 0).any() for f in range(2))        # a tubelet row is kept


@pytest.mark.parametrize("F", [1, 64, 65])
def test_frame_counts_on_a_coherent_video(F):
    case = make_case(21, F, 24, 2, 3, synth.coherent_video)
    got = check_case(case)
    assert got['cnt'].min() > 0


@functools.lru_cache(maxsize=None)
def big_list():
    """ONE list of 1000 + 24 candidates: B = 1100 boxes, an arbitrary keep list of 1050 of them (descending score, nothing
    suppressed), 24 tubelet rows that are jittered copies of detection boxes"""
    rng = np.random.RandomState(5)
    B, T = 1100, 24
    boxes = synth.boxes_1(rng, B, degenerate=400)[None]
    scores = synth.tie_free_scores(rng, B)[None, :, None]
    pick = rng.permutation(B)[:1050]
    ki = pick[np.argsort(-scores[0, pick, 0], kind='stable')].astype(np.int32)[None, None]
    tracks = np.zeros((1, T, 1, 5), np.float32)
    tracks[0, :, 0, :4] = boxes[0, rng.permutation(B)[:T]] + rng.randint(-3, 4, (T, 4))
    tracks[0, :, 0, 4] = rng.rand(T)
    return tracks, np.array([T], np.int32), rng.rand(1, T, 1), (boxes, scores, ki, np.array([[1050]], np.int32))


def test_the_1024_candidate_limit():
    tracks, nt, score, still = big_list()
    want = expected(tracks, nt, score, None, still, top_still=1000)
    got = run(tracks, nt, score, None, still, top_still=1000)
    assert outputs_equal(got, want) and got['tracks'].shape[1] == 1024 and 100 < got['cnt'][0, 0] < 1024
    assert (got['src'][0, :got['cnt'][0, 0], 0] < 0).any()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("tboxes", [True, False])
def test_score_series_and_boxes(dtype, tboxes):
    case = make_case(*CASES[0])
    sc = case['score'].astype(dtype)
    got = check_case(case, tboxes=tboxes, score=sc)
    live = got['src'] < 0
    live &= got['src'] != SRC_PAD
    assert live.any() and got['score'].dtype == np.float64
    if dtype == np.float64:         # the f64 score comes back unrounded
        assert (got['score'][live] != got['tracks'][..., 4][live].astype(np.float64)).any()


def test_f64_scores_equal_in_f32_tie_and_resolve_by_index():
    A, Bx = [10, 10, 109, 109], [12, 12, 111, 111]
    tracks = np.zeros((1, 2, 1, 5), np.float32)
    tracks[0, :, 0, :4] = [A, Bx]
    nt = np.array([2], np.int32)
    for lo, hi in ((0, 1), (1, 0)):         # whichever slot holds the larger f64 score: slot 1 is first
        score = np.zeros((1, 2, 1))
        score[0, lo, 0], score[0, hi, 0] = 0.75, np.nextafter(0.75, 1.0)
        got = run(tracks, nt, score)
        assert outputs_equal(got, expected(tracks, nt, score))
        assert got['src'][0, :, 0].tolist() == [-2, SRC_PAD] and got['score'][0, 0, 0] == score[0, 1, 0] and got['cnt'][0, 0] == 1


def test_garbage_behind_the_counts_and_odd_coordinates():
    case = dict(make_case(*CASES[2]))
    rng = np.random.RandomState(3)
    F, B, C = case['scores'].shape
    ki, kc = case['keep_idx'].copy(), case['keep_cnt']
    behind = np.arange(ki.shape[2])[None, None, :] >= kc[:, :, None]
    ki[behind] = rng.randint(-2 ** 31, 2 ** 31 - 1, int(behind.sum()))           # never read: any index at all
    tracks, score, tboxes, nt = case['tracks'].copy(), case['score'].copy(), case['tboxes'].copy(), case['ntracks'] - np.array([7, 0, 66], np.int32)
    dead = np.arange(tracks.shape[1])[None, :] >= nt[:, None]
    assert dead.any() and behind.any()
    tracks[dead] = rng.rand(int(dead.sum()), F, 5) * 500
    tboxes[dead] = tracks[dead][..., :4]
    score[dead] = 2.0 + rng.rand(int(dead.sum()), F)                              # would be on top of every list
    boxes = case['boxes'].copy()
    b0, b1 = int(ki[0, 0, 0]), int(ki[1, 0, 1])                                   # kept boxes of two lists
    boxes[0, b0, 2] = np.nan
    boxes[1, b1, 2] = np.inf
    still = (boxes, case['scores'], ki, kc)
    want = expected(tracks, nt, score, tboxes, still)
    got = run(tracks, nt, score, tboxes, still)
    assert outputs_equal(got, want)
    assert np.isnan(got['tracks'][0, :, 0, 2][got['src'][0, :, 0] == b0]).all() and (got['src'][0, :, 0] == b0).sum() == 1
    assert (got['score'][~np.isnan(got['score'])] < 2.0).all()


def _zero_width_pair(nan_one):
    """two identical zero-width boxes with the two best scores of their list"""
    tracks = np.zeros((1, 3, 1, 5), np.float32)
    tracks[0, :, 0, :4] = [[50, 50, 49, 80], [50, 50, 49, 80], [200, 200, 260, 260]]
    score = np.array([[[0.9], [np.nan if nan_one else 0.8], [0.5]]])
    return tracks, np.array([3], np.int32), score


def test_zero_union_of_an_evaluated_pair():
    import torch
    from vdetlib_amd import _lib, ops
    tracks, nt, score = _zero_width_pair(False)
    with pytest.raises(ZeroDivisionError):
        expected(tracks, nt, score)
    with pytest.raises(ZeroDivisionError):
        run(tracks, nt, score)
    ctx = _lib.get_context(torch.cuda.current_device())
    ops.nms_tracks(dev(tracks), dev(nt), dev(score), sync=False)
    with pytest.raises(ZeroDivisionError):
        ctx.sync()
    ctx.sync()                                       # the status word was cleared with the report
    tracks, nt, score = _zero_width_pair(True)       # the NaN-scored one is no row: nothing is evaluated against it
    got = run(tracks, nt, score)
    assert outputs_equal(got, expected(tracks, nt, score)) and got['cnt'][0, 0] == 2
    # the same pair at the bottom of the list: 0.5 is kept (IoU 0 with both), then -1.0 is kept and tested against -2.0
    score[0, 0, 0], score[0, 1, 0] = -2.0, -1.0
    with pytest.raises(ZeroDivisionError):
        expected(tracks, nt, score)
    with pytest.raises(ZeroDivisionError):
        run(tracks, nt, score)


def test_capacity_below_the_survivor_count():
    import torch
    from vdetlib_amd import _lib, ops
    case = make_case(*CASES[0])
    C, T, F = case['tracks'].shape[:3]
    B = case['boxes'].shape[1]
    R = 45
    want = expected(case['tracks'], case['ntracks'], case['score'], case['tboxes'], still_of(case), R=R)
    assert want['cnt'].max() > R and want['cnt'].min() < R
    d = [dev(case[k]) for k in ('tracks', 'ntracks', 'score', 'tboxes', 'boxes', 'scores', 'keep_idx', 'keep_cnt')]
    with pytest.raises(ValueError, match="capacity"):
        ops.nms_tracks(d[0], d[1], d[2], tboxes=d[3], still=tuple(d[4:]), cap=R)
    # the C entry point on buffers with a guard pattern behind R rows
    ctx = _lib.get_context(torch.cuda.current_device())
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    N, G = C * R * F, 4096
    ot = torch.full((N * 5 + G,), 7.25, dtype=torch.float32).cuda()
    osc = torch.full((N + G,), 7.25, dtype=torch.float64).cuda()
    osrc = torch.full((N + G,), 12345, dtype=torch.int32).cuda()
    ocnt = torch.full((C * F + G,), 12345, dtype=torch.int32).cuda()
    ont = torch.full((C + G,), 12345, dtype=torch.int32).cuda()
    ctx.check(ctx.lib.vdet_nms_tracks(ctx.h, F, C, T, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), 1, d[3].data_ptr(),
                                      d[4].data_ptr(), d[5].data_ptr(), B, d[6].data_ptr(), d[7].data_ptr(), B, B, THRESH, R,
                                      ot.data_ptr(), osc.data_ptr(), osrc.data_ptr(), ocnt.data_ptr(), ont.data_ptr()))
    with pytest.raises(ValueError, match="capacity"):
        ctx.sync()
    torch.cuda.synchronize()
    got = dict(tracks=ot[:N * 5].view(C, R, F, 5), score=osc[:N].view(C, R, F), src=osrc[:N].view(C, R, F), cnt=ocnt[:C * F].view(C, F),
               ntracks=ont[:C])
    assert outputs_equal(host(got), want)
    assert (ot[N * 5:] == 7.25).all() and (osc[N:] == 7.25).all() and all((x[n:] == 12345).all() for x, n in ((osrc, N), (ocnt, C * F), (ont, C)))


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


def test_host_limits():
    import torch
    from vdetlib_amd import _lib, ops
    case = make_case(*CASES[2])
    d = {k: dev(case[k]) for k in ('tracks', 'ntracks', 'score', 'tboxes', 'boxes', 'scores', 'keep_idx', 'keep_cnt')}
    still = (d['boxes'], d['scores'], d['keep_idx'], d['keep_cnt'])
    ctx = _lib.get_context(torch.cuda.current_device())
    ctx.set_timing(2)
    try:
        ctx.last_timing()
        T = case['tracks'].shape[1]
        for kw in (dict(top_still=1025 - T), dict(cap=1025), dict(cap=0), dict(top_still=-1)):
            with pytest.raises(ValueError):
                ops.nms_tracks(d['tracks'], d['ntracks'], d['score'], tboxes=d['tboxes'], still=still, **kw)
        # the C entry point refuses the same on its own
        F, B, C = case['scores'].shape
        args = lambda top, R, Bc=B: (ctx.h, F, C, T, d['tracks'].data_ptr(), d['ntracks'].data_ptr(), d['score'].data_ptr(), 1, None,
                                     d['boxes'].data_ptr(), d['scores'].data_ptr(), Bc, d['keep_idx'].data_ptr(), d['keep_cnt'].data_ptr(),
                                     B, top, THRESH, R, 1, 1, 1, 1, 1)
        for a in (args(1025 - T, 1024), args(10, 1025), args(10, 0), args(10, 100, 32768), args(-1, 100)):
            with pytest.raises(ValueError):
                ctx.check(ctx.lib.vdet_nms_tracks(*a))
        off = np.array([0, 2, 2], np.int64)
        with pytest.raises(ValueError):
            ctx.check(ctx.lib.vdet_nms_tracks_batch(ctx.h, off.ctypes.data, 2, *args(10, 100)[2:]))
        assert sum(n for _, n in ctx.last_timing().values()) == 0, "a refused call launched something"
    finally:
        ctx.set_timing(0)


def test_async_gives_the_same_bits():
    import torch
    from vdetlib_amd import _lib, ops
    case = make_case(*CASES[1])
    d = [dev(case[k]) for k in ('tracks', 'ntracks', 'score', 'tboxes', 'boxes', 'scores', 'keep_idx', 'keep_cnt')]
    ctx = _lib.get_context(torch.cuda.current_device())
    res = ops.nms_tracks(d[0], d[1], d[2], tboxes=d[3], still=tuple(d[4:]), sync=False)
    ctx.sync()
    want = expected(case['tracks'], case['ntracks'], case['score'], case['tboxes'], still_of(case))
    assert outputs_equal(host(res), want)
    ki = case['keep_idx'].copy()
    ki[0, 0, 0] = -1
    ops.nms_tracks(d[0], d[1], d[2], tboxes=d[3], still=(d[4], d[5], dev(ki), d[7]), sync=False)
    with pytest.raises(ValueError, match="keep"):
        ctx.sync()
    # the dict form: merge_tracks' / interpolate_tracks' keys
    as_dict = dict(tracks=d[0], ntracks=d[1], series=(d[2].float().double(), d[2]), tboxes=d[3])
    assert outputs_equal(host(ops.nms_tracks(as_dict, score=1, still=tuple(d[4:]))), want)


BATCH_FRAMES = (1, 5, 7)
BC, BB, BT = 3, 48, 3


@functools.lru_cache(maxsize=None)
def batch_cases():
    return [make_case(31 + v, F, BB, BC, BT) for v, F in enumerate(BATCH_FRAMES)]


def pack_batch(cases):
    """per-video cases -> (a dict in video_batch's layout on the device, the frame-major still-image tensors)"""
    import torch
    off = np.concatenate([[0], np.cumsum([c['tracks'].shape[2] for c in cases])]).astype(np.int64)
    T = cases[0]['tracks'].shape[1]

    def flat(key, per):
        buf = torch.from_numpy(np.concatenate([np.ascontiguousarray(c[key]).reshape(-1) for c in cases])).cuda()
        return [buf[BC * T * per * int(off[v]): BC * T * per * int(off[v + 1])].view(*((BC, T, int(off[v + 1] - off[v])) + ((per,) if per > 1 else ())))
                for v in range(len(cases))]
    bo = dict(tracks=flat('tracks', 5), pooled=flat('score', 1), tboxes=flat('tboxes', 4),
              ntracks=dev(np.stack([c['ntracks'] for c in cases])), frame_off=off)
    still = tuple(dev(np.concatenate([c[k] for c in cases])) for k in ('boxes', 'scores', 'keep_idx', 'keep_cnt'))
    return bo, still


def test_batch_equals_single_video_calls():
    import torch
    from vdetlib_amd import _lib, ops
    cases = batch_cases()
    bo, still = pack_batch(cases)
    ctx = _lib.get_context(torch.cuda.current_device())
    ctx.set_timing(1)
    try:
        out = ops.nms_tracks_batch(bo, 'pooled', still=still, thresh=THRESH)
        assert sum(n for _, n in ctx.last_timing().values()) == 1        # ONE launch for the whole batch
    finally:
        ctx.set_timing(0)
    off, R = out['frame_off'], BB + 2 * BT
    assert np.array_equal(off, bo['frame_off']) and tuple(out['cnt'].shape) == (BC, int(off[-1])) and tuple(out['ntracks'].shape) == (3, BC)
    for k in ('tracks', 'score', 'src'):            # views of ONE allocation per field, video after video
        ops._batch_flat(out[k], 1)
        assert len({x.untyped_storage().data_ptr() for x in out[k]}) == 1
    for v, case in enumerate(cases):
        one = run(case['tracks'], case['ntracks'], case['score'], case['tboxes'], still_of(case))
        assert outputs_equal(one, expected(case['tracks'], case['ntracks'], case['score'], case['tboxes'], still_of(case)))
        got = dict(tracks=out['tracks'][v].cpu().numpy(), score=out['score'][v].cpu().numpy(), src=out['src'][v].cpu().numpy(),
                   cnt=out['cnt'][:, int(off[v]):int(off[v + 1])].cpu().numpy(), ntracks=out['ntracks'][v].cpu().numpy())
        assert got['tracks'].shape == (BC, R, BATCH_FRAMES[v], 5) and outputs_equal(got, one), v
    # without tboxes the track rows are the boxes; without the still-image source R = T
    few = ops.nms_tracks_batch(bo, 'pooled', thresh=THRESH, use_tboxes=False)
    for v, case in enumerate(cases):
        assert same_bits(few['tracks'][v].cpu().numpy(), run(case['tracks'], case['ntracks'], case['score'])['tracks']), v


def _host_dets(video, want):
    from vdetlib_amd import eval as vev
    return vev.detections_from_tracks(video, want['tracks'], want['ntracks'], want['score'])


def test_end_to_end_average_precision():
    """DetEvaluator.add_detections on the device result == eval.evaluate on the lists `expected` made: AP per class and mAP
    within the evaluator's stated 1e-12, identical tp sequences (test_eval_gpu._check) -- one video, then the batch."""
    from test_eval_gpu import _check
    from vdetlib_amd import eval as vev, ops
    cases = batch_cases()
    annots = [c['annot'] for c in cases]
    one = cases[2]
    d = [dev(one[k]) for k in ('tracks', 'ntracks', 'score', 'tboxes', 'boxes', 'scores', 'keep_idx', 'keep_cnt')]
    out = ops.nms_tracks(d[0], d[1], d[2], tboxes=d[3], still=tuple(d[4:]), thresh=THRESH)
    want = expected(one['tracks'], one['ntracks'], one['score'], one['tboxes'], still_of(one))
    ev = ops.DetEvaluator(vev.gt_table_from_annots(annots[2:]))
    assert ev.add_detections(annots[2]['video'], out) == int(want['cnt'].sum()) > 0
    aps, m = _check(ev, _host_dets(annots[2]['video'], want), annots[2:], 'voc')
    assert m > 0
    bo, still = pack_batch(cases)
    bout = ops.nms_tracks_batch(bo, 'pooled', still=still, thresh=THRESH)
    evb = ops.DetEvaluator(vev.gt_table_from_annots(annots))
    dets = []
    for c, a in zip(cases, annots):
        dets += _host_dets(a['video'], expected(c['tracks'], c['ntracks'], c['score'], c['tboxes'], still_of(c)))
    assert evb.add_detections([a['video'] for a in annots], bout) == len(dets)
    _check(evb, dets, annots, 'voc')
    # the duplicates of the doubled set are gone: add_tracks of the same tubelets adds more detections
    evt = ops.DetEvaluator(vev.gt_table_from_annots(annots[2:]))
    evt.add_tracks(annots[2]['video'], d[0], d[1], d[2], d[3])
    evn = ops.DetEvaluator(vev.gt_table_from_annots(annots[2:]))
    evn.add_detections(annots[2]['video'], ops.nms_tracks(d[0], d[1], d[2], tboxes=d[3], thresh=THRESH))
    assert 0 < evn.stream()[0].numel() < evt.stream()[0].numel()
