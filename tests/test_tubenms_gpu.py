"""-m gpu: ops.nms_tubelets / ops.nms_tubelets_batch (csrc/tubenms_kernels.hpp) against the numpy rule (tests/tubenms_spec.py).
Every output -- tracks, tboxes, anchors, each series, ntracks, src, tscore, by, overlaps -- is compared by bit pattern, a NaN
equal to a NaN; there is no tolerance and no case is excluded.  Every buffer the call allocates is filled with a poison byte
before the launches (``poisoned``), so an element the kernels do not write shows; the inputs are compared before and after.

Sizes (tubenms_cases): the pair pass stages CHUNK = 32 frames at a time and works on tiles of TILE = 32 slots, which is also the
width of a word of the bit rows.  T_SIZES covers one slot, one pair, the word / tile edge, two and three tiles per side and the
limit of 256; F_SIZES one and two frames, one below / at / above the chunk and more than three chunks."""
import contextlib
import functools

import numpy as np
import pytest

import tubenms_cases as cases
import tubenms_spec as spec
from test_tubenms_cpu import bits, same

pytestmark = pytest.mark.gpu

CHUNK, TILE = cases.CHUNK, cases.TILE
KEYS = ('tracks', 'ntracks', 'tboxes', 'anchors', 'src', 'tscore', 'by', 'overlaps')


def test_shapes_straddle_the_chunk_and_the_tile():
    """the sizes below still sit on both sides of the kernel's constants (read from its source)"""
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'vdetlib_amd', 'csrc', 'tubenms_kernels.hpp')).read()
    fc = int(re.search(r'kTubeFC = (\d+)', src).group(1))
    tile = int(re.search(r'kTubeTile = (\d+)', src).group(1))
    assert (fc, tile) == (CHUNK, TILE)
    assert {fc - 1, fc, fc + 1} <= set(cases.F_SIZES) and max(cases.F_SIZES) > 3 * fc and {1, 2} <= set(cases.F_SIZES)
    assert {tile - 1, tile, tile + 1, 2 * tile, 2 * tile + 1, 256, 1, 2} <= set(cases.T_SIZES)


@contextlib.contextmanager
def poisoned():
    """torch.empty hands out memory filled with 0xA5 bytes while the block runs: as f32 / f64 a finite negative number, as
    int32 -1515870811 -- nothing the rule can produce"""
    import torch
    real = torch.empty

    def empty(*a, **kw):
        t = real(*a, **kw)
        if t.numel():
            t.view(torch.uint8).fill_(0xA5)
        return t
    torch.empty = empty
    try:
        yield
    finally:
        torch.empty = real


def dev(x):
    import torch
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def host(out):
    r = {k: out[k].cpu().numpy() for k in KEYS if k in out and out[k] is not None}
    r['series'] = tuple(x.cpu().numpy() for x in out.get('series', ()))
    return r


def run(tracks, ntracks, score, tboxes=None, anchors=None, series=(), **kw):
    """ops.nms_tubelets on device copies, outputs poisoned first -> numpy; the inputs must come back bit-identical"""
    from vdetlib_amd import ops
    ins = [tracks, ntracks, score, tboxes, anchors] + list(series)
    d = [dev(x) for x in ins]
    with poisoned():
        out = ops.nms_tubelets(d[0], d[1], d[2], tboxes=d[3], anchors=d[4], series=tuple(d[5:]) or None, **kw)
    for x, y in zip(ins, d):
        assert x is None or same(x, y.cpu().numpy())
    return host(out)


def check(got, want, overlaps=True):
    keys = [k for k in KEYS if k in want and (overlaps or k != 'overlaps')]
    assert sorted(k for k in got if k != 'series') == sorted(keys)
    for k in keys:
        assert same(got[k], want[k]), k
    assert len(got['series']) == len(want['series'])
    for q, (x, y) in enumerate(zip(got['series'], want['series'])):
        assert same(x, y), ('series', q)


@functools.lru_cache(maxsize=None)
def want_of(seed, C, T, F, nser, tboxes, kind, dtype, norm, thresh, min_shared):
    s = cases.random_set(seed, C, T, F, nser, tboxes)
    score = (s['score2'] if kind == 'slot' else s['score3']).astype(dtype)
    return spec.expected(s['tracks'], s['ntracks'], score, s['tboxes'], s['anchors'], s['series'], thresh, norm,
                         'max' if kind == 'max' else 'mean', min_shared)


def run_random(seed, C, T, F, nser=2, tboxes=True, kind='mean', dtype=np.float64, norm='union', thresh=0.4, min_shared=1, **kw):
    s = cases.random_set(seed, C, T, F, nser, tboxes)
    score = (s['score2'] if kind == 'slot' else s['score3']).astype(dtype)
    got = run(s['tracks'], s['ntracks'], score, s['tboxes'], s['anchors'], s['series'], thresh=thresh, norm=norm,
              reduce='max' if kind == 'max' else 'mean', min_shared=min_shared, **kw)
    return got, want_of(seed, C, T, F, nser, tboxes, kind, np.dtype(dtype).type, norm, thresh, min_shared)


@pytest.mark.parametrize("F", [1, 2])
@pytest.mark.parametrize("T", cases.T_SIZES)
def test_slot_counts(T, F):
    """every T with one and two frames; four classes: ntracks = T, above T (clamped), below the live slots (garbage behind the
    count), 0.  The settings rotate with T so that every norm and every score kind meets a tile edge."""
    i = cases.T_SIZES.index(T)
    kind, norm = ('mean', 'slot', 'max')[(i + F) % 3], spec.NORMS[i % 3]
    got, want = run_random(300 + T, 4, T, F, nser=1 + i % 2, tboxes=bool((i + F) % 2), kind=kind, norm=norm, return_overlaps=True)
    check(got, want)
    assert want['ntracks'][3] == 0 and (want['by'][3] == -1).all() and np.isnan(want['overlaps'][3]).all()
    if T >= 31:
        assert (want['ntracks'][:3] < np.clip([T, T + 3, T // 2], 0, T)).all() and (want['ntracks'][:3] > 0).all()


@pytest.mark.parametrize("T", [5, 33])
@pytest.mark.parametrize("F", cases.F_SIZES[2:])
def test_frame_chunks(F, T):
    """F one below, at and one above the chunk of 32 frames and over more than three chunks, within one tile and across tiles"""
    got, want = run_random(400 + F, 3, T, F, kind=('mean', 'max')[F % 2], dtype=np.float32, return_overlaps=True)
    check(got, want)
    assert (want['ntracks'][:3] > 0).all()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("kind", ["mean", "max", "slot"])
@pytest.mark.parametrize("norm", spec.NORMS)
def test_norms_reduces_and_score_types(norm, kind, dtype):
    got, want = run_random(500, 4, 33, CHUNK + 1, kind=kind, dtype=dtype, norm=norm, thresh=0.3, min_shared=2, return_overlaps=True)
    check(got, want)


@pytest.mark.parametrize("nser", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("tboxes", [False, True])
def test_series_and_tboxes(nser, tboxes):
    """0..4 series, tboxes on and off; return_overlaps off gives the same other outputs"""
    got, want = run_random(600, 4, 9, CHUNK + 1, nser=nser, tboxes=tboxes)
    check(got, want, overlaps=False)
    assert ('tboxes' in got) == tboxes and len(got['series']) == nser
    if nser == 2:
        again, _ = run_random(600, 4, 9, CHUNK + 1, nser=nser, tboxes=tboxes, return_overlaps=True)
        check(again, want)


def test_exotic_boxes():
    """NaN, inf, inverted and zero-size boxes, coordinates up to 65535 and fractional: no contribution, no error"""
    tracks, ntracks, score = cases.exotic_set()
    for norm in spec.NORMS:
        check(run(tracks, ntracks, score, thresh=0.3, norm=norm, return_overlaps=True), spec.expected(tracks, ntracks, score, thresh=0.3, norm=norm))
    tb = np.ascontiguousarray(tracks[..., :4][:, ::-1])            # the odd boxes as tboxes of other slots: existence stays with column 0
    check(run(tracks, ntracks, score, tboxes=tb, thresh=0.3, return_overlaps=True), spec.expected(tracks, ntracks, score, tboxes=tb, thresh=0.3))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_score_edges(dtype):
    """NaN, +/-0.0, tied and infinite tubelet scores, per slot and through both reductions"""
    tracks, ntracks, score = cases.score_edge_set()
    score = score.astype(dtype)
    for thresh in (0.5, 1.5):
        check(run(tracks, ntracks, score, thresh=thresh, return_overlaps=True), spec.expected(tracks, ntracks, score, thresh=thresh))
    s3 = np.repeat(score[:, :, None], 2, axis=2)
    s3[0, 0] = [-0.0, 0.0]                                          # max: +0.0 whatever the order; mean: -0.0 + 0.0
    s3[0, 1] = [0.0, -0.0]
    s3[0, 7] = [np.nan, -0.0]
    for reduce in spec.REDUCES:
        want = spec.expected(tracks, ntracks, s3, thresh=1.5, reduce=reduce)
        check(run(tracks, ntracks, s3, thresh=1.5, reduce=reduce, return_overlaps=True), want)
        assert want['ntracks'][0] == 9


def test_knife_edges():
    tracks, ntracks, score = cases.knife_pair()
    for thresh, n in ((0.5, 1), (float(np.nextafter(0.5, 1.0)), 2)):
        got = run(tracks, ntracks, score, thresh=thresh, return_overlaps=True)
        check(got, spec.expected(tracks, ntracks, score, thresh=thresh))
        assert got['ntracks'][0] == n and got['overlaps'][0, 0, 1] == 0.5
    tracks, ntracks, score = cases.contained_pair()
    for norm, ms, n in (('union', 1, 2), ('min', 1, 1), ('shared', 2, 1), ('shared', 3, 2)):
        got = run(tracks, ntracks, score, thresh=0.5, norm=norm, min_shared=ms, return_overlaps=True)
        check(got, spec.expected(tracks, ntracks, score, thresh=0.5, norm=norm, min_shared=ms))
        assert got['ntracks'][0] == n


def test_thresh_above_one_and_planted():
    got, want = run_random(700, 4, 65, 3, thresh=1.0000001, return_overlaps=True)
    check(got, want)
    ts = spec.tubelet_scores(cases.random_set(700, 4, 65, 3)['tracks'], cases.random_set(700, 4, 65, 3)['ntracks'],
                             cases.random_set(700, 4, 65, 3)['score3'])
    for c in range(4):
        assert got['src'][c, :got['ntracks'][c]].tolist() == spec.order_of(ts[c])
    tracks, ntracks, score, owner = cases.planted_set()
    got = run(tracks, ntracks, score, thresh=0.3, return_overlaps=True)
    check(got, spec.expected(tracks, ntracks, score, thresh=0.3))
    assert got['ntracks'][0] == owner.max() + 1 + (owner < 0).sum()


def test_dict_input_async_and_explicit_context():
    import torch
    from vdetlib_amd import _lib, ops
    s = cases.random_set(800, 4, 33, CHUNK + 1)
    want = want_of(800, 4, 33, CHUNK + 1, 2, True, 'mean', np.float64, 'union', 0.4, 1)
    d = dict(tracks=dev(s['tracks']), ntracks=dev(s['ntracks']), anchors=dev(s['anchors']), tboxes=dev(s['tboxes']),
             series=tuple(dev(x) for x in s['series']))
    with poisoned():
        out = ops.nms_tubelets(d, score=dev(s['score3']), thresh=0.4, return_overlaps=True, sync=False)
    _lib.get_context(torch.cuda.current_device()).sync()
    check(host(out), want)
    # the score named by index: series 1 of the dict
    by_index = host(ops.nms_tubelets(d, score=1, thresh=0.4, return_overlaps=True))
    check(by_index, spec.expected(s['tracks'], s['ntracks'], s['series'][1], s['tboxes'], s['anchors'], s['series'], thresh=0.4))
    cx = _lib.Context()
    try:
        check(host(ops.nms_tubelets(d, score=dev(s['score3']), thresh=0.4, return_overlaps=True, ctx=cx)), want)
    finally:
        cx.close()


FRAMES = (1, CHUNK - 2, CHUNK + 1, CHUNK, 2 * CHUNK + 6)       # a 1-frame video; borders at 1, 31, 64, 96: behind, before and on a chunk seam


def _pack(sets, off, C, T):
    """per-video sets -> a dict in video_batch's layout on the device"""
    import torch

    def flat(get, per, dtype):
        buf = torch.from_numpy(np.concatenate([np.ascontiguousarray(get(s)).reshape(-1) for s in sets]).astype(dtype)).cuda()
        return [buf[C * T * per * int(off[v]): C * T * per * int(off[v + 1])].view(*((C, T, int(off[v + 1] - off[v])) + ((per,) if per > 1 else ())))
                for v in range(len(sets))]
    return dict(tracks=flat(lambda s: s['tracks'], 5, np.float32), det=flat(lambda s: s['series'][0], 1, np.float64),
                pooled=flat(lambda s: s['series'][1], 1, np.float64), tboxes=flat(lambda s: s['tboxes'], 4, np.float32),
                score32=flat(lambda s: s['score3'], 1, np.float32),
                anchors=torch.from_numpy(np.stack([s['anchors'] for s in sets])).cuda(),
                ntracks=torch.from_numpy(np.stack([s['ntracks'] for s in sets])).cuda(), frame_off=np.asarray(off, np.int64))


def test_batch_equals_single_video_calls():
    import torch
    from vdetlib_amd import _lib, ops
    C, T = 4, 33
    off = np.concatenate([[0], np.cumsum(FRAMES)]).astype(np.int64)
    assert {int(o) % CHUNK for o in off[1:]} >= {0, 1, CHUNK - 1}           # video borders on, behind and before a seam
    sets = [cases.random_set(900 + v, C, T, F) for v, F in enumerate(FRAMES)]
    bo = _pack(sets, off, C, T)
    cx = _lib.Context()
    try:
        n0 = cx.query(11)
        with poisoned():
            out = ops.nms_tubelets_batch(bo, score='score32', thresh=0.4, reduce='max', norm='min', return_overlaps=True, ctx=cx)
        assert cx.query(11) == n0 + 1
        waits = cx.query(8)
        again = ops.nms_tubelets_batch(bo, score='score32', thresh=0.4, reduce='max', norm='min', return_overlaps=True, sync=False, ctx=cx)
        assert cx.query(11) == n0 + 1 and cx.query(8) == waits              # the same offsets: neither a copy nor a wait
        cx.sync()
    finally:
        cx.close()
    assert np.array_equal(out['frame_off'], off) and tuple(out['anchors'].shape) == (len(FRAMES), C, T, 3)
    for k in ('tracks', 'det', 'pooled', 'tboxes'):
        ops._batch_flat(out[k], 1)
        assert all(same(x.cpu().numpy(), y.cpu().numpy()) for x, y in zip(out[k], again[k]))
    for v, s in enumerate(sets):
        want = spec.expected(s['tracks'], s['ntracks'], s['score3'].astype(np.float32), s['tboxes'], s['anchors'], s['series'],
                             0.4, 'min', 'max')
        one = run(s['tracks'], s['ntracks'], s['score3'].astype(np.float32), s['tboxes'], s['anchors'], s['series'], thresh=0.4,
                  reduce='max', norm='min', return_overlaps=True)
        check(one, want)
        got = dict(tracks=out['tracks'][v], tboxes=out['tboxes'][v], anchors=out['anchors'][v], ntracks=out['ntracks'][v],
                   src=out['src'][v], tscore=out['tscore'][v], by=out['by'][v], overlaps=out['overlaps'][v],
                   series=(out['det'][v], out['pooled'][v]))
        check(host(got), want)
    # a score per tubelet [V,C,T]; a dict without pooled / tboxes / anchors returns none
    s2 = torch.from_numpy(np.stack([s['score2'] for s in sets])).cuda()
    few = ops.nms_tubelets_batch(dict(tracks=bo['tracks'], ntracks=bo['ntracks'], frame_off=off, det=bo['det']), score=s2, thresh=0.4)
    assert few['pooled'] == [] and few['tboxes'] == [] and few['anchors'] is None
    for v, s in enumerate(sets):
        want = spec.expected(s['tracks'], s['ntracks'], s['score2'], series=s['series'][:1], thresh=0.4)
        assert same(few['tracks'][v].cpu().numpy(), want['tracks']) and same(few['det'][v].cpu().numpy(), want['series'][0])
        assert same(few['src'][v].cpu().numpy(), want['src']) and same(few['by'][v].cpu().numpy(), want['by'])


def test_flow_from_anchors():
    """top_anchors -> track_from_anchors -> nms_tubelets on a small planted video: the spec's result, fewer tubelets than
    anchors, and a result every consumer of tubelets takes as it is -- single video and batch."""
    import torch
    from vdetlib_amd import eval as vev, ops
    boxes, scores = cases.planted_video()
    F, B, C = scores.shape
    K, T = 3, 9
    tb, ts = dev(boxes), dev(scores)
    fr, ab, sc, _ = ops.top_anchors(tb, ts, T)
    tracks, anchors, ntracks = ops.track_from_anchors(tb, fr, ab, sc)
    det, _ = ops.anchor_propagate_tracks(tracks, ntracks, anchors, tb, ts)
    with poisoned():
        out = ops.nms_tubelets(tracks, ntracks, sc, anchors=anchors, series=det, thresh=0.5, norm='min', return_overlaps=True)
    want = spec.expected(tracks.cpu().numpy(), ntracks.cpu().numpy(), sc.cpu().numpy(), anchors=anchors.cpu().numpy(),
                         series=(det.cpu().numpy(),), thresh=0.5, norm='min')
    check(host(out), want)
    assert (want['ntracks'] == K).all() and (ntracks.cpu().numpy() == T).all()      # one tubelet per planted object
    # the consumers take the result as it is
    merged = ops.merge_tracks(out, out, 'combine')
    assert (merged['ntracks'].cpu().numpy() == 2 * K).all()
    per_frame = ops.nms_tracks(out, thresh=0.5)
    assert per_frame['cnt'].cpu().numpy().max() == K
    assert ops.rescore_tubelets(out['tracks'], out['ntracks'], tb, ts) is not None
    annots = [{'video': 'v', 'annotations': [
        {'id': str(c), 'track': [{'frame': 1, 'bbox': [0, 50, 80, 110], 'class_index': c + 1}]} for c in range(C)]}]
    ev = ops.DetEvaluator(vev.gt_table_from_annots(annots))
    boxes_kept = int((~np.isnan(want['series'][0])).sum())
    assert 0 < ev.add_tracks('v', out['tracks'], out['ntracks'], out['series'][0]) <= boxes_kept
    # the batch flow: the same video cut in two
    off = np.array([0, 5, F], np.int64)
    fr, ab, sc, _ = ops.top_anchors(tb, ts, T, frame_off=off)
    bo = ops.track_from_anchors_batch(tb, off, fr, ab, sc)
    ops.anchor_propagate_tracks_batch(bo, tb, ts)
    with poisoned():
        bout = ops.nms_tubelets_batch(bo, score=sc, thresh=0.5, norm='min')
    for v in range(2):
        one = spec.expected(bo['tracks'][v].cpu().numpy(), bo['ntracks'][v].cpu().numpy(), sc[v].cpu().numpy(),
                            anchors=bo['anchors'][v].cpu().numpy(), series=(bo['det'][v].cpu().numpy(),), thresh=0.5, norm='min')
        assert same(bout['tracks'][v].cpu().numpy(), one['tracks']) and same(bout['det'][v].cpu().numpy(), one['series'][0])
        assert same(bout['src'][v].cpu().numpy(), one['src']) and (one['ntracks'] == K).all()
        assert same(bout['anchors'][v].cpu().numpy(), one['anchors']) and same(bout['ntracks'][v].cpu().numpy(), one['ntracks'])
    again = ops.merge_tracks_batch(bout, bout, 'combine')
    assert (again['ntracks'].cpu().numpy() == 2 * K).all()
    assert ops.nms_tracks_batch(bout, score='det')['cnt'].cpu().numpy().max() == K
    assert ops.rescore_tubelets_batch(bout, tb, ts) is not None
