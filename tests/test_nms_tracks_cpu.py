"""CPU-only: ops.nms_tracks / ops.nms_tracks_batch (per-frame NMS of tubelets with still-image detections) -- the C-ABI
symbols and prototypes, the ops signatures and every ValueError that starts no device work, the specification helper
`expected` (the rows of every (class, frame) list in the header's order, then `oracle.nms`), pinned on a hand-made list, and
the input condition of the GPU cases of test_nms_tracks_gpu.py: over each generated case still-image rows and tubelet rows are
both kept and suppressed, exact score ties occur and no list raises ZeroDivisionError.

The generator: synth.vid_with_objects, the still-image survivors of oracle.nms_volume(0.3) and the re-scored tubelets of
oracle.rescored_tubelets (pooled score, regressed boxes), the tubelet set doubled -- the second copy behind the first, its boxes
jittered by +-3 px and its scores by 1e-2 * randn -- to stand in for merge_tracks('combine') of the two routes."""
import functools
import inspect
import os
import re

import numpy as np
import pytest

import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC_PAD = np.iinfo(np.int32).min
CASES = ((11, 9, 64, 3, 4), (12, 5, 130, 2, 6), (13, 3, 40, 3, 33))     # seed, F, B, C, T (T tubelets per route: 2T slots)
THRESH = 0.5


def _oracle():
    from oracle import oracle as o
    o.build()
    return o


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    an, bn = (np.isnan(a), np.isnan(b)) if a.dtype.kind == 'f' else (np.zeros(a.shape, bool), np.zeros(b.shape, bool))
    return bool(np.array_equal(an, bn) and np.array_equal(a.view(u)[~an], b.view(u)[~bn]))


def outputs_equal(got, want):
    """tracks, score and src by bit pattern (a NaN equal to a NaN), cnt and ntracks equal"""
    return all(same_bits(got[k], want[k]) for k in ('tracks', 'score', 'src')) and \
        np.array_equal(got['cnt'], want['cnt']) and np.array_equal(got['ntracks'], want['ntracks']) and \
        got['cnt'].dtype == np.int32 and got['ntracks'].dtype == np.int32


def double_tubelets(seed, tr, nt, sc, bx):
    """[C,T,...] -> [C,2T,...]: per class the nt live slots, then their jittered copies (boxes +-3 px, scores + 1e-2 * randn),
    NaN behind -- the layout merge_tracks('combine') leaves."""
    C, T, F = sc.shape
    rng = np.random.RandomState(seed)
    jit = rng.randint(-3, 4, (C, T, F, 4)).astype(np.float32)
    sj = 1e-2 * rng.randn(C, T, F)
    tracks = np.full((C, 2 * T, F, 5), np.nan, np.float32)
    score = np.full((C, 2 * T, F), np.nan)
    tboxes = np.full((C, 2 * T, F, 4), np.nan, np.float32)
    for c in range(C):
        n = int(nt[c])
        tracks[c, :n], score[c, :n], tboxes[c, :n] = tr[c, :n], sc[c, :n], bx[c, :n]
        tracks[c, n:2 * n] = tr[c, :n]
        tracks[c, n:2 * n, :, :4] += jit[c, :n]
        score[c, n:2 * n] = sc[c, :n] + sj[c, :n]
        tboxes[c, n:2 * n] = bx[c, :n] + jit[c, :n]
    return tracks, (2 * np.asarray(nt)).astype(np.int32), score, tboxes


@functools.lru_cache(maxsize=None)
def make_case(seed, F, B, C, T, video=synth.vid_with_objects):
    o = _oracle()
    made = video(seed, F, B, C)
    boxes, scores = made[0], made[1]
    keep_idx, keep_cnt = o.nms_volume(boxes, scores, 0.3)
    if T:
        tr, nt, pooled, bx = o.rescored_tubelets(boxes, scores, 0.3, 0.0, T, 0.5, 0.7, 3)
        tracks, ntracks, score, tboxes = double_tubelets(seed, tr, nt, pooled, bx)
    else:
        tracks, ntracks = np.zeros((C, 0, F, 5), np.float32), np.zeros(C, np.int32)
        score, tboxes = np.zeros((C, 0, F)), np.zeros((C, 0, F, 4), np.float32)
    case = dict(boxes=boxes, scores=scores, keep_idx=keep_idx, keep_cnt=keep_cnt, tracks=tracks, ntracks=ntracks, score=score,
                tboxes=tboxes, annot=made[2] if len(made) > 2 else None)
    for v in case.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return case


def list_rows(c, f, tracks, ntracks, score, tboxes=None, still=None, top_still=None):
    """The candidate rows of list (c, f) in the header's order: (dets [n,5] f32, f64 scores [n], src [n])."""
    T = tracks.shape[1]
    dets, s64, src = [], [], []
    if still is not None:
        boxes, scores, keep_idx, keep_cnt = still
        top = min(keep_idx.shape[2], 1024 - T) if top_still is None else top_still
        for k in range(min(int(keep_cnt[f, c]), top)):
            b = int(keep_idx[f, c, k])
            s = np.float32(scores[f, b, c])
            if not np.isnan(s):
                dets.append(list(boxes[f, b]) + [s]); s64.append(np.float64(s)); src.append(b)
    for t in range(int(ntracks[c])):
        if np.isnan(tracks[c, t, f, 0]):
            continue
        with np.errstate(over='ignore'):
            s = np.float32(score[c, t, f])
        if not np.isnan(s):
            box = tboxes[c, t, f] if tboxes is not None else tracks[c, t, f, :4]
            dets.append(list(box) + [s]); s64.append(np.float64(score[c, t, f])); src.append(-(t + 1))
    return np.array(dets, np.float32).reshape(-1, 5), np.array(s64, np.float64), np.array(src, np.int32)


def expected(tracks, ntracks, score, tboxes=None, still=None, thresh=THRESH, top_still=None, R=None):
    """THE specification: every list's rows through oracle.nms, written into the rank layout.  ZeroDivisionError where
    oracle.nms raises it.  R: rows of the output (default top_still + T); rows past R are dropped, cnt is the full count."""
    o = _oracle()
    C, T, F = tracks.shape[:3]
    if R is None:
        ts = 0 if still is None else (min(still[2].shape[2], 1024 - T) if top_still is None else top_still)
        R = max(ts + T, 1)
    out = dict(tracks=np.full((C, R, F, 5), np.nan, np.float32), score=np.full((C, R, F), np.nan),
               src=np.full((C, R, F), SRC_PAD, np.int32), cnt=np.zeros((C, F), np.int32), ntracks=np.zeros(C, np.int32))
    for c in range(C):
        for f in range(F):
            dets, s64, src = list_rows(c, f, tracks, ntracks, score, tboxes, still, top_still)
            keep = o.nms(dets, thresh)
            out['cnt'][c, f] = len(keep)
            for r, i in enumerate(keep[:R]):
                out['tracks'][c, r, f], out['score'][c, r, f], out['src'][c, r, f] = dets[i], s64[i], src[i]
            out['ntracks'][c] = max(out['ntracks'][c], min(len(keep), R))
    return out


def still_of(case):
    return case['boxes'], case['scores'], case['keep_idx'], case['keep_cnt']


# ---- symbols, prototypes, signatures -------------------------------------------------------------------------------------
def _prototype(name):
    src = open(os.path.join(ROOT, 'include', 'vdet_hip.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    m = re.search(r'\bint\s+%s\s*\(([^)]*)\)\s*;' % name, src)
    assert m, name
    return [' '.join(a.split()) for a in m.group(1).split(',')]


def test_symbols_and_prototypes():
    from vdetlib_amd import _lib
    common = ['int64_t C', 'int T', 'const float *d_tracks', 'const int32_t *d_ntracks', 'const void *d_score', 'int score_f64',
              'const float *d_tboxes', 'const float *d_boxes', 'const float *d_scores', 'int64_t B', 'const int32_t *d_keep_idx',
              'const int32_t *d_keep_cnt', 'int64_t cap', 'int top_still', 'double thresh', 'int R', 'float *d_tracks_out',
              'double *d_score_out', 'int32_t *d_src_out', 'int32_t *d_cnt_out', 'int32_t *d_ntracks_out']
    assert _prototype('vdet_nms_tracks') == ['vdet_ctx *ctx', 'int64_t F'] + common
    assert _prototype('vdet_nms_tracks_batch') == ['vdet_ctx *ctx', 'const int64_t *h_frame_off', 'int64_t V'] + common
    assert len(_lib.SYMBOLS['vdet_nms_tracks'][1]) == 2 + len(common)
    assert len(_lib.SYMBOLS['vdet_nms_tracks_batch'][1]) == 3 + len(common)
    L = _lib.load_library()
    assert hasattr(L, 'vdet_nms_tracks') and hasattr(L, 'vdet_nms_tracks_batch')
    hdr = open(os.path.join(ROOT, 'include', 'vdet_hip.h')).read()
    assert 'device tubelet NMS' in hdr and 'INT32_MIN' in hdr


def test_ops_signatures():
    from vdetlib_amd import ops
    p = inspect.signature(ops.nms_tracks).parameters
    assert list(p)[:3] == ['tracks', 'ntracks', 'score']
    assert {k: p[k].default for k in ('tboxes', 'still', 'thresh', 'top_still', 'cap', 'sync', 'ctx')} == \
        dict(tboxes=None, still=None, thresh=0.5, top_still=None, cap=None, sync=True, ctx=None)
    q = inspect.signature(ops.nms_tracks_batch).parameters
    assert list(q)[0] == 'batch_out' and q['score'].default == 'pooled' and q['still'].default is None and q['thresh'].default == 0.5
    assert 'add_detections' in vars(ops.DetEvaluator)
    assert list(inspect.signature(ops.DetEvaluator.add_detections).parameters) == ['self', 'video_or_videos', 'out']


def _host_args(C=2, T=3, F=4, B=5, k=5):
    import torch
    return dict(tracks=torch.zeros(C, T, F, 5), ntracks=torch.zeros(C, dtype=torch.int32), score=torch.zeros(C, T, F, dtype=torch.float64),
                tboxes=torch.zeros(C, T, F, 4),
                still=(torch.zeros(F, B, 4), torch.zeros(F, B, C), torch.zeros(F, C, k, dtype=torch.int32),
                       torch.zeros(F, C, dtype=torch.int32)))


def _still_with(a, i, x):
    s = list(a['still'])
    s[i] = x
    return tuple(s)


def test_value_errors_start_no_device_work():
    """host tensors throughout: whatever passes the shape checks ends at the device check, a ValueError as well"""
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
        {},                                             # every shape is right: host tensors
    ]
    for kw in bad:
        args = dict(a, **kw)
        with pytest.raises(ValueError) as e:
            ops.nms_tracks(args.pop('tracks'), args.pop('ntracks'), args.pop('score'), **args)
        assert ('same GPU' in str(e.value)) == (kw == {}), (kw.keys(), str(e.value))
    # the dict form: ntracks must stay None, score names a series
    d = dict(tracks=a['tracks'], ntracks=a['ntracks'], series=(a['score'],), tboxes=a['tboxes'])
    for kw in (dict(ntracks=a['ntracks']), dict(score=1), dict(score='pooled'), {}):
        with pytest.raises(ValueError):
            ops.nms_tracks(d, **kw)
    with pytest.raises(ValueError):
        ops.nms_tracks(dict(tracks=a['tracks']))
    # C*cap*F and C*T*F below 2^31 - 16 (meta tensors: no memory behind them)
    with pytest.raises(ValueError, match="2\\^31"):
        ops.nms_tracks(torch.empty(3000, 0, 1000, 5, device='meta'), torch.empty(3000, dtype=torch.int32, device='meta'),
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
        (dict(bo, frame_off=np.array([0, 2, 2])), {}), (dict(bo, frame_off=np.array([1, 2, 5])), {}), ({k: v for k, v in bo.items() if k != 'ntracks'}, {}),
        (bo, dict(score='nope')), (bo, dict(score=3)), (dict(bo, pooled=[]), {}), (dict(bo, pooled=bo['pooled'][:1]), {}),
        (dict(bo, ntracks=torch.zeros(C, dtype=torch.int32)), {}), (dict(bo, tracks=bo['tracks'][::-1]), {}),
        (dict(bo, tboxes=bo['tracks']), {}), (dict(bo, pooled=[bo['pooled'][0], bo['det'][1]]), {}),
        (bo, dict(still=(still[0][:4],) + still[1:])), (bo, dict(top_still=3)), (bo, dict(still=still, top_still=1022)), (bo, dict(cap=0)),
        (dict(bo, pooled=[x.clone() for x in bo['pooled']]), {}),      # not consecutive views of one allocation
        (bo, {}), (bo, dict(score='det', still=still)),                 # every shape is right: host tensors
    ]
    for i, (b, kw) in enumerate(bad):
        with pytest.raises(ValueError) as e:
            ops.nms_tracks_batch(b, **kw)
        assert ('same GPU' in str(e.value)) == (i >= len(bad) - 2), (i, str(e.value))


# ---- the specification helper ---------------------------------------------------------------------------------------------
def test_expected_on_a_hand_made_list():
    """Six candidate rows of one list (C = F = 1), written out:
      still k=0: box A, 0.9            tubelet t=0: box A shifted by 2 px, 0.9   (a tie with k=0: the tubelet row goes first)
      still k=1: box B, 0.8            tubelet t=1: box B, NaN score             (absent)
      still k=2: box C, 0.7            tubelet t=2: box C, 0.95 -- but ntracks = 2: a dead slot, never read
    Order: t=0 (0.9, higher row), k=0 (0.9; IoU with t=0 about 0.92: suppressed), k=1 (0.8, kept), k=2 (0.7, kept)."""
    A, B, Cx = [10, 10, 109, 109], [300, 300, 399, 399], [600, 50, 699, 149]
    boxes = np.array([[A, B, Cx, [0, 0, 5, 5]]], np.float32)                 # [1,4,4]
    scores = np.array([[[0.9], [0.8], [0.7], [0.99]]], np.float32)           # [1,4,1]: box 3 is behind the count
    keep_idx = np.array([[[0, 1, 2, 3]]], np.int32)
    keep_cnt = np.array([[3]], np.int32)
    tracks = np.zeros((1, 3, 1, 5), np.float32)
    tracks[0, :, 0, :4] = [[12, 12, 111, 111], B, Cx]
    ntracks = np.array([2], np.int32)
    score = np.array([[[np.float64(np.float32(0.9))], [np.nan], [0.95]]])
    dets, s64, src = list_rows(0, 0, tracks, ntracks, score, None, (boxes, scores, keep_idx, keep_cnt))
    assert src.tolist() == [0, 1, 2, -1] and dets.shape == (4, 5)
    out = expected(tracks, ntracks, score, None, (boxes, scores, keep_idx, keep_cnt))
    assert out['tracks'].shape == (1, 7, 1, 5) and out['cnt'].tolist() == [[3]] and out['ntracks'].tolist() == [3]
    assert out['src'][0, :, 0].tolist() == [-1, 1, 2] + [SRC_PAD] * 4
    assert same_bits(out['tracks'][0, :3, 0], np.array([[12, 12, 111, 111, 0.9], B + [0.8], Cx + [0.7]], np.float32))
    assert same_bits(out['score'][0, :3, 0], np.array([0.9, 0.8, 0.7], np.float32).astype(np.float64))
    assert np.isnan(out['tracks'][0, 3:]).all() and np.isnan(out['score'][0, 3:]).all()
    # the same tie inside one source: the higher slot first
    tracks2 = np.zeros((1, 2, 1, 5), np.float32)
    tracks2[0, :, 0, :4] = [A, [12, 12, 111, 111]]
    out = expected(tracks2, np.array([2], np.int32), np.full((1, 2, 1), 0.5))
    assert out['src'][0, :, 0].tolist() == [-2, SRC_PAD] and out['cnt'].tolist() == [[1]]
    # a capacity below the survivor count: the count stays, the rows end at R
    out = expected(tracks, ntracks, score, None, (boxes, scores, keep_idx, keep_cnt), R=2)
    assert out['cnt'].tolist() == [[3]] and out['ntracks'].tolist() == [2] and out['src'][0, :, 0].tolist() == [-1, 1]


@pytest.mark.parametrize("shape", CASES)
def test_generated_cases_exercise_every_outcome(shape):
    """The input condition of the GPU cases, checked here on the CPU."""
    case = make_case(*shape)
    seed, F, B, C, T = shape
    o = _oracle()
    ks = ss = kt = st = ties = 0
    for c in range(C):
        for f in range(F):
            dets, _, src = list_rows(c, f, case['tracks'], case['ntracks'], case['score'], case['tboxes'], still_of(case))
            keep = o.nms(dets, THRESH)                      # (raises ZeroDivisionError: the condition "no list raises")
            kept = np.zeros(len(dets), bool)
            kept[keep] = True
            ks += int((kept & (src >= 0)).sum()); ss += int((~kept & (src >= 0)).sum())
            kt += int((kept & (src < 0)).sum()); st += int((~kept & (src < 0)).sum())
            ties += len(dets) - len(np.unique(dets[:, 4]))
    assert min(ks, ss, kt, st, ties) >= 1, (ks, ss, kt, st, ties)
    expected(case['tracks'], case['ntracks'], case['score'], case['tboxes'], still_of(case))
