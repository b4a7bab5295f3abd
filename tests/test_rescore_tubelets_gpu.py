"""-m gpu: ops.rescore_tubelets / ops.rescore_tubelets_batch (csrc/rescore_kernels.hpp) against the numpy specification of
tests/rescore_spec.py, the existing re-scoring paths, the single-video call on every slice of a batch, and the reference's
recorded outputs.  Every comparison is exact: f64 / f32 values equal with a NaN equal to a NaN, src equal."""
import functools

import numpy as np
import pytest

import rescore_spec as R
import synth

pytestmark = pytest.mark.gpu

KEYS = ('det', 'pooled', 'tboxes', 'src')


def g(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def n_(t):
    return t.cpu().numpy()


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind == 'f')


def batch_dict(tracks, ntracks, off):
    """per-video numpy tracks -> a dict in video_batch's layout (consecutive views of one device buffer)"""
    import torch
    C, T = tracks[0].shape[:2]
    flat = g(np.concatenate([np.ascontiguousarray(t, np.float32).ravel() for t in tracks]))
    tv = [flat[C * T * 5 * off[v]: C * T * 5 * off[v + 1]].view(C, T, off[v + 1] - off[v], 5) for v in range(len(off) - 1)]
    return dict(tracks=tv, ntracks=g(np.asarray(ntracks, np.int32)), frame_off=np.asarray(off, np.int64),
                anchors=torch.zeros((len(off) - 1, C, T, 3), dtype=torch.float32, device='cuda'))


def check_views(out, want, what=''):
    """out: a rescore_tubelets_batch dict, want: spec_batch's [det, pooled, tboxes, src] per-video lists"""
    for k, w in zip(KEYS, want):
        for v in range(len(w)):
            x = n_(out[k][v])
            print('%s %s video %d: %d of %d elements differ' % (what, k, v, int((~((x == w[v]) | ((x != x) & (w[v] != w[v])))).sum()), x.size))
            assert same(x, w[v]), (what, k, v)


MODES = {'complete_w3': dict(window=3), 'raw_w1': dict(complete=False, window=1), 'floor64_w5': dict(floor=np.float64, window=5),
         'floor32': dict(floor=np.float32)}


def mode_args(mode, floor):
    """(keyword arguments of the spec, of the device call) for per-video numpy floors"""
    kw = dict(MODES[mode])
    dt = kw.pop('floor', None)
    if dt is None:
        return kw, kw
    fl = [f.astype(dt) for f in floor]
    if dt is np.float64:                                             # one flat tensor in the batch layout
        return dict(kw, floor=fl), dict(kw, floor=g(np.concatenate([f.ravel() for f in fl])))
    return dict(kw, floor=fl), dict(kw, floor=[g(f) for f in fl])     # separate per-video tensors


@functools.lru_cache(maxsize=None)
def parity_case(B, off):
    boxes, scores, tracks, ntracks, floor, cz = R.batch_case(R.PARITY_SEEDS[B], off, B)
    R.check_census(cz, off)
    return boxes, scores, tracks, ntracks, floor


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("off", ((0, 9), (0, 1, 2), (0, 3, 4, 13)), ids=("09", "012", "03413"))
@pytest.mark.parametrize("B", (5, 300, 1100))
def test_spec_parity(oracle, B, off, mode):
    """Tubelets WITH holes, misses at both ends and inside, tied maxima, both floor outcomes: a frame-addressed completion or
    pool (rescore_tracks' treatment of its contiguous tubelets) fails this test."""
    from vdetlib_amd import ops
    boxes, scores, tracks, ntracks, floor = parity_case(B, off)
    skw, dkw = mode_args(mode, floor)
    want, eindex = R.spec_batch(tracks, ntracks, boxes, scores, off, **skw)
    assert not eindex
    bo = batch_dict(tracks, ntracks, off)
    keys = sorted(bo)
    out = ops.rescore_tubelets_batch(bo, g(boxes), g(scores), **dkw)
    check_views(out, want, mode)
    assert sorted(bo) == keys and out is not bo                              # a NEW dict, the input untouched
    assert all(same(n_(a), t) for a, t in zip(out['tracks'], tracks)) and out['ntracks'] is bo['ntracks']
    if len(off) == 2:                                                       # ... and the single-video entry point
        fl = skw.get('floor')
        one = ops.rescore_tubelets(bo['tracks'][0], bo['ntracks'][0], g(boxes), g(scores),
                                   **dict(dkw, floor=None if fl is None else g(fl[0])))
        for k, x in zip(KEYS, one):
            assert same(n_(x), want[KEYS.index(k)][0]), k


@pytest.mark.parametrize("F", (63, 64, 65, 130))
def test_chunk_edges_of_the_ordinal_compaction(oracle, F):
    from vdetlib_amd import ops
    boxes, scores = R.volume(9200 + F, F, 5, 2)
    tracks, floor = R.tubelets(9200 + F, boxes, 2, 3)
    nt = np.full(2, 3, np.int32)
    holes = np.isnan(tracks[..., 0])
    assert holes[:, :, 62:66].any() and (~holes[:, :, 62:66]).any() if F > 66 else holes.any()
    for skw, dkw in ((dict(window=5), dict(window=5)), (dict(floor=floor, window=3), dict(floor=g(floor), window=3))):
        want = R.spec(tracks, nt, boxes, scores, **skw)
        assert not want[4]
        got = ops.rescore_tubelets(g(tracks), g(nt), g(boxes), g(scores), **dkw)
        for k, x, w in zip(KEYS, got, want):
            assert same(n_(x), w), (k, sorted(skw))


def test_a_long_video(oracle):
    """1600 frames: beyond the LDS stage of the one-wave-per-series kernel, next to a 9-frame video that takes it."""
    from vdetlib_amd import ops
    off, B, C, T = (0, 1600, 1609), 5, 1, 2
    boxes, scores, tracks, ntracks, floor, cz = R.batch_case(9300, off, B, C, T)
    assert cz['all_miss'] == 0 and cz['leading'] + cz['trailing'] > 0 and cz['interior'] > 0 and cz['inner_hole'] > 0
    bo = batch_dict(tracks, ntracks, off)
    for skw, dkw in ((dict(window=5), dict(window=5)), (dict(complete=False, window=3), dict(complete=False, window=3))):
        want, eindex = R.spec_batch(tracks, ntracks, boxes, scores, off, **skw)
        assert not eindex
        check_views(ops.rescore_tubelets_batch(bo, g(boxes), g(scores), **dkw), want, 'long')


def test_existing_paths_reproduced():
    """Hole-free tubelets of the greedy tracker: bit for bit rescore_tracks' and video_batch's own re-scoring."""
    from vdetlib_amd import ops
    F, B, C, T = 12, 300, 3, 4
    boxes, scores = synth.coherent_video(9400, F, B, C)
    tb, ts = g(boxes), g(scores)
    _, _, tracks, anchors, ntracks = ops.nms_track_volume(tb, ts, max_tracks=T)
    det0, pooled0, box0 = ops.rescore_tracks(tracks, ntracks, tb, ts)
    det, pooled, tboxes, src = ops.rescore_tubelets(tracks, ntracks, tb, ts)
    assert int(n_(ntracks).min()) >= 1 and (n_(det0) == n_(det0)).any()
    assert same(n_(det), n_(det0)) and same(n_(pooled), n_(pooled0)) and same(n_(tboxes), n_(box0))
    assert (n_(src)[np.isnan(n_(det))] == -1).all() and (n_(src) >= 0).any()
    off = [0, 5, 12]
    vb = ops.video_batch(tb, ts, off, max_tracks=T, rescore=True)
    out = ops.rescore_tubelets_batch(vb, tb, ts)
    for v in range(2):
        for k in ('det', 'pooled', 'tboxes'):
            assert same(n_(out[k][v]), n_(vb[k][v])), (k, v)
        assert same(n_(out['tracks'][v]), n_(vb['tracks'][v]))
    assert 'keep_idx' not in out and out['anchors'] is vb['anchors']


def anchor_batch(off, B, C, T, seed):
    """anchor-route tubelets of a coherent volume: (boxes, scores, their device copies, the batch dict with the propagated det)"""
    from vdetlib_amd import ops
    boxes, scores = synth.coherent_video(seed, off[-1], B, C)
    tb, ts = g(boxes), g(scores)
    fr, ab, sc, _ = ops.top_anchors(tb, ts, T, frame_off=off)
    fr = fr.clone()
    fr[0, 0, 1] = 0                                                  # an empty slot below a live one
    fr[-1, -1, T - 1] = 0                                            # an empty LAST slot: ntracks = T - 1 there
    out = ops.track_from_anchors_batch(tb, off, fr, ab, sc)
    ops.anchor_propagate_tracks_batch(out, tb, ts)
    return boxes, scores, tb, ts, out


def check_batch_equals_singles(bo, tb, ts, boxes, scores, oracle, **kw):
    from vdetlib_amd import ops
    off = [int(x) for x in bo['frame_off']]
    out = ops.rescore_tubelets_batch(bo, tb, ts, **kw)
    tracks = [n_(t) for t in bo['tracks']]
    want, eindex = R.spec_batch(tracks, n_(bo['ntracks']), boxes, scores, off, **kw)
    assert not eindex
    check_views(out, want)
    for v in range(len(off) - 1):
        one = ops.rescore_tubelets(bo['tracks'][v], bo['ntracks'][v], tb[off[v]:off[v + 1]], ts[off[v]:off[v + 1]], **kw)
        for k, x in zip(KEYS, one):
            assert same(n_(out[k][v]), n_(x)), (k, v)
    return out


def test_batch_equals_the_single_video_call(oracle):
    from vdetlib_amd import ops
    off, B, C, T = [0, 3, 4, 13], 70, 2, 3
    boxes, scores, tb, ts, out = anchor_batch(off, B, C, T, 9500)
    nt = n_(out['ntracks'])
    assert nt[-1, -1] == T - 1 and nt[0, 0] == T and np.isnan(n_(out['tracks'][0])[0, 1]).all()
    res = check_batch_equals_singles(out, tb, ts, boxes, scores, oracle)
    assert np.isnan(n_(res['det'][0])[0, 1]).all() and (n_(res['src'][0])[0, 1] == -1).all()
    # merged sets: 2T slots per class, the live ones of b behind those of a
    other = ops.track_from_anchors_batch(tb, off, *ops.top_anchors(tb, ts, T, frame_off=off)[:3], link_thres=0.9, max_frames=3)
    ops.anchor_propagate_tracks_batch(other, tb, ts)
    merged = ops.merge_tracks_batch(out, other, 'combine')
    assert merged['tracks'][0].shape[1] == 2 * T
    check_batch_equals_singles(merged, tb, ts, boxes, scores, oracle, window=5)


def test_interpolated_tubelets(oracle):
    """tubelets tracked on every second frame and interpolated back: fractional boxes against the dense volume"""
    from vdetlib_amd import ops
    doff, B, C, T = [0, 5, 13], 70, 2, 3
    boxes, scores = synth.coherent_video(9600, doff[-1], B, C)
    rows = [0, 2, 4, 5, 7, 9, 11]
    soff = [0, 3, 7]
    sb, ss = g(boxes[rows]), g(scores[rows])
    fr, ab, sc, _ = ops.top_anchors(sb, ss, T, frame_off=soff)
    out = ops.track_from_anchors_batch(sb, soff, fr, ab, sc, link_thres=0.3)
    dense = ops.interpolate_tracks_batch(out, np.array([1, 3, 5, 1, 3, 5, 7], np.int32), [5, 8])
    x = np.concatenate([n_(t)[..., :4].ravel() for t in dense['tracks']])
    assert (x[x == x] % 1 != 0).any()                                # fractional boxes
    assert [int(v) for v in dense['frame_off']] == doff
    check_batch_equals_singles(dense, g(boxes), g(scores), boxes, scores, oracle, overlap_thres=0.5)


@pytest.mark.parametrize("knob", ["VDET_NO_INDEX", "VDET_FORCE_GENERAL"])
def test_fallback_paths_agree(oracle, monkeypatch, knob):
    """whole-frame scans instead of the x-window, on a volume with an irregular frame (a NaN box, an inf-wide box)"""
    import torch
    from vdetlib_amd import _lib, ops
    off, B = (0, 3, 4, 13), 300
    boxes, scores, tracks, ntracks, floor = parity_case(B, off)
    boxes = boxes.copy()
    boxes[5, 7] = np.nan
    boxes[6, 9, 2] = np.inf
    boxes[6, 11, 0] = -np.inf
    want, eindex = R.spec_batch(tracks, ntracks, boxes, scores, off, window=3)
    assert not eindex
    bo = batch_dict(tracks, ntracks, off)
    monkeypatch.setenv(knob, "1")
    cx = _lib.Context(torch.cuda.current_device())
    monkeypatch.delenv(knob)
    cd = _lib.Context(torch.cuda.current_device())
    try:
        for c in (cx, cd):
            check_views(ops.rescore_tubelets_batch(bo, g(boxes), g(scores), ctx=c), want, knob)
    finally:
        cx.close()
        cd.close()


def test_nan_and_inf_rules(oracle):
    from vdetlib_amd import ops
    F, B, C, T = 9, 5, 2, 3
    boxes, scores = R.volume(9100, F, B, C)
    tracks, floor = R.tubelets(9100, boxes, C, T)
    nt = np.full(C, T, np.int32)
    _, _, _, src0, _ = R.spec(tracks, nt, boxes, scores)
    hits = np.argwhere(src0 >= 0)
    # three hits of class 0 on different frames: their candidates are the followed proposal p and p + 1
    pick, seen = [], set()
    for c, t, f in hits:
        if c == 0 and f not in seen:
            seen.add(f)
            pick.append((int(t), int(f), int(src0[c, t, f]) & ~1))
    assert len(pick) >= 3
    scores = scores.copy()
    (t1, f1, p1), (t2, f2, p2), (t3, f3, p3) = pick[:3]
    scores[f1, p1 + 1, 0] = np.nan                                  # a NaN behind a number: the NaN wins
    scores[f2, p2, 0] = scores[f2, p2 + 1, 0] = np.nan              # two NaNs: the first
    scores[f3, p3, 0] = scores[f3, p3 + 1, 0] = -np.inf             # -inf: a hit whose score counts as missing
    floor = floor.copy()
    floor[1, 0, :] = np.nan                                         # a NaN floor stands
    dt, dn, db, ds = g(tracks), g(nt), g(boxes), g(scores)
    want = R.spec(tracks, nt, boxes, scores, window=3)
    got = [n_(x) for x in ops.rescore_tubelets(dt, dn, db, ds, complete=False, window=1)]
    assert np.isnan(got[0][0, t1, f1]) and got[3][0, t1, f1] == p1 + 1
    assert np.isnan(got[0][0, t2, f2]) and got[3][0, t2, f2] == p2
    assert got[0][0, t3, f3] == -np.inf and got[3][0, t3, f3] == p3
    for skw, dkw in ((dict(window=3), dict(window=3)), (dict(complete=False, window=1), dict(complete=False, window=1)),
                     (dict(floor=floor, window=3), dict(floor=g(floor), window=3))):
        want = R.spec(tracks, nt, boxes, scores, **skw)
        got = [n_(x) for x in ops.rescore_tubelets(dt, dn, db, ds, **dkw)]
        assert not want[4]
        for k, x, w in zip(KEYS, got, want):
            assert same(x, w), (k, sorted(skw))
    # with a floor a NaN never beats it
    assert got[3][0, t1, f1] == -1 and got[0][0, t1, f1] == floor[0, t1, f1] and got[3][0, t2, f2] == -1
    assert np.isnan(got[0][1, 0][~np.isnan(tracks[1, 0, :, 0])]).all() and (got[3][1, 0] == -1).all()


def all_miss_case():
    boxes, scores = R.volume(9100, 9, 5, 2)
    tracks, floor = R.tubelets(9100, boxes, 2, 3)
    present = ~np.isnan(tracks[1, 2, :, 0])
    tracks[1, 2, present, :4] += np.float32(2000)                   # every box of one tubelet far from every detection
    return boxes, scores, tracks, np.full(2, 3, np.int32)


def test_all_miss_tubelet_raises(oracle):
    from vdetlib_amd import _lib, ops
    boxes, scores, tracks, nt = all_miss_case()
    want = R.spec(tracks, nt, boxes, scores)
    assert want[4]
    dt, dn, db, ds = g(tracks), g(nt), g(boxes), g(scores)
    cx = _lib.Context()
    try:
        with pytest.raises(IndexError):
            ops.rescore_tubelets(dt, dn, db, ds, ctx=cx)
        got = ops.rescore_tubelets(dt, dn, db, ds, sync=False, ctx=cx)
        with pytest.raises(IndexError):
            cx.sync()
        for k, x, w in zip(KEYS, got, want):                        # the tubelet keeps its sentinels, every other is served
            assert same(n_(x), w), k
        assert (n_(got[0])[1, 2][~np.isnan(tracks[1, 2, :, 0])] == -1e5).all() and np.isnan(n_(got[1])[1, 2]).all()
        for kw in (dict(complete=False), dict(floor=g(np.zeros((2, 3, 9))), complete=False)):
            ops.rescore_tubelets(dt, dn, db, ds, ctx=cx, **kw)     # no completion: nothing to raise
    finally:
        cx.close()


def test_argument_errors():
    import torch
    from vdetlib_amd import ops
    boxes, scores, tracks, nt = all_miss_case()
    dt, dn, db, ds = g(tracks), g(nt), g(boxes), g(scores)
    bo = batch_dict([tracks], nt[None], [0, 9])
    for fn in (lambda: ops.rescore_tubelets(dt, dn, db, ds, window=4),
               lambda: ops.rescore_tubelets_batch(bo, db, ds, window=2),
               lambda: ops.rescore_tubelets(dt.double(), dn, db, ds),
               lambda: ops.rescore_tubelets(dt, dn.long(), db, ds),
               lambda: ops.rescore_tubelets(dt, dn, db, ds, floor=torch.zeros((2, 3, 9), dtype=torch.int32, device='cuda')),
               lambda: ops.rescore_tubelets(dt, dn, db, ds[:, :, :1]),
               lambda: ops.rescore_tubelets(dt, dn, db[:8], ds),
               lambda: ops.rescore_tubelets(dt, dn, db, ds, floor=torch.zeros((2, 3, 8), device='cuda')),
               lambda: ops.rescore_tubelets(dt, dn, db, ds.cpu()),
               lambda: ops.rescore_tubelets_batch(bo, db, ds, floor=[torch.zeros((2, 3, 9))]),
               lambda: ops.rescore_tubelets(g(tracks[:, :, :1]), dn, torch.zeros((1, 32768, 4), device='cuda'),
                                            torch.zeros((1, 32768, 2), device='cuda')),
               lambda: ops.rescore_tubelets_batch({}, db, ds),
               lambda: ops.rescore_tubelets_batch(dict(bo, tracks=[dt[:, :, :8]]), db, ds),
               lambda: ops.rescore_tubelets_batch(dict(bo, ntracks=dn), db, ds)):
        with pytest.raises(ValueError):
            fn()
    with pytest.raises(ValueError, match='Window size must be odd!'):
        ops.rescore_tubelets(dt, dn, db, ds, window=0)
    with pytest.raises(ValueError, match='not a .* result'):
        ops.rescore_tubelets_batch(dict(frame_off=[0, 9]), db, ds)


def test_consumers_take_the_new_dict(oracle):
    from vdetlib_amd import eval as vev, ops
    from vdetlib_amd.vdet.tcn import TCNNet
    off, B, C, T = [0, 3, 4, 13], 70, 2, 3
    V = len(off) - 1
    boxes, scores, tb, ts, prop = anchor_batch(off, B, C, T, 9700)
    res = ops.rescore_tubelets_batch(prop, tb, ts, overlap_thres=0.5)
    # 'max' of the two scorings of the same tubelets: the propagated anchor score against the re-scored one
    merged = ops.merge_tracks_batch(prop, res, 'max')
    for v in range(V):
        a, b = n_(prop['det'][v]), n_(res['det'][v])
        with np.errstate(invalid='ignore'):
            fb = b > a
        assert same(n_(merged['det'][v]), np.where(fb, b, a)) and same(n_(merged['from_b'][v]).astype(bool), fb)
    assert not np.concatenate([n_(x).ravel() for x in merged['from_b']]).all()
    # the TCN on det, per-frame NMS on pooled / tboxes
    net = TCNNet.random([(n, 1) for n in ('det_scores', 'track_scores', 'anchors', 'abs_anchors')], hidden=(8,), kernel=3, seed=3)
    conv = ops.tcn_tracks_batch(net, res, series='det')
    nms = ops.nms_tracks_batch(res, score='pooled')
    for v in range(V):
        tr, nt, an = res['tracks'][v], res['ntracks'][v], res['anchors'][v]
        assert same(n_(conv[v]), n_(ops.tcn_tracks(net, tr, nt, an, res['det'][v])))
        one = ops.nms_tracks(tr, nt, res['pooled'][v], tboxes=res['tboxes'][v])
        for k in ('tracks', 'score', 'src'):
            assert same(n_(nms[k][v]), n_(one[k])), (k, v)
    # the evaluator
    names = ['v%d' % v for v in range(V)]
    annots = [{'video': names[v], 'annotations': [{'id': '0', 'track': [
        {'frame': f + 1, 'bbox': [int(x) for x in n_(res['tboxes'][v])[0, 0, f]], 'class_index': 1, 'class': 'c1'}
        for f in range(off[v + 1] - off[v]) if not np.isnan(n_(res['tboxes'][v])[0, 0, f, 0])]}]} for v in range(V)]
    gt = vev.gt_table_from_annots(annots)
    eb, e1 = ops.DetEvaluator(gt, classes=[1, 2]), ops.DetEvaluator(gt, classes=[1, 2])
    n_batch = eb.add_batch(names, res)
    n_single = sum(e1.add_tracks(names[v], res['tracks'][v], res['ntracks'][v], res['pooled'][v], boxes=res['tboxes'][v])
                   for v in range(V))
    assert n_batch == n_single > 0
    (ab, mb), (a1, m1) = eb.compute(), e1.compute()
    assert sorted(ab) == sorted(a1) and all(ab[k] == a1[k] or (ab[k] != ab[k] and a1[k] != a1[k]) for k in a1)
    _, views, _, _ = ops.tubelets_overlap_batch(eb, names, res, use_tboxes=True)
    assert len(views) == V


def test_reference_goldens():
    """The device against the REFERENCE's recorded outputs on tubelets with holes (tests/golden/make_rescore_golden.py):
    raw_dets_spatial_max_pooling + score_proto_temporal_maxpool (3, 5), and rcnn_sampling_dets_scoring behind its CNN."""
    from vdetlib_amd import ops
    for case in R.load_golden():
        boxes, scores, tracks, floor = R.golden_inputs(case)
        dt, dn, db, ds = g(tracks), g(np.full(case['C'], case['T'], np.int32)), g(boxes), g(scores)
        gold = R.golden_arrays(case, 'maxpool')
        for window, key in ((3, 'pool3'), (5, 'pool5')):
            det, pooled, tb, _ = ops.rescore_tubelets(dt, dn, db, ds, overlap_thres=case['overlap_thres'], window=window)
            assert same(n_(det), gold['det_score']) and same(n_(pooled), gold[key]), (case['seed'], window)
            assert same(n_(tb).astype(np.float64), gold['bbox'])
        gold = R.golden_arrays(case, 'sampling')
        det, pooled, tb, src = ops.rescore_tubelets(dt, dn, db, ds, floor=g(floor), overlap_thres=case['overlap_thres'], window=1)
        assert same(n_(det), gold['det_score']) and same(n_(tb).astype(np.float64), gold['bbox']) and same(n_(pooled), n_(det))
