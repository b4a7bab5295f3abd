"""-m gpu: the anchor route over video batches -- ops.top_anchors(frame_off=...), ops.track_from_anchors_batch,
ops.anchor_propagate_tracks_batch -- against the single-video calls on every video's own slice (bit for bit, NaN rows
included), video boundaries, empty slots, errors, the consumers of video_batch's layout, the dict route end to end, and
the staging of the per-video table (vdet_query 11)."""
import numpy as np
import pytest

import synth

pytestmark = pytest.mark.gpu


def same(a, b):
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def g(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def n_(t):
    return t.cpu().numpy()


def coherent_video(seed, F, B, C):
    """boxes that drift 3 px per frame (so chains link across frames -- and would across videos), random scores"""
    rng = np.random.RandomState(seed)
    base = synth.boxes_1(rng, B)
    boxes = np.stack([base + np.float32(3 * f) for f in range(F)], 0).astype(np.float32)
    scores = rng.rand(F, B, C).astype(np.float32)
    return boxes, scores


def per_video(tb, ts, off, fr, ab, sc, **kw):
    """the single-video calls on every slice"""
    from vdetlib_amd import ops
    out = []
    for v in range(len(off) - 1):
        sl = slice(int(off[v]), int(off[v + 1]))
        tr, an, nt = ops.track_from_anchors(tb[sl], fr[v], ab[v], None if sc is None else sc[v], **kw)
        det, best = ops.anchor_propagate_tracks(tr, nt, an, tb[sl], ts[sl])
        out.append((tr, an, nt, det, best))
    return out


def check_batch(out, det, best, singles):
    for v, (tr, an, nt, d1, b1) in enumerate(singles):
        assert same(n_(out['tracks'][v]), n_(tr)), v
        assert same(n_(out['anchors'][v]), n_(an)) and same(n_(out['ntracks'][v]), n_(nt)), v
        assert same(n_(det[v]), n_(d1)) and same(n_(best[v]), n_(b1)), v


@pytest.mark.parametrize("B", (5, 300, 1100))
@pytest.mark.parametrize("off", ([0, 1, 2], [0, 3, 4, 9]), ids=("012", "0349"))
def test_batch_equals_the_single_video_calls(off, B):
    from vdetlib_amd import ops
    C, T, F = 2, 3, off[-1]
    boxes, scores = coherent_video(8100 + B + F, F, B, C)
    boxes[F - 1, 0] = np.nan                                         # a NaN box in the volume
    tb, ts = g(boxes), g(scores)
    sel = ops.top_anchors(tb, ts, T, frame_off=off)
    assert tuple(sel[0].shape) == (len(off) - 1, C, T) and tuple(sel[1].shape) == (len(off) - 1, C, T, 4)
    for v in range(len(off) - 1):
        one = ops.top_anchors(tb[off[v]:off[v + 1]].contiguous(), ts[off[v]:off[v + 1]].contiguous(), T)
        for a, b in zip(sel, one):
            assert np.array_equal(n_(a[v]).view(np.uint32), n_(b).view(np.uint32)), v
    fr, ab, sc, _ = sel
    for kw in (dict(), dict(link_thres=0.9, max_frames=3)):
        out = ops.track_from_anchors_batch(tb, off, fr, ab, sc, **kw)
        det, best = ops.anchor_propagate_tracks_batch(out, tb, ts)
        assert out['det'] is det and tuple(best.shape) == (len(off) - 1, C, T)
        check_batch(out, det, best, per_video(tb, ts, off, fr, ab, sc, **kw))
    # (the comparison above is not NaN against NaN: every live slot whose anchor box is a number has its anchor row; the
    # planted NaN box is an anchor itself when B = 5, and its tubelet has no row)
    live = (n_(fr) > 0) & ~np.isnan(n_(ab)).any(-1)
    assert live.sum() >= (len(off) - 1) * C * T - C
    assert sum(int((~np.isnan(n_(t)[..., 0])).sum()) for t in out['tracks']) >= live.sum()


def boundary_case():
    """videos of 3, 1 and 4 frames; one object drifting through ALL frames at box 2: a chain that ignored the video
    boundaries would run through the whole volume"""
    off = [0, 3, 4, 8]
    F, B = 8, 70
    rng = np.random.RandomState(8200)
    boxes = np.stack([synth.boxes_1(rng, B) for _ in range(F)], 0).astype(np.float32)
    obj = np.array([300, 200, 420, 330], np.float32)
    for f in range(F):
        boxes[f, 2] = obj + np.float32(3 * f)
    scores = rng.rand(F, B, 2).astype(np.float32)
    fr = np.zeros((3, 2, 3), np.int32)
    ab = np.zeros((3, 2, 3, 4), np.float32)
    fr[0, 0, 0] = 3; ab[0, 0, 0] = boxes[2, 2]                     # the last frame of video 0
    fr[1, 0, 1] = 1; ab[1, 0, 1] = boxes[3, 2]                     # the one-frame video (slot 0 below it is empty)
    fr[2, 1, 0] = 1; ab[2, 1, 0] = boxes[4, 2]                     # the first frame of video 2
    fr[2, 1, 2] = 2; ab[2, 1, 2] = boxes[5, 2]
    return off, boxes, scores, fr, ab                                # video 2 class 0 and video 0 class 1: all empty


def test_chains_stop_at_video_boundaries_and_empty_slots():
    from vdetlib_amd import ops
    off, boxes, scores, fr, ab = boundary_case()
    tb, ts, tf, ta = g(boxes), g(scores), g(fr), g(ab)
    out = ops.track_from_anchors_batch(tb, off, tf, ta)
    det, best = ops.anchor_propagate_tracks_batch(out, tb, ts)
    check_batch(out, det, best, per_video(tb, ts, off, tf, ta, None))
    rows = [(~np.isnan(n_(t)[..., 0])).sum(-1) for t in out['tracks']]
    assert rows[0].tolist() == [[3, 0, 0], [0, 0, 0]]                # back to the video's first frame, not beyond its last
    assert rows[1].tolist() == [[0, 1, 0], [0, 0, 0]]
    assert rows[2].tolist() == [[0, 0, 0], [4, 0, 4]]                # forward to the video's last frame
    assert n_(out['ntracks']).tolist() == [[1, 0], [2, 0], [0, 3]]
    assert n_(best)[0, 0, 0] == 2 and n_(best)[2, 1, 2] == 2 and n_(best)[0, 1].tolist() == [-1, -1, -1]
    # max_frames cuts the chain inside the video
    cut = ops.track_from_anchors_batch(tb, off, tf, ta, max_frames=3)
    assert (~np.isnan(n_(cut['tracks'][2])[1, 0, :, 0])).sum() == 2
    # a whole batch of empty slots
    none = ops.track_from_anchors_batch(tb, off, g(np.zeros_like(fr)), ta)
    assert all(np.isnan(n_(t)).all() for t in none['tracks']) and not n_(none['ntracks']).any()


def test_anchor_frame_beyond_its_video_is_latched():
    from vdetlib_amd import _lib, ops
    off, boxes, scores, fr, ab = boundary_case()
    bad = fr.copy()
    bad[1, 1, 0] = 2                                                # F_v + 1 of the one-frame video (a valid frame of the volume)
    ab[1, 1, 0] = boxes[4, 2]
    tb, ts = g(boxes), g(scores)
    cx = _lib.Context()
    try:
        with pytest.raises(ValueError):
            ops.track_from_anchors_batch(tb, off, g(bad), g(ab), ctx=cx)
        out = ops.track_from_anchors_batch(tb, off, g(bad), g(ab), sync=False, ctx=cx)
        with pytest.raises(ValueError):
            cx.sync()
        good = ops.track_from_anchors_batch(tb, off, g(fr), g(ab), ctx=cx)
        assert np.isnan(n_(out['tracks'][1])[1, 0]).all()            # written as an empty slot
        for v in range(3):
            assert same(n_(out['tracks'][v]), n_(good['tracks'][v]))  # every other slot is still correct
        assert n_(out['ntracks']).tolist() == n_(good['ntracks']).tolist()
    finally:
        cx.close()


def test_batch_route_feeds_the_consumers():
    from vdetlib_amd import eval as vev, ops
    from vdetlib_amd.vdet.tcn import TCNNet
    import torch
    off, C, T, B = [0, 3, 4, 9], 2, 3, 70
    F = off[-1]
    V = len(off) - 1
    boxes, scores = coherent_video(8300, F, B, C)
    tb, ts = g(boxes), g(scores)
    fr, ab, sc, _ = ops.top_anchors(tb, ts, T, frame_off=off)
    out = ops.track_from_anchors_batch(tb, off, fr, ab, sc)
    det, best = ops.anchor_propagate_tracks_batch(out, tb, ts)
    singles = per_video(tb, ts, off, fr, ab, sc)
    names = ['v%d' % v for v in range(V)]
    annots = [{'video': names[v], 'annotations': [{'id': '0', 'track': [
        {'frame': f + 1, 'bbox': [int(x) for x in n_(singles[v][0])[0, 0, f, :4]], 'class_index': 1, 'class': 'c1'}
        for f in range(off[v + 1] - off[v]) if not np.isnan(n_(singles[v][0])[0, 0, f, 0])]}]} for v in range(V)]
    gt = vev.gt_table_from_annots(annots)
    # the TCN on the propagated scores
    net = TCNNet.random([(n, 1) for n in ('det_scores', 'track_scores', 'anchors', 'abs_anchors')], hidden=(8,), kernel=3, seed=3)
    conv = ops.tcn_tracks_batch(net, out, series='det')
    for v, (tr, an, nt, d1, _) in enumerate(singles):
        assert same(n_(conv[v]), n_(ops.tcn_tracks(net, tr, nt, an, d1)))
    # overlap with the ground truth
    ev = ops.DetEvaluator(gt, classes=[1, 2])
    _, views, mean, flag = ops.tubelets_overlap_batch(ev, names, out)
    for v, (tr, an, nt, _, _) in enumerate(singles):
        ov1, m1, f1 = ops.tubelets_overlap(ev, names[v], tr, nt)
        assert same(n_(views[v]), n_(ov1)) and same(n_(mean[v]), n_(m1)) and same(n_(flag[v]), n_(f1))
    # interpolation (identity frames: every frame is a knot)
    dense = ops.interpolate_tracks_batch(out, None, [off[v + 1] - off[v] for v in range(V)])
    for v, (tr, an, nt, _, _) in enumerate(singles):
        one = ops.interpolate_tracks(tr, nt, an, ())
        assert same(n_(dense['tracks'][v]), n_(one['tracks'])) and same(n_(dense['anchors'][v]), n_(one['anchors']))
    # the evaluator: add_batch reads the score series as 'pooled' and the boxes as 'tboxes' (the tracks' own boxes here)
    tbx = torch.cat([t[..., :4].reshape(-1) for t in out['tracks']])
    feed = dict(out, pooled=out['det'],
                tboxes=[tbx[C * T * 4 * off[v]: C * T * 4 * off[v + 1]].view(C, T, off[v + 1] - off[v], 4) for v in range(V)])
    eb = ops.DetEvaluator(gt, classes=[1, 2])
    n_batch = eb.add_batch(names, feed)
    e1 = ops.DetEvaluator(gt, classes=[1, 2])
    n_single = sum(e1.add_tracks(names[v], s[0], s[2], scores=s[3]) for v, s in enumerate(singles))
    assert n_batch == n_single > 0
    (ab_, mb), (a1, m1) = eb.compute(), e1.compute()
    assert sorted(ab_) == sorted(a1) and all(ab_[k] == a1[k] or (ab_[k] != ab_[k] and a1[k] != a1[k]) for k in a1)
    assert mb == m1 or (mb != mb and m1 != m1)


def test_end_to_end_against_the_dict_route(oracle):
    """protocol.top_detections -> track_from_det (a Python IoU-link plug-in: the oracle's rows) -> anchor_propagate on
    dicts, against top_anchors -> track_from_anchors -> anchor_propagate_tracks on one 6-frame, 8-box, 2-class video."""
    from vdetlib_amd import ops
    from vdetlib_amd.utils import protocol
    from vdetlib_amd.vdet import track as vtrack, tubelet_cls
    F, B, T = 6, 8, 8                    # (top_num = B*F would return the proto unsorted: stay below)
    name = 'e2e_vid'
    vid = synth.make_vid_proto(name, F)
    det = synth.make_det_proto(8400, name, F, B, ['__background__', 'airplane', 'antelope'])
    dets = det['detections']
    boxes = np.array([d['bbox'] for d in dets], np.float32).reshape(F, B, 4)
    scores = np.array([[s['score'] for s in d['scores']] for d in dets], np.float32).reshape(F, B, 3)
    tb, ts = g(boxes), g(scores)

    def iou_link(vid_proto, d):
        rows = oracle.iou_link_rows_box(boxes, d['frame'] - 1, np.asarray(d['bbox'], np.float32), 0.5, 0)
        return [[{'frame': f + 1, 'bbox': [float(x) for x in rows[f, :4]], 'score': float(rows[f, 4]), 'anchor': f + 1 - d['frame']}
                 for f in range(F) if not np.isnan(rows[f, 0])]]
    fr, ab, sc, ix = ops.top_anchors(tb, ts, T)
    tracks, anchors, nt = ops.track_from_anchors(tb, fr, ab, sc)
    dscore, _ = ops.anchor_propagate_tracks(tracks, nt, anchors, tb, ts)
    tracks, dscore, fr_h = n_(tracks), n_(dscore), n_(fr)
    for c in (1, 2):
        top = protocol.top_detections(det, T, c)
        assert [d['frame'] for d in top['detections']] == fr_h[c].tolist()
        tp = vtrack.track_from_det(vid, top, iou_link)
        # (anchor_propagate reads the score list BY POSITION class_idx - 1, top_detections by the class_index key:
        #  position c of this proto's score lists is class_index c)
        score_proto = tubelet_cls.anchor_propagate(vid, tp, det, c + 1)
        assert len(score_proto['tubelets']) == T
        for t, tub in enumerate(score_proto['tubelets']):
            has = ~np.isnan(tracks[c, t, :, 0])
            assert [b['frame'] for b in tub['boxes']] == (np.nonzero(has)[0] + 1).tolist()
            for b in tub['boxes']:
                f = b['frame'] - 1
                assert b['bbox'] == tracks[c, t, f, :4].tolist()                      # boxes exactly
                assert abs(b['track_score'] - float(tracks[c, t, f, 4])) <= 1e-5
                assert abs(b['det_score'] - dscore[c, t, f]) <= 1e-5


def test_same_offsets_stage_the_table_once():
    from vdetlib_amd import _lib, ops
    off, boxes, scores, fr, ab = boundary_case()
    tb, ts, tf, ta = g(boxes), g(scores), g(fr), g(ab)
    cx = _lib.Context()
    try:
        n0 = cx.query(11)
        out = ops.track_from_anchors_batch(tb, off, tf, ta, ctx=cx)
        assert cx.query(11) == n0 + 1
        before = cx.query(8)
        for _ in range(3):
            sel = ops.top_anchors(tb, ts, 3, frame_off=off, sync=False, ctx=cx)
            out = ops.track_from_anchors_batch(tb, off, tf, ta, sync=False, ctx=cx)
            ops.anchor_propagate_tracks_batch(out, tb, ts, sync=False, ctx=cx)
        assert cx.query(11) == n0 + 1 and cx.query(8) == before       # neither a copy nor a wait
        cx.sync()
        ops.track_from_anchors_batch(tb, [0, 4, 8], tf[:2], ta[:2], ctx=cx)
        assert cx.query(11) == n0 + 2                                 # other offsets: staged again
        assert tuple(sel[0].shape) == (3, 2, 3)
    finally:
        cx.close()


# ---- video_batch's layout: one reader for every consumer (ops._batch_read / _batch_field / _batch_views) -----------------------
def small_batch():
    """videos of 1, 2 and 3 frames, B = 8, C = 2, T = 2: (offsets, boxes, scores, video_batch's dict, names, gt table)"""
    from vdetlib_amd import eval as vev, ops
    off, B, C, T = [0, 1, 3, 6], 8, 2, 2
    boxes, scores = coherent_video(8500, off[-1], B, C)
    tb, ts = g(boxes), g(scores)
    vb = ops.video_batch(tb, ts, off, max_tracks=T)
    names = ['v%d' % v for v in range(3)]
    annots = [{'video': names[v], 'annotations': [{'id': '0', 'track': [
        {'frame': f + 1, 'bbox': [int(x) for x in n_(vb['tracks'][v])[0, 0, f, :4]], 'class_index': 1, 'class': 'c1'}
        for f in range(off[v + 1] - off[v]) if not np.isnan(n_(vb['tracks'][v])[0, 0, f, 0])]}]} for v in range(3)]
    return off, tb, ts, vb, names, vev.gt_table_from_annots(annots)


def one_allocation(d, keys):
    from vdetlib_amd import ops
    for k in keys:
        assert ops._batch_flat(d[k], 1).data_ptr() == d[k][0].data_ptr(), k
        assert len({x.untyped_storage().data_ptr() for x in d[k]}) == 1, k


def test_per_video_clones_are_refused_on_the_host():
    """per-video tensors of their own allocations are not the layout: the kernels would index past the first of them"""
    from vdetlib_amd import ops
    off, tb, ts, vb, names, gt = small_batch()
    apart = lambda d, k: dict(d, **{k: [x.clone() for x in d[k]]})
    ev = ops.DetEvaluator(gt, classes=[1, 2])
    assert ev.add_batch(names, vb) > 0
    dets = ops.nms_tracks_batch(vb, 'pooled')
    assert ev.add_detections(names, dets) > 0
    n = ev.stream()[0].numel()
    calls = [lambda: ev.add_batch(names, apart(vb, 'pooled')), lambda: ev.add_batch(names, apart(vb, 'tboxes')),
             lambda: ev.add_batch(names, apart(vb, 'tracks')),
             lambda: ev.add_detections(names, apart(dets, 'score')), lambda: ev.add_detections(names, apart(dets, 'tracks')),
             lambda: ops.tubelets_overlap_batch(ev, names, apart(vb, 'tracks')),
             lambda: ops.tubelets_overlap_batch(ev, names, apart(vb, 'tboxes'), use_tboxes=True),
             lambda: ops.anchor_propagate_tracks_batch(apart(vb, 'tracks'), tb, ts)]
    for i, call in enumerate(calls):
        with pytest.raises(ValueError, match="consecutive"):
            call()
        assert ev.stream()[0].numel() == n, i
    assert ev.add_batch(names, vb) > 0 and ev.stream()[0].numel() > n           # the evaluator still works


def test_chain_of_batch_stages_equals_the_single_video_calls():
    """video_batch -> rescore_tubelets_batch -> merge_tracks_batch -> nms_tracks_batch -> add_detections: every stage hands on
    a dict the reader accepts, every field one allocation, per video the bits of the single-video calls"""
    import torch
    from vdetlib_amd import ops
    off, tb, ts, vb, names, gt = small_batch()
    rs = ops.rescore_tubelets_batch(vb, tb, ts)
    mg = ops.merge_tracks_batch(rs, rs, 'combine')
    dets = ops.nms_tracks_batch(mg, 'pooled')
    for d, keys in ((vb, ('tracks', 'det', 'pooled', 'tboxes')), (rs, ('tracks', 'det', 'pooled', 'tboxes', 'src')),
                    (mg, ('tracks', 'det', 'pooled', 'tboxes')), (dets, ('tracks', 'score', 'src'))):
        b = ops._batch_read(d, need=('anchors',) if d is not dets else ())
        assert b.V == 3 and b.Ft == 6 and b.tracks.data_ptr() == d['tracks'][0].data_ptr()
        one_allocation(d, keys)
    assert 'src' not in vb and rs['tracks'][0] is vb['tracks'][0]                # a new dict; the input is left alone
    eb, e1 = ops.DetEvaluator(gt, classes=[1, 2]), ops.DetEvaluator(gt, classes=[1, 2])
    for v in range(3):
        sl = slice(off[v], off[v + 1])
        tr, nt, an = vb['tracks'][v], vb['ntracks'][v], vb['anchors'][v]
        single = ops.rescore_tubelets(tr, nt, tb[sl], ts[sl])
        for k, x in zip(('det', 'pooled', 'tboxes', 'src'), single):
            assert same(n_(rs[k][v]), n_(x)), (v, k)
        a = dict(tracks=tr, ntracks=nt, anchors=an, series=single[:2], tboxes=single[2])
        m1 = ops.merge_tracks(a, a, 'combine')
        for k, x in (('tracks', m1['tracks']), ('det', m1['series'][0]), ('pooled', m1['series'][1]), ('tboxes', m1['tboxes']),
                     ('anchors', m1['anchors']), ('ntracks', m1['ntracks'])):
            assert same(n_(mg[k][v]), n_(x)), (v, k)
        d1 = ops.nms_tracks(m1, score=1)
        for k in ('tracks', 'score', 'src', 'ntracks'):
            assert same(n_(dets[k][v]), n_(d1[k])), (v, k)
        assert same(n_(dets['cnt'][:, sl]), n_(d1['cnt'])), v
        e1.add_detections(names[v], d1)
    assert eb.add_detections(names, dets) == e1.stream()[0].numel() > 0
    for x, y in zip(eb.stream(raw=True), e1.stream(raw=True)):
        assert torch.equal(x, y)
