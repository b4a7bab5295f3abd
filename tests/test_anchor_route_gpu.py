"""-m gpu: the device anchor route (ops.track_from_anchors, ops.anchor_propagate_tracks, csrc/anchor_kernels.hpp; the
dict-level anchor_propagate through hot.anchor_argmax) against
  1. oracle.iou_link_rows_box per slot, bit for bit (anchors at both ends, in the middle, fractional, empty slots);
  2. tie and NaN rules of a link step;
  3. the greedy tracker's own tubelets from its own anchors, below and above its 1 024-box link-table limit, leaving the
     context's cached state as it was;
  4. a loop of oracle.iou + np.argmax + broadcast for the propagation;
  5. the consumers of the [C,T,F,...] layout;  6. the dict API;  7. argument errors;  8. no host wait.
Every comparison is exact: oracle and kernels do the same f32 / f64 operations in the same order.
The link kernel has ONE path for every size (a step scans the whole frame), so there is no fallback switch to compare with."""
import numpy as np
import pytest

import synth

pytestmark = pytest.mark.gpu


def same(a, b):
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def g(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def link(boxes, frames, aboxes, ascores=None, **kw):
    from vdetlib_amd import ops
    out = ops.track_from_anchors(g(boxes), g(frames), g(aboxes), None if ascores is None else g(ascores), **kw)
    return tuple(x.cpu().numpy() for x in out)


def want_link(oracle, boxes, frames, aboxes, link_thres, max_frames):
    C, T = frames.shape
    F = boxes.shape[0]
    tracks = np.full((C, T, F, 5), np.nan, np.float32)
    nt = np.zeros(C, np.int32)
    for c in range(C):
        for t in range(T):
            if frames[c, t] >= 1:
                tracks[c, t] = oracle.iou_link_rows_box(boxes, int(frames[c, t]) - 1, np.trunc(aboxes[c, t]), link_thres, max_frames)
                nt[c] = t + 1
    return tracks, nt


# ---------------------------------------------------------------------------------------------------------------------
# 1. link vs oracle, small
# ---------------------------------------------------------------------------------------------------------------------
F1, B1 = 7, 70
OBJ_A = np.array([300, 200, 420, 330], np.float32)
OBJ_B = np.array([700.4, 100.7, 990.2, 560.9], np.float32)


def small_video():
    """7 frames x 70 boxes (one full wave plus a tail): noise boxes (fractional on the odd frames) and two planted objects
    drifting 3 px per frame, A at index 11 + f, B (fractional) at index 65 in the tail."""
    rng = np.random.RandomState(7101)
    boxes = np.stack([synth.boxes_1(rng, B1, frac=(f % 2 == 1)) for f in range(F1)], 0)
    for f in range(F1):
        boxes[f, 11 + f] = OBJ_A + np.float32(3 * f)
        boxes[f, 65] = OBJ_B + np.float32(3 * f)
    return boxes.astype(np.float32)


def small_anchors():
    frames = np.array([[1, 0, F1],            # first frame | an EMPTY slot below the last live one | last frame
                       [4, 3, 0]], np.int32)  # the middle | fractional coordinates | a slot above the class's last live slot
    ab = np.zeros((2, 3, 4), np.float32)
    ab[0, 0] = OBJ_A
    ab[0, 1] = [1, 2, 3, 4]                   # (ignored: the slot is empty)
    ab[0, 2] = OBJ_A + 3 * (F1 - 1)
    ab[1, 0] = np.trunc(OBJ_B + 9)
    ab[1, 1] = OBJ_A + 6 + np.array([0.7, 0.9, 0.2, 0.6], np.float32)
    sc = np.array([[0.9, 0.1, 0.8], [0.7, 0.6, 0.5]], np.float32)
    return frames, ab, sc


@pytest.mark.parametrize("link_thres", (0.5, 0.9))
@pytest.mark.parametrize("max_frames", (0, 4, 5))
def test_link_equals_oracle_small(oracle, max_frames, link_thres):
    boxes = small_video()
    frames, ab, sc = small_anchors()
    tracks, anchors, nt = link(boxes, frames, ab, sc, link_thres=link_thres, max_frames=max_frames)
    wt, wnt = want_link(oracle, boxes, frames, ab, link_thres, max_frames)
    assert tracks.dtype == np.float32 and anchors.dtype == np.float32 and nt.dtype == np.int32
    for c in range(2):
        for t in range(3):
            assert same(tracks[c, t], wt[c, t]), (c, t, tracks[c, t], wt[c, t])
    assert nt.tolist() == wnt.tolist() == [3, 2]
    assert np.isnan(tracks[0, 1]).all() and np.isnan(tracks[1, 2]).all()
    want_an = np.stack([frames.astype(np.float32), np.full((2, 3), -1, np.float32), sc], -1)
    assert same(anchors, want_an)
    # the anchors really link (the comparison above is not NaN against NaN) and max_frames cuts the reach
    n_rows = (~np.isnan(tracks[..., 0])).sum(-1)
    reach = F1 if max_frames == 0 else int(np.ceil((max_frames + 1) / 2.)) - 1
    assert n_rows[0, 0] == min(F1, 1 + reach) and n_rows[0, 2] == min(F1, 1 + reach) and n_rows[1, 0] == min(F1, 1 + 2 * reach)
    assert n_rows[1, 1] == min(F1, 1 + min(reach, 2) + min(reach, 4))
    assert np.array_equal(tracks[1, 1, 2], np.append(np.trunc(ab[1, 1]), np.float32(1)))       # the truncated anchor


def test_link_without_scores_single_class(oracle):
    boxes = small_video()
    frames, ab, _ = small_anchors()
    frames, ab = frames.reshape(1, 6), ab.reshape(1, 6, 4)
    tracks, anchors, nt = link(boxes, frames, ab)
    wt, wnt = want_link(oracle, boxes, frames, ab, 0.5, 0)
    assert same(tracks, wt) and nt.tolist() == wnt.tolist() == [5]
    assert same(anchors, np.stack([frames.astype(np.float32), np.full((1, 6), -1, np.float32), np.zeros((1, 6), np.float32)], -1))


# ---------------------------------------------------------------------------------------------------------------------
# 2. ties and NaN
# ---------------------------------------------------------------------------------------------------------------------
CUR = np.array([100, 100, 199, 199], np.float32)
RIGHT, LEFT = CUR + np.array([2, 0, 2, 0], np.float32), CUR - np.array([2, 0, 2, 0], np.float32)    # the same IoU bits with CUR


def far_video(F, B, seed):
    """noise boxes that do not touch the 100..260 square the cases below play in"""
    rng = np.random.RandomState(seed)
    b = np.stack([synth.boxes_1(rng, B) for _ in range(F)], 0)
    return (b + np.array([400, 300, 400, 300], np.float32)).astype(np.float32)


@pytest.mark.parametrize("B,i,j", [(70, 5, 40), (70, 5, 69), (1030, 3, 1027)])
@pytest.mark.parametrize("first", ("right", "left"))
def test_tie_goes_to_the_lowest_index(oracle, B, i, j, first):
    boxes = far_video(4, B, 7200 + B)
    a, b = (RIGHT, LEFT) if first == "right" else (LEFT, RIGHT)
    boxes[1, i], boxes[1, j] = a, b
    boxes[2, j], boxes[2, i] = a + 1, b + 1       # what follows either winner: the chains differ from here on
    ious = oracle._iou_f32_row(CUR, boxes[1, [i, j]])
    assert ious[0] == ious[1] >= 0.9               # a true tie, bit for bit
    frames = np.array([[1]], np.int32)
    tracks, _, _ = link(boxes, frames, CUR.reshape(1, 1, 4))
    want = oracle.iou_link_rows_box(boxes, 0, CUR, 0.5, 0)
    assert same(tracks[0, 0], want)
    assert np.array_equal(tracks[0, 0, 1, :4], a) and np.array_equal(tracks[0, 0, 2, :4], a + 1)
    # ... and backward, from the last frame
    rev = boxes[::-1].copy()
    tracks, _, _ = link(rev, np.array([[4]], np.int32), CUR.reshape(1, 1, 4))
    assert same(tracks[0, 0], oracle.iou_link_rows_box(rev, 3, CUR, 0.5, 0))
    assert np.array_equal(tracks[0, 0, 2, :4], a)


def test_nan_boxes_are_out_of_the_running(oracle):
    B = 70
    boxes = far_video(4, B, 7301)
    boxes[1, 0] = np.nan                            # NaN boxes in front of, and behind, the match
    boxes[1, 7, 2] = np.nan                         # one NaN coordinate
    boxes[1, 33] = RIGHT
    boxes[1, 68] = np.nan
    boxes[2, 64] = RIGHT + 2
    boxes[3, 2] = RIGHT + 4
    tracks, _, _ = link(boxes, np.array([[1]], np.int32), CUR.reshape(1, 1, 4))
    assert same(tracks[0, 0], oracle.iou_link_rows_box(boxes, 0, CUR, 0.5, 0))
    assert np.array_equal(tracks[0, 0, :, :4], np.stack([CUR, RIGHT, RIGHT + 2, RIGHT + 4]))
    # a frame of NaN boxes only: the chain stops, the good match behind it is not reached
    boxes[2] = np.nan
    tracks, _, _ = link(boxes, np.array([[1]], np.int32), CUR.reshape(1, 1, 4))
    assert same(tracks[0, 0], oracle.iou_link_rows_box(boxes, 0, CUR, 0.5, 0))
    assert not np.isnan(tracks[0, 0, 1]).any() and np.isnan(tracks[0, 0, 2:]).all()
    # a NaN anchor box: its row is (NaN box, 1), nothing links
    tracks, _, nt = link(boxes, np.array([[2]], np.int32), np.full((1, 1, 4), np.nan, np.float32))
    assert same(tracks[0, 0], oracle.iou_link_rows_box(boxes, 1, np.full(4, np.nan, np.float32), 0.5, 0))
    assert nt.tolist() == [1] and tracks[0, 0, 1, 4] == 1 and np.isnan(tracks[0, 0, [0, 2, 3]]).all()


def test_iou_equal_to_the_threshold_links(oracle):
    boxes = far_video(3, 70, 7302)
    cur = np.array([100, 100, 109, 109], np.float32)           # 10 x 10
    half = np.array([100, 100, 109, 119], np.float32)          # 10 x 20 around it: IoU = 100 / 200
    boxes[1, 66] = half
    boxes[2, 1] = np.array([100, 100, 109, 139], np.float32)   # 10 x 40: IoU with `half` = 200 / 400
    assert oracle._iou_f32_row(cur, boxes[1, 66:67])[0] == np.float32(0.5)
    tracks, _, _ = link(boxes, np.array([[1]], np.int32), cur.reshape(1, 1, 4), link_thres=0.5)
    assert same(tracks[0, 0], oracle.iou_link_rows_box(boxes, 0, cur, 0.5, 0))
    assert np.array_equal(tracks[0, 0, 1], np.append(half, np.float32(0.5))) and tracks[0, 0, 2, 4] == np.float32(0.5)
    above = float(np.nextafter(np.float32(0.5), np.float32(1)))
    tracks, _, _ = link(boxes, np.array([[1]], np.int32), cur.reshape(1, 1, 4), link_thres=above)
    assert same(tracks[0, 0], oracle.iou_link_rows_box(boxes, 0, cur, above, 0)) and np.isnan(tracks[0, 0, 1:]).all()


# ---------------------------------------------------------------------------------------------------------------------
# 3. against the greedy tracker (shared by 4 and 5)
# ---------------------------------------------------------------------------------------------------------------------
FG, CG, TG = 30, 4, 5
_greedy = {}


def greedy_case(B):
    """nms_track_volume on a cache-enabled context, then track_from_anchors of ITS anchors on the same context, then
    nms_track_volume again"""
    if B not in _greedy:
        import torch
        from vdetlib_amd import _lib, ops
        boxes, scores = synth.coherent_video(7400 + B, FG, B, CG, frac=True)
        tb, ts = g(boxes), g(scores)
        cx = _lib.Context(torch.cuda.current_device())
        try:
            cx.set_cache(True)
            run = lambda: tuple(x.cpu().numpy() for x in ops.nms_track_volume(tb, ts, max_tracks=TG, ctx=cx))
            first = run()
            _, _, tr, an, nt = first
            live = np.arange(TG)[None, :] < nt[:, None]
            frames = np.where(live, an[..., 0], 0).astype(np.int32)
            idx = np.where(live, an[..., 1], 0).astype(np.int64)
            ab = np.where(live[..., None], boxes[np.maximum(frames - 1, 0), idx], 0).astype(np.float32)
            sc = np.where(live, an[..., 2], 0).astype(np.float32)
            mine = ops.track_from_anchors(tb, g(frames), g(ab), g(sc), ctx=cx)
            second = run()
        finally:
            cx.close()
        _greedy[B] = dict(boxes=boxes, scores=scores, tb=tb, ts=ts, first=first, second=second, frames=frames, ab=ab, sc=sc,
                          live=live, mine=mine)
    return _greedy[B]


@pytest.mark.parametrize("B", (300, 1100))           # above 1 024 boxes the greedy side scans its link steps on demand
def test_equals_the_greedy_tracker_from_its_own_anchors(B):
    k = greedy_case(B)
    _, _, tr, an, nt = k['first']
    mt, ma, mnt = (x.cpu().numpy() for x in k['mine'])
    assert nt.min() >= 1 and mnt.tolist() == nt.tolist()
    for c in range(CG):
        for t in range(int(nt[c])):
            assert same(mt[c, t], tr[c, t]), (c, t)
            assert ma[c, t, 0] == an[c, t, 0] and ma[c, t, 1] == -1 and ma[c, t, 2] == an[c, t, 2]
        assert np.isnan(mt[c, int(nt[c]):]).all()
    assert (~np.isnan(mt[..., 0])).sum() > 4 * int(nt.sum())          # tubelets, not lone anchors
    for a, b in zip(k['first'], k['second']):                          # the context's cached state was left alone
        assert same(a, b)


# ---------------------------------------------------------------------------------------------------------------------
# 4. propagation
# ---------------------------------------------------------------------------------------------------------------------
def want_propagate(oracle, tracks, nt, anchors, boxes, scores):
    C, T, F = tracks.shape[:3]
    det = np.full((C, T, F), np.nan, np.float64)
    best = np.full((C, T), -1, np.int32)
    for c in range(C):
        for t in range(min(int(nt[c]), T)):
            fa = int(anchors[c, t, 0])
            if fa < 1 or np.isnan(tracks[c, t, fa - 1, 0]):
                continue
            ov = oracle.iou(tracks[c, t, fa - 1, :4].astype(np.float64)[None], boxes[fa - 1].astype(np.float64))[0]
            best[c, t] = int(np.argmax(ov))
            det[c, t, ~np.isnan(tracks[c, t, :, 0])] = np.float64(scores[fa - 1, best[c, t], c])
    return det, best


def propagate(tracks, nt, anchors, boxes, scores, **kw):
    from vdetlib_amd import ops
    det, best = ops.anchor_propagate_tracks(g(tracks), g(nt), g(anchors), g(boxes), g(scores), **kw)
    return det.cpu().numpy(), best.cpu().numpy()


def test_propagate_small_tubelets(oracle):
    boxes = small_video()
    scores = np.random.RandomState(7501).rand(F1, B1, 2).astype(np.float32)
    frames, ab, sc = small_anchors()
    tracks, anchors, nt = link(boxes, frames, ab, sc, max_frames=5)
    det, best = propagate(tracks, nt, anchors, boxes, scores)
    wd, wb = want_propagate(oracle, tracks, nt, anchors, boxes, scores)
    assert det.dtype == np.float64 and best.dtype == np.int32
    assert same(det, wd) and same(best, wb)
    assert best[0, 0] == 11 and best[0, 2] == 11 + F1 - 1 and best[1, 0] == 65 and best[0, 1] == -1 and best[1, 2] == -1
    assert np.array_equal(np.isnan(det), np.isnan(tracks[..., 0]))


@pytest.mark.parametrize("B", (300, 1100))
def test_propagate_greedy_tubelets(oracle, B):
    from vdetlib_amd import ops
    k = greedy_case(B)
    _, _, tr, an, nt = k['first']
    mt, ma, mnt = k['mine']
    wd, wb = want_propagate(oracle, tr, nt, an, k['boxes'], k['scores'])
    for tracks, anchors, ntr in ((g(tr), g(an), g(nt)), (mt, ma, mnt)):      # the greedy call's layout and this route's
        det, best = ops.anchor_propagate_tracks(tracks, ntr, anchors, k['tb'], k['ts'])
        assert same(det.cpu().numpy(), wd) and same(best.cpu().numpy(), wb)
    assert (wb[k['live']] >= 0).all() and not np.isnan(wd).all()


def test_propagate_argmax_rules(oracle):
    """hand-made tubelets: duplicate detections, NaN boxes, a zero union, a NaN anchor row, t >= ntracks"""
    F, B, C, T = 4, 70, 2, 4
    rng = np.random.RandomState(7502)
    boxes = np.stack([synth.boxes_1(rng, B, frac=True) for _ in range(F)], 0)
    scores = rng.rand(F, B, C).astype(np.float32)
    tracks = np.full((C, T, F, 5), np.nan, np.float32)
    anchors = np.zeros((C, T, 3), np.float32)
    nt = np.array([4, 2], np.int32)
    box = np.array([50.5, 60.25, 140.5, 170.75], np.float32)
    # (0,0) anchor frame 2: the anchor box itself sits at 66 and again at 9 -> 9; rows on frames 1, 2, 4
    boxes[1, 66] = box; boxes[1, 9] = box
    tracks[0, 0, [0, 1, 3]] = np.append(box, 0.5); anchors[0, 0] = [2, -1, 0.3]
    # (0,1) anchor frame 3: NaN boxes at 68 and 4 beat the exact copy at 1 -> 4 (the first NaN)
    boxes[2, 1] = box; boxes[2, 68] = np.nan; boxes[2, 4, 3] = np.nan
    tracks[0, 1, 2] = np.append(box, 1.0); anchors[0, 1] = [3, -1, 0.0]
    # (0,2) anchor frame 1: a zero-area anchor box against a zero-area detection: 0 / 0 = NaN at 5, no error
    flat = np.array([10, 10, 9, 20], np.float32)
    boxes[0, 5] = np.array([50, 50, 49, 60], np.float32)
    tracks[0, 2, 0] = np.append(flat, 1.0); tracks[0, 2, 1] = np.append(box, 0.7); anchors[0, 2] = [1, -1, 0.0]
    # (0,3) a live slot whose anchor row is NaN (rows elsewhere)
    tracks[0, 3, 0] = np.append(box, 0.7); anchors[0, 3] = [4, -1, 0.0]
    # (1,0) a dead slot below ntracks; (1,1) plain, frame 4; (1,2) t >= ntracks with rows and an anchor
    tracks[1, 1, 3] = np.append(boxes[3, 30], 1.0); anchors[1, 1] = [4, -1, 0.0]
    tracks[1, 2, :] = np.append(box, 1.0); anchors[1, 2] = [1, -1, 0.0]
    wd, wb = want_propagate(oracle, tracks, nt, anchors, boxes, scores)
    assert wb.tolist() == [[9, 4, 5, -1], [-1, 30, -1, -1]]
    assert np.isnan(oracle.iou(flat[None].astype(np.float64), boxes[0, 5:6].astype(np.float64))[0, 0])
    det, best = propagate(tracks, nt, anchors, boxes, scores)
    assert same(best, wb) and same(det, wd)
    assert det[0, 0, 0] == np.float64(scores[1, 9, 0]) and np.isnan(det[0, 0, 2]) and np.isnan(det[0, 3]).all() and np.isnan(det[1, 2]).all()
    # (the call waited for the device and raised nothing: a zero union is not an error here)


# ---------------------------------------------------------------------------------------------------------------------
# 5. into the consumers
# ---------------------------------------------------------------------------------------------------------------------
def test_chain_into_the_consumers():
    from vdetlib_amd import eval as vev, ops
    from vdetlib_amd.vdet.tcn import TCNNet
    k = greedy_case(300)
    tr, an, nt = k['mine']
    has = ~np.isnan(tr[..., 0].cpu().numpy())
    det, pooled, ob = ops.rescore_tracks(tr, nt, k['tb'], k['ts'], overlap_thres=0.7, window=3)
    assert tuple(pooled.shape) == (CG, TG, FG) and tuple(ob.shape) == (CG, TG, FG, 4)
    prop, _ = ops.anchor_propagate_tracks(tr, nt, an, k['tb'], k['ts'])
    annot = {'video': 'anchor_vid', 'annotations': [{'id': '0', 'track': [
        {'frame': f + 1, 'bbox': [int(v) for v in tr[0, 0, f, :4].cpu().numpy()], 'class_index': 1, 'class': 'c1'}
        for f in range(FG) if has[0, 0, f]]}]}
    for series in (pooled, prop):                  # (a video is added to an evaluator once: one evaluator per score series)
        ev = ops.DetEvaluator(vev.gt_table_from_annots([annot]), classes=[1, 2, 3, 4])
        assert ev.add_tracks('anchor_vid', tr, nt, scores=series) == int(has.sum())
        aps, _ = ev.compute()
        assert 0.0 < max(v for v in aps.values() if v == v) <= 1.0
    net = TCNNet.random([(n, 1) for n in ('det_scores', 'track_scores', 'anchors', 'abs_anchors')], hidden=(8,), kernel=3, seed=3)
    conv = ops.tcn_tracks(net, tr, nt, an, prop)
    assert conv.dtype == __import__('torch').float32 and tuple(conv.shape) == (CG, TG, FG)
    assert np.array_equal(~np.isnan(conv.cpu().numpy()), has)


# ---------------------------------------------------------------------------------------------------------------------
# 6. dict API
# ---------------------------------------------------------------------------------------------------------------------
def test_dict_anchor_propagate_is_one_device_call(oracle, monkeypatch):
    from vdetlib.vdet import tubelet_cls as T
    from vdetlib_amd import hot
    name = 'dict_vid'
    rng = np.random.RandomState(7601)
    vid = synth.make_vid_proto(name, 3)
    dets, per_frame = [], {}
    for f in (1, 2, 3):
        bx = synth.boxes_1(rng, 9, frac=True).astype(np.float64)
        sc = rng.rand(9, 3)
        per_frame[f] = (bx, sc)
        for b, s in zip(bx, sc):
            dets.append({'frame': f, 'bbox': b.tolist(), 'scores': [{'class_index': i + 1, 'score': float(v)} for i, v in enumerate(s)]})
    det_proto = {'video': name, 'detections': dets}

    def tracklet(anchor_frame, base):
        return [{'frame': f, 'bbox': [int(v) for v in base + 2 * f], 'score': 0.5, 'anchor': f - anchor_frame, 'hash': str(f)}
                for f in (1, 2, 3)]
    track_proto = {'video': name, 'method': 'x', 'tracks': [tracklet(2, per_frame[2][0][4]), tracklet(3, per_frame[3][0][7])]}
    calls = []
    real = hot.anchor_argmax
    monkeypatch.setattr(hot, 'anchor_argmax', lambda *a, **k: (calls.append(len(a[0])), real(*a, **k))[1])
    out = T.anchor_propagate(vid, track_proto, det_proto, 2)
    assert calls == [2]                                         # both tubelets in ONE device call
    assert out['method'] == 'anchor_propagate' and len(out['tubelets']) == 2
    for tub, tr, fa in zip(out['tubelets'], track_proto['tracks'], (2, 3)):
        ab = [b['bbox'] for b in tr if b['anchor'] == 0]
        best = int(np.argmax(oracle.iou(np.asarray(ab, dtype=np.float64), per_frame[fa][0])[0]))
        assert [b['det_score'] for b in tub['boxes']] == [float(per_frame[fa][1][best, 1])] * 3


# ---------------------------------------------------------------------------------------------------------------------
# 7. errors, 8. no host wait
# ---------------------------------------------------------------------------------------------------------------------
def test_argument_errors_leave_the_context_usable(oracle):
    import torch
    from vdetlib_amd import ops
    boxes = small_video()
    frames, ab, sc = small_anchors()
    tb, tf, ta, ts = g(boxes), g(frames), g(ab), g(sc)
    bad = [lambda: ops.track_from_anchors(tb[:, :0], tf, ta),                           # B == 0
           lambda: ops.track_from_anchors(tb.double(), tf, ta),                         # f64 boxes
           lambda: ops.track_from_anchors(tb, tf.long(), ta),
           lambda: ops.track_from_anchors(tb, tf, ta.double()),
           lambda: ops.track_from_anchors(tb, tf, ta[:, :2]),                           # shape mismatches
           lambda: ops.track_from_anchors(tb, tf, ta, ts[:1]),
           lambda: ops.track_from_anchors(tb[..., :3], tf, ta),
           lambda: ops.track_from_anchors(tb, tf.reshape(-1), ta),
           lambda: ops.track_from_anchors(tb, tf.cpu(), ta),                            # device mismatch
           lambda: ops.track_from_anchors(tb, g(np.where(frames == 4, F1 + 1, frames).astype(np.int32)), ta),   # frame F + 1
           lambda: ops.track_from_anchors(tb, g(np.where(frames == 4, -1, frames).astype(np.int32)), ta)]
    for k, fn in enumerate(bad):
        with pytest.raises(ValueError):
            fn()
            pytest.fail("case %d raised nothing" % k)
    tracks, anchors, nt = ops.track_from_anchors(tb, tf, ta, ts)
    scores = g(np.random.RandomState(7701).rand(F1, B1, 2).astype(np.float32))
    bad = [lambda: ops.anchor_propagate_tracks(tracks.double(), nt, anchors, tb, scores),
           lambda: ops.anchor_propagate_tracks(tracks, nt.long(), anchors, tb, scores),
           lambda: ops.anchor_propagate_tracks(tracks, nt, anchors, tb[:3], scores),
           lambda: ops.anchor_propagate_tracks(tracks, nt, anchors, tb, scores[..., :1]),
           lambda: ops.anchor_propagate_tracks(tracks, nt, anchors[:, :2], tb, scores),
           lambda: ops.anchor_propagate_tracks(tracks, nt[:1], anchors, tb, scores),
           lambda: ops.anchor_propagate_tracks(tracks, nt, anchors, tb, scores.cpu()),
           lambda: ops.anchor_propagate_tracks(tracks, nt, torch.where(anchors == 4, F1 + 1.0, anchors.double()).float(), tb, scores)]
    for k, fn in enumerate(bad):
        with pytest.raises(ValueError):
            fn()
            pytest.fail("case %d raised nothing" % k)
    # ... and the context still works
    wt, wnt = want_link(oracle, boxes, frames, ab, 0.5, 0)
    tracks, anchors, nt = ops.track_from_anchors(tb, tf, ta, ts)
    assert same(tracks.cpu().numpy(), wt) and nt.cpu().numpy().tolist() == wnt.tolist()
    det, best = ops.anchor_propagate_tracks(tracks, nt, anchors, tb, scores)
    wd, wb = want_propagate(oracle, wt, wnt, anchors.cpu().numpy(), boxes, scores.cpu().numpy())
    assert same(det.cpu().numpy(), wd) and same(best.cpu().numpy(), wb)


def test_async_calls_never_wait_for_the_device(oracle):
    from vdetlib_amd import _lib, ops
    boxes = small_video()
    frames, ab, sc = small_anchors()
    tb, tf, ta, ts = g(boxes), g(frames), g(ab), g(sc)
    scores = np.random.RandomState(7801).rand(F1, B1, 2).astype(np.float32)
    tsc = g(scores)
    wt, wnt = want_link(oracle, boxes, frames, ab, 0.5, 0)
    cx = _lib.Context()
    try:
        cx.set_async(True)
        prop = lambda o, **kw: ops.anchor_propagate_tracks(o[0], o[2], o[1], tb, tsc, ctx=cx, **kw)
        first = ops.track_from_anchors(tb, tf, ta, ts, ctx=cx)
        p1 = prop(first)
        before = cx.query(8)
        again = ops.track_from_anchors(tb, tf, ta, ts, sync=False, ctx=cx)
        p2 = prop(again, sync=False)
        third = ops.track_from_anchors(tb, tf, ta, ts, sync=False, ctx=cx)
        p3 = prop(third, sync=False)
        assert cx.query(8) == before, "an asynchronous anchor-route call waited for the device"
        cx.sync()
        assert cx.query(8) == before + 1
        wd, wb = want_propagate(oracle, wt, wnt, first[1].cpu().numpy(), boxes, scores)
        for out, p in ((first, p1), (again, p2), (third, p3)):
            assert same(out[0].cpu().numpy(), wt) and out[2].cpu().numpy().tolist() == wnt.tolist()
            assert same(p[0].cpu().numpy(), wd) and same(p[1].cpu().numpy(), wb)
    finally:
        cx.close()
