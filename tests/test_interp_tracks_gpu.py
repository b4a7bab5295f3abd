"""-m gpu: device interpolation of strided / holey tubelets to dense frames (ops.interpolate_tracks[_batch],
csrc/interp_kernels.hpp) against
  1. oracle.tubelet_interpolation per slot, on the f64 bits (the f32 outputs: the f64 values rounded once);
  2. the reference's own recorded output (proto_golden['interpolation']) under test_pipeline_gpu.py's comparison;
  3. the dict path end to end on a strided video (tracks_to_proto + score_proto_interpolation + score_conv_cls +
     eval.evaluate), box fields and conv_score on the bits, APs < 1e-12;
  4. the batch form against the per-video form, and through tcn_tracks_batch / tubelets_overlap_batch / add_batch;
  5. no host wait;  6. argument errors.
The kernel has ONE path for every size (it keeps no knot list), so there is no fallback switch to compare with."""
import contextlib
import io
import math

import numpy as np
import pytest

import synth

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------------------------
# hand-built cases
# ---------------------------------------------------------------------------------------------------------------------
def build_case(name, seed, Fs, F, frames, knots, nt, C=2, T=4, f32_series=False, with_boxes=False, nan_series=None, nser=2,
               integer=False):
    """knots: {(c, t): rows with a box}.  Rows of slots t >= nt[c] listed in ``knots`` are filled too (they must come
    out NaN).  nan_series: (c, t, row) whose series 0 value is NaN."""
    rng = np.random.RandomState(seed)
    tracks = np.full((C, T, Fs, 5), np.nan, np.float32)
    boxes = (rng.uniform(0, 900, (C, T, Fs, 4)) if not integer else rng.randint(0, 900, (C, T, Fs, 4))).astype(np.float32)
    series = [rng.randn(C, T, Fs) for _ in range(nser)]
    anchors = np.zeros((C, T, 3), np.float32)
    for (c, t), rows in knots.items():
        rows = np.asarray(rows, dtype=np.int64)
        vals = rng.uniform(0, 900, (len(rows), 5)) if not integer else rng.randint(0, 900, (len(rows), 5))
        tracks[c, t, rows] = vals.astype(np.float32)
        tracks[c, t, rows, 4] = rng.rand(len(rows)).astype(np.float32)
        if len(rows):
            anchors[c, t] = [rows[len(rows) // 2] + 1, rng.randint(0, 50), rng.rand()]
    if nan_series is not None:
        series[0][nan_series] = np.nan
    if f32_series:
        series = [s.astype(np.float32) for s in series]
    return dict(name=name, Fs=Fs, F=F, frames=None if frames is None else np.asarray(frames, dtype=np.int64), knots=knots,
                nt=np.asarray(nt, dtype=np.int32), tracks=tracks, boxes=boxes if with_boxes else None, series=series,
                anchors=anchors, nan_series=nan_series)


def cases():
    out = []
    r = lambda a, b: list(range(a, b))
    # stride 1 (identity axis, holes of different lengths); first knot at frame 1 / 2 / 3; last at F / F-1 / F-2; L = 0, 1, 2
    out.append(build_case('stride1_holes', 1, 40, 40, None,
                          {(0, 0): r(0, 3) + [5, 6, 12] + r(30, 40),        # frames 1..40: first 1, last F
                           (0, 1): [1, 3, 4, 20],                           # first knot at 2 -> 1
                           (0, 2): [2, 9, 10, 11, 37],                      # first at 3, last at F-2
                           (0, 3): [],                                      # L = 0
                           (1, 0): [7],                                     # L = 1
                           (1, 1): [4, 38],                                 # L = 2, last at F-1 -> F
                           (1, 2): [1],                                     # L = 1 at frame 2: copied, NOT extrapolated
                           (1, 3): r(3, 30)},                               # t >= ntracks: rows not NaN, output NaN
                          nt=[4, 3], with_boxes=True, nan_series=(0, 0, 12)))
    # stride 2 from frame 2: first knot at 2 -> 1; last sampled frame F-1 -> F
    out.append(build_case('stride2', 2, 20, 41, r(2, 41)[::2],
                          {(0, 0): r(0, 20), (0, 1): [0, 5, 19], (1, 0): r(3, 11), (1, 1): [19], (1, 2): [18, 19]},
                          nt=[2, 3], f32_series=True))
    # stride 3 from frame 1: last sampled frame 43 = F-2
    out.append(build_case('stride3', 3, 15, 45, r(1, 45)[::3],
                          {(0, 0): r(0, 15), (0, 1): [2, 3, 9, 14], (0, 2): [0, 14], (1, 0): r(4, 9), (1, 3): r(0, 15)},
                          nt=[3, 1], with_boxes=True, f32_series=True, nser=4))
    # stride 7 from frame 3: first knot at 3, last at F
    out.append(build_case('stride7', 4, 12, 80, r(3, 81)[::7],
                          {(0, 0): r(0, 12), (0, 1): [0, 11], (1, 0): [1, 2, 6], (1, 1): r(5, 12)}, nt=[2, 2], nser=1))
    # L > 64 (more than one wave step), gaps of more than 64 frames (filled by the whole wave), a long gap right after a
    # first knot at frame 2 (the front rule and the wave fill on one interval), and knots that straddle the 64-row chunks
    out.append(build_case('long_identity', 5, 300, 300, None,
                          {(0, 0): [k for k in range(300) if k % 11 not in (3, 4)],          # L = 246
                           (0, 1): [0, 100, 199, 298],                                       # gaps 99, 98, 98; last F-1 -> F
                           (0, 2): [1, 150, 151, 299],                                       # first at 2, gap 148
                           (0, 3): [63, 64, 127, 129, 255],
                           (1, 0): r(60, 200), (1, 1): [299], (1, 2): [0, 299]}, nt=[4, 3], nser=0))
    # a long strided video: 300 sampled rows at stride 7 = 2 100 dense frames per tubelet, no series dtype in f64, boxes given
    out.append(build_case('long_stride7', 6, 300, 2100, r(2, 2101)[::7],
                          {(0, 0): r(0, 300), (0, 1): [k for k in range(300) if k % 5], (1, 0): [0, 1, 250, 299], (1, 1): r(100, 170)},
                          nt=[2, 2], with_boxes=True, nser=3))
    # integer boxes
    out.append(build_case('integer', 7, 10, 30, r(2, 30)[::3], {(0, 0): r(0, 10), (1, 0): [2, 7]}, nt=[1, 1], integer=True))
    return out


def case_frames(c):
    return np.arange(1, c['Fs'] + 1, dtype=np.int64) if c['frames'] is None else c['frames']


def live_knots(c):
    """[(frames of the knots, F)] of every live slot"""
    fr = case_frames(c)
    return [(fr[np.asarray(rows, dtype=np.int64)], c['F']) for (cc, t), rows in c['knots'].items() if t < c['nt'][cc]]


def test_case_set_covers_what_the_issue_lists():
    from vdetlib_amd import ops
    assert callable(ops.interpolate_tracks)
    cs = cases()
    strides = set()
    for c in cs:
        fr = case_frames(c)
        strides.add(int(fr[1] - fr[0]))
        assert np.all(np.diff(fr) == fr[1] - fr[0])
    assert {1, 2, 3, 7} <= strides
    kn = [k for c in cs for k in live_knots(c)]
    lens = [len(k) for k, _ in kn]
    assert 0 in lens and 1 in lens and 2 in lens and max(lens) > 64
    many = [(k, F) for k, F in kn if len(k) >= 2]
    assert {1, 2, 3} <= {int(k[0]) for k, _ in many}
    assert {0, 1, 2} <= {int(F - k[-1]) for k, F in many}
    # identity-axis holes of different lengths
    holes = set()
    for c in cs:
        if c['frames'] is None:
            for k, _ in live_knots(c):
                holes |= set((np.diff(k) - 1).tolist())
    assert len(holes - {0}) >= 3 and max(holes) > 64
    # a slot t >= ntracks[c] whose rows are NOT NaN
    assert any(t >= c['nt'][cc] and len(rows) > 0 for c in cs for (cc, t), rows in c['knots'].items())
    assert any(np.any(c['tracks'][~np.isnan(c['tracks'])] % 1 != 0) for c in cs)                       # fractional boxes
    assert any(s.dtype == np.float32 for c in cs for s in c['series']) and any(s.dtype == np.float64 for c in cs for s in c['series'])
    assert any(np.any(s[~np.isnan(s)] % 1 != 0) for c in cs for s in c['series'])                      # fractional scores
    assert any(c['boxes'] is None for c in cs) and any(c['boxes'] is not None for c in cs)
    nan_cases = [c for c in cs if c['nan_series'] is not None]
    assert nan_cases and all(c['nan_series'][2] in c['knots'][c['nan_series'][:2]] and np.isnan(c['series'][0][c['nan_series']])
                             for c in nan_cases)
    assert max(F for _, F in kn) >= 2000


def expected(oracle, tracks, nt, anchors, series, boxes, frames, F):
    """Every output of interpolate_tracks, assembled per slot from oracle.tubelet_interpolation (f64)."""
    C, T, Fs = tracks.shape[:3]
    fr = np.arange(1, Fs + 1, dtype=np.int64) if frames is None else np.asarray(frames, dtype=np.int64)
    nser = len(series)
    out = dict(tracks=np.full((C, T, F, 5), np.nan), boxes64=np.full((C, T, F, 4), np.nan), anchor=np.full((C, T, F), np.nan),
               series=[np.full((C, T, F), np.nan) for _ in range(nser)], anchors=anchors.astype(np.float32).copy())
    for c in range(C):
        for t in range(min(int(nt[c]), T)):
            rows = np.nonzero(~np.isnan(tracks[c, t, :, 0]))[0]
            a0 = float(anchors[c, t, 0])
            arow = int(a0) - 1 if a0 >= 1 else -1
            xa = float(fr[arow]) if 0 <= arow < Fs else float('nan')
            if not math.isnan(xa):
                out['anchors'][c, t, 0] = np.float32(xa)
            if len(rows) == 0:
                continue
            bx = (tracks[c, t, rows, :4] if boxes is None else boxes[c, t, rows]).astype(np.float64)
            cols = [bx, tracks[c, t, rows, 4:5].astype(np.float64), (fr[rows].astype(np.float64) - xa)[:, None]]
            cols += [s[c, t, rows].astype(np.float64)[:, None] for s in series]
            fields = np.concatenate(cols, axis=1)
            if len(rows) == 1:
                dense, vals = fr[rows], fields
            else:
                with np.errstate(all='ignore'):
                    dense, vals = oracle.tubelet_interpolation(fr[rows], fields, F)
            d = np.asarray(dense) - 1
            out['boxes64'][c, t, d] = vals[:, :4]
            out['tracks'][c, t, d] = vals[:, :5]
            out['anchor'][c, t, d] = vals[:, 5]
            for q in range(nser):
                out['series'][q][c, t, d] = vals[:, 6 + q]
    return out


def bits64(a, b):
    a, b = np.atleast_1d(np.ascontiguousarray(a, dtype=np.float64)), np.atleast_1d(np.ascontiguousarray(b, dtype=np.float64))
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a.view(np.int64)[~na], b.view(np.int64)[~nb])


def bits32(a, b):
    assert a.dtype == np.float32
    b = np.ascontiguousarray(b).astype(np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(np.ascontiguousarray(a).view(np.int32)[~na], b.view(np.int32)[~nb])


def run_case(c, **kw):
    import torch
    from vdetlib_amd import ops
    g = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return ops.interpolate_tracks(g(c['tracks']), g(c['nt']), g(c['anchors']), [g(s) for s in c['series']],
                                  boxes=None if c['boxes'] is None else g(c['boxes']), frames=c['frames'], num_frames=c['F'], **kw)


def check_against(out, want, tag):
    import torch
    assert out['boxes64'].dtype == torch.float64 and out['anchor'].dtype == torch.float64
    assert bits64(out['boxes64'].cpu().numpy(), want['boxes64']), tag
    assert bits64(out['anchor'].cpu().numpy(), want['anchor']), tag
    assert len(out['series']) == len(want['series'])
    for got, w in zip(out['series'], want['series']):
        assert got.dtype == torch.float64 and bits64(got.cpu().numpy(), w), tag
    assert bits32(out['tboxes'].cpu().numpy(), want['boxes64']), tag
    assert bits32(out['tracks'].cpu().numpy(), want['tracks']), tag
    assert bits32(out['anchors'].cpu().numpy(), want['anchors']), tag


def test_bit_equal_to_the_oracle(oracle):
    n = 0
    for c in cases():
        out = run_case(c)
        want = expected(oracle, c['tracks'], c['nt'], c['anchors'], c['series'], c['boxes'], c['frames'], c['F'])
        check_against(out, want, c['name'])
        C, T = c['tracks'].shape[:2]
        assert tuple(out['tracks'].shape) == (C, T, c['F'], 5) and out['ntracks'].cpu().numpy().tolist() == c['nt'].tolist()
        n += 1
    assert n == len(cases()) == 7


# ---------------------------------------------------------------------------------------------------------------------
# the reference's recorded output
# ---------------------------------------------------------------------------------------------------------------------
def _close(a, b, tol):
    """tests/test_pipeline_gpu.py::_close: ints / strings exact, floats within tol."""
    if isinstance(a, dict):
        assert isinstance(b, dict) and sorted(a) == sorted(b), (sorted(a), sorted(b) if isinstance(b, dict) else b)
        for k in a:
            _close(a[k], b[k], tol)
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), (len(a), len(b))
        for x, y in zip(a, b):
            _close(x, y, tol)
    elif isinstance(a, float) or isinstance(b, float):
        assert abs(float(a) - float(b)) <= tol, (a, b)
    else:
        assert a == b, (a, b)


def test_reference_golden_cases(proto_golden):
    import torch
    from vdetlib_amd import ops
    F = 12
    g = proto_golden['interpolation']
    assert sorted(g) == ['dense', 'min2_maxF1', 'single', 'sparse']
    for tag, c in g.items():
        tubs = c['inp']['tubelets']
        assert len(tubs) == 1
        bx = tubs[0]['boxes']
        tracks = np.full((1, 1, F, 5), np.nan, np.float32)
        det = np.full((1, 1, F), np.nan)
        for b in bx:
            tracks[0, 0, b['frame'] - 1] = b['bbox'] + [b['track_score']]
            det[0, 0, b['frame'] - 1] = b['det_score']
            assert b['anchor'] == b['frame'] - bx[0]['frame']
        anchors = np.array([[[bx[0]['frame'], 0, 0]]], np.float32)
        out = ops.interpolate_tracks(torch.from_numpy(tracks).cuda(), torch.ones(1, dtype=torch.int32).cuda(),
                                     torch.from_numpy(anchors).cuda(), [torch.from_numpy(det).cuda()], num_frames=F)
        b64, ser, anc = out['boxes64'].cpu().numpy()[0, 0], out['series'][0].cpu().numpy()[0, 0], out['anchor'].cpu().numpy()[0, 0]
        got = [{'frame': f + 1, 'det_score': float(ser[f]), 'anchor': float(anc[f]), 'bbox': [float(v) for v in b64[f]]}
               for f in range(F) if not np.isnan(out['tracks'][0, 0, f, 0].item())]
        want = [{k: b[k] for k in ('frame', 'det_score', 'anchor', 'bbox')} for b in c['out']['tubelets'][0]['boxes']]
        _close(got, want, tol=1e-9)


# ---------------------------------------------------------------------------------------------------------------------
# strided video end to end
# ---------------------------------------------------------------------------------------------------------------------
B, C, T = 64, 4, 4
STRIDE, FS = 3, 8
FRAMES = np.arange(2, 2 + STRIDE * FS, STRIDE)       # 2, 5, ..., 23: the first sampled frame fires lo == 2 -> 1,
FD = int(FRAMES[-1]) + 1                              # ... the last one is F - 1 = 23 of F = 24 frames
# (class, first sampled row, one past the last): lifetimes on the SAMPLED axis
OBJECTS = [(1, 0, FS), (2, 3, 4), (2, 5, 8), (3, 0, 5), (1, 2, 7)]


def make_video(seed, nfs=FS, frames=FRAMES, objects=OBJECTS):
    """The sampled volume of a planted-object video (integer boxes): 6 jittered copies of every object while it lives +
    low-scored clutter; ground truth on EVERY dense frame the object spans (linear motion, so the interpolated boxes lie
    near it)."""
    rng = np.random.RandomState(seed)
    boxes = np.zeros((nfs, B, 4), np.float32)
    scores = (0.05 * rng.rand(nfs, B, C)).astype(np.float32)
    name = 'interp_%d' % seed
    annot = {'video': name, 'annotations': []}
    for i in range(nfs):
        cx, cy = rng.uniform(0, 1100, B), rng.uniform(620, 900, B)
        boxes[i] = np.stack([cx, cy, cx + rng.uniform(20, 200, B), cy + rng.uniform(20, 150, B)], 1)
    for k, (cls, r0, r1) in enumerate(objects):
        r1 = min(r1, nfs)
        x, y = 60 + 190 * k, 50 + 60 * k
        box = np.array([x, y, x + rng.uniform(80, 160), y + rng.uniform(80, 160)])
        vel = rng.uniform(-1, 1, 2)
        track = []
        for f in range(int(frames[r0]), int(frames[r1 - 1]) + 1):
            track.append({'frame': f, 'bbox': [int(q) for q in np.round(box + np.tile(vel, 2) * f)], 'class_index': cls, 'class': 'c%d' % cls})
        annot['annotations'].append({'id': str(k), 'track': track})
        for i in range(r0, r1):
            gtb = np.round(box + np.tile(vel, 2) * int(frames[i]))
            for j in range(6):
                boxes[i, k * 6 + j] = gtb + rng.randint(-4, 5, 4)
                scores[i, k * 6 + j, cls - 1] = 0.6 + 0.39 * rng.rand()
    return np.round(boxes).astype(np.float32), scores, annot


TRACK_KW = dict(nms_thres=0.3, thres=0.5, max_tracks=T, link_thres=0.4)


def knot_lengths(tr, nt):
    has = ~np.isnan(tr[..., 0])
    return [(c, t, np.nonzero(has[c, t])[0]) for c in range(tr.shape[0]) for t in range(int(nt[c]))]


def assert_tracker_shapes(tr, nt, frames, F):
    ks = knot_lengths(tr, nt)
    lens = [len(r) for _, _, r in ks]
    assert sum(l >= 2 for l in lens) >= 3 and 1 in lens, lens
    assert any(len(r) >= 2 and frames[r[0]] == 2 for _, _, r in ks), "no tubelet fires lo == 2 -> 1"
    assert any(len(r) >= 2 and frames[r[-1]] == F - 1 for _, _, r in ks), "no tubelet fires hi == F-1 -> F"


def test_strided_video_tracker_shapes_on_the_oracle(oracle):
    """What test_strided_video_equals_the_dict_path asserts about the GPU tracker, on the CPU oracle's tracker."""
    from vdetlib_amd import ops
    assert callable(ops.interpolate_tracks_batch)
    boxes, scores, _ = make_video(11)
    tr = np.full((C, T, FS, 5), np.nan, np.float32)
    nt = np.zeros(C, np.int32)
    for c in range(C):
        trc, _, n = oracle.greedy_track_volume(boxes, scores[:, :, c], **TRACK_KW)
        tr[c], nt[c] = trc, n
    assert_tracker_shapes(tr, nt, FRAMES, FD)


def test_strided_video_equals_the_dict_path():
    import torch
    from vdetlib_amd import eval as vev, ops
    from vdetlib_amd.utils.protocol import tubelets_proto_from_tracks_proto
    from vdetlib_amd.vdet import tubelet_cls as TC
    from vdetlib_amd.vdet.tcn import TCNNet
    boxes, scores, annot = make_video(11)
    name = annot['video']
    tb, ts = torch.from_numpy(boxes).cuda(), torch.from_numpy(scores).cuda()
    _, _, tr, an, nt = ops.nms_track_volume(tb, ts, **TRACK_KW)
    det, pooled, ob = ops.rescore_tracks(tr, nt, tb, ts, overlap_thres=0.5, window=3)
    trh, anh, nth, deth, obh = (x.cpu().numpy() for x in (tr, an, nt, det, ob))
    assert_tracker_shapes(trh, nth, FRAMES, FD)
    net = TCNNet.random([(n, 1) for n in ('det_scores', 'anchors', 'abs_anchors')], hidden=(8, 8), kernel=3, seed=3)
    # device
    out = ops.interpolate_tracks(tr, nt, an, [det], boxes=ob, frames=FRAMES, num_frames=FD)
    conv = ops.tcn_tracks(net, out['tracks'], nt, out['anchors'], out['series'][0])
    ev = ops.DetEvaluator(vev.gt_table_from_annots([annot]))
    n_added = ev.add_tracks(name, out['tracks'], nt, scores=conv, boxes=out['tboxes'])
    # dict path: protos of the same device tensors with the frame map applied
    vid = synth.make_vid_proto(name, FD)
    protos = []
    for c in range(C):
        tp = ops.tracks_to_proto(name, trh[c], anh[c], int(nth[c]))
        tubs = tubelets_proto_from_tracks_proto(tp['tracks'], c + 1)
        for t, tub in enumerate(tubs):
            arow = int(anh[c, t, 0]) - 1
            for box in tub['boxes']:
                row = box['frame'] - 1
                box['det_score'] = float(deth[c, t, row])
                box['bbox'] = [int(v) for v in obh[c, t, row]]
                assert box['bbox'] == [float(v) for v in obh[c, t, row]]           # integer boxes: int() changes nothing
                box['frame'] = int(FRAMES[row])
                box['anchor'] = int(FRAMES[row] - FRAMES[arow])
                box['gt_overlap'] = 0
        sp = {'video': name, 'method': 'test', 'tubelets': tubs}
        dense = TC.score_proto_interpolation(sp, vid)
        for tub in dense['tubelets']:
            for box in tub['boxes']:
                box.setdefault('gt_overlap', 0)
                box.setdefault('track_score', 0.0)
        with contextlib.redirect_stdout(io.StringIO()):
            protos.append(TC.score_conv_cls(dense, net))
    b64, ser, anc, cv = (x.cpu().numpy() for x in (out['boxes64'], out['series'][0], out['anchor'], conv))
    has = ~np.isnan(out['tracks'][..., 0].cpu().numpy())
    nbox = 0
    for c, sp in enumerate(protos):
        assert len(sp['tubelets']) == int(nth[c])
        for t, tub in enumerate(sp['tubelets']):
            fr = [b['frame'] for b in tub['boxes']]
            assert fr == (np.nonzero(has[c, t])[0] + 1).tolist(), (c, t)
            for b in tub['boxes']:
                f = b['frame'] - 1
                assert bits64(b64[c, t, f], np.array(b['bbox'], dtype=np.float64)), (c, t, f)
                assert bits64(ser[c, t, f], np.float64(b['det_score'])) and bits64(anc[c, t, f], np.float64(b['anchor'])), (c, t, f)
                assert bits32(cv[c, t, f:f + 1], np.array([b['conv_score']], dtype=np.float32)), (c, t, f)
                nbox += 1
        assert not has[c, int(nth[c]):].any()
    assert nbox == int(has.sum()) == n_added > 0
    dets = vev.detections_from_score_protos(protos, key='conv_score')
    aps_h, map_h = vev.evaluate(dets, vev.ground_truth_from_annots([annot]), 0.5)
    aps_d, map_d = ev.compute()
    assert sorted(aps_d) == sorted(aps_h)
    for c in aps_h:
        assert (math.isnan(aps_h[c]) and math.isnan(aps_d[c])) or abs(aps_d[c] - aps_h[c]) < 1e-12, (c, aps_d[c], aps_h[c])
    assert abs(map_d - map_h) < 1e-12 and map_h > 0


# ---------------------------------------------------------------------------------------------------------------------
# batch
# ---------------------------------------------------------------------------------------------------------------------
def test_batch_equals_video_by_video():
    import torch
    from vdetlib_amd import eval as vev, ops
    from vdetlib_amd.vdet.tcn import TCNNet
    # (sampled rows, stride, first frame, dense frames)
    geo = [(8, 3, 2, 24), (5, 1, 1, 5), (12, 2, 1, 25), (6, 7, 3, 40)]
    frs = [np.arange(f0, f0 + s * n, s) for n, s, f0, _ in geo]
    vids = [make_video(30 + i, nfs=n, frames=frs[i], objects=[(1, 0, n), (2, 1, 2), (3, 2, n - 1), (2, 3, 5)])
            for i, (n, s, f0, F) in enumerate(geo)]
    boxes = torch.from_numpy(np.concatenate([v[0] for v in vids], 0)).cuda()
    scores = torch.from_numpy(np.concatenate([v[1] for v in vids], 0)).cuda()
    off = np.concatenate([[0], np.cumsum([g[0] for g in geo])])
    bo = ops.video_batch(boxes, scores, off, overlap_thres=0.5, **TRACK_KW)
    assert int(bo['ntracks'].sum()) >= 2 * len(geo)
    nf = [g[3] for g in geo]
    dn = ops.interpolate_tracks_batch(bo, np.concatenate(frs), nf)
    assert dn['frame_off'].tolist() == np.concatenate([[0], np.cumsum(nf)]).tolist()
    names = [v[2]['video'] for v in vids]
    net = TCNNet.random([(n, 1) for n in ('det_scores', 'track_scores', 'anchors', 'abs_anchors')], hidden=(8, 8), kernel=3, seed=5)
    ev_b = ops.DetEvaluator(vev.gt_table_from_annots([v[2] for v in vids]))
    ev_1 = ops.DetEvaluator(vev.gt_table_from_annots([v[2] for v in vids]))
    conv_b = ops.tcn_tracks_batch(net, dn, series='det')
    flat, ov_views, mean_b, flag_b = ops.tubelets_overlap_batch(ev_b, names, dn, use_tboxes=True)
    n_b = ev_b.add_batch(names, dn)
    n_1 = 0
    eq = lambda a, b: a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.nan_to_num(-7.0), b.nan_to_num(-7.0))
    for v in range(len(geo)):
        one = ops.interpolate_tracks(bo['tracks'][v], bo['ntracks'][v], bo['anchors'][v], [bo['det'][v], bo['pooled'][v]],
                                     boxes=bo['tboxes'][v], frames=frs[v], num_frames=nf[v])
        assert tuple(dn['tracks'][v].shape) == (C, T, nf[v], 5)
        assert eq(dn['tracks'][v], one['tracks']) and eq(dn['tboxes'][v], one['tboxes']) and eq(dn['boxes64'][v], one['boxes64'])
        assert eq(dn['det'][v], one['series'][0]) and eq(dn['pooled'][v], one['series'][1]) and eq(dn['anchor'][v], one['anchor'])
        assert eq(dn['anchors'][v], one['anchors']) and (~torch.isnan(one['tracks'][..., 0])).any()
        c1 = ops.tcn_tracks(net, one['tracks'], bo['ntracks'][v], one['anchors'], one['series'][0])
        assert eq(conv_b[v], c1)
        go, m1, f1 = ops.tubelets_overlap(ev_1, names[v], one['tracks'], bo['ntracks'][v], boxes=one['tboxes'])
        assert eq(ov_views[v], go) and eq(mean_b[v], m1) and torch.equal(flag_b[v], f1)
        n_1 += ev_1.add_tracks(names[v], one['tracks'], bo['ntracks'][v], scores=one['series'][1], boxes=one['tboxes'])
    assert n_b == n_1 > 0
    for a, b in zip(ev_b.stream(raw=True), ev_1.stream(raw=True)):
        assert torch.equal(a, b)
    assert ev_b.compute() == ev_1.compute() or str(ev_b.compute()) == str(ev_1.compute())


# ---------------------------------------------------------------------------------------------------------------------
# no host wait, argument errors
# ---------------------------------------------------------------------------------------------------------------------
def test_async_call_never_waits_for_the_device(oracle):
    from vdetlib_amd import _lib
    cx = _lib.Context()
    try:
        for c in (cases()[2], cases()[0]):                 # a frame table (staged in the context) and the identity axis
            want = expected(oracle, c['tracks'], c['nt'], c['anchors'], c['series'], c['boxes'], c['frames'], c['F'])
            first = run_case(c, ctx=cx)
            before = cx.query(8)
            again = run_case(c, sync=False, ctx=cx)
            third = run_case(c, sync=False, ctx=cx)
            assert cx.query(8) == before, "an asynchronous interpolate_tracks waited for the device"
            cx.sync()
            assert cx.query(8) == before + 1
            for out in (first, again, third):
                check_against(out, want, c['name'])
    finally:
        cx.close()


def test_argument_errors():
    import torch
    from vdetlib_amd import ops
    c = cases()[2]
    g = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    tr, nt, an, bx = g(c['tracks']), g(c['nt']), g(c['anchors']), g(c['boxes'])
    ser = [g(s) for s in c['series']]
    fr, F = c['frames'], c['F']
    ok = lambda **kw: ops.interpolate_tracks(**dict(dict(tracks=tr, ntracks=nt, anchors=an, series=ser, boxes=bx, frames=fr, num_frames=F), **kw))
    ok()
    with pytest.raises(ValueError):
        ok(tracks=tr.double())                                     # dtypes
    with pytest.raises(ValueError):
        ok(ntracks=nt.long())
    with pytest.raises(ValueError):
        ok(anchors=an.double())
    with pytest.raises(ValueError):
        ok(boxes=bx.double())
    with pytest.raises(ValueError):
        ok(series=[ser[0].half()])
    with pytest.raises(ValueError):
        ok(series=[ser[0], ser[1].double()])                       # mixed series dtypes
    with pytest.raises(ValueError):
        ok(series=ser + ser[:1])                                   # more than 4 series
    with pytest.raises(ValueError):
        ok(tracks=tr[..., :4])                                     # shapes
    with pytest.raises(ValueError):
        ok(ntracks=nt[:1])
    with pytest.raises(ValueError):
        ok(anchors=an[:, :2])
    with pytest.raises(ValueError):
        ok(boxes=bx[:, :, :-1])
    with pytest.raises(ValueError):
        ok(series=[ser[0][:, :, :-1]])
    with pytest.raises(ValueError):
        ok(series=[ser[0].cpu()])                                  # devices
    with pytest.raises(ValueError):
        ok(tracks=tr.cpu())
    with pytest.raises(ValueError):
        ok(boxes=bx.cpu())
    with pytest.raises(ValueError):
        ok(frames=fr[:-1])                                         # wrong length
    bad = fr.copy()
    bad[3] = bad[2]
    with pytest.raises(ValueError):
        ok(frames=bad)                                             # not strictly ascending
    with pytest.raises(ValueError):
        ok(frames=fr - 1)                                          # below 1
    with pytest.raises(ValueError):
        ok(frames=fr.astype(np.float64))                           # not integers
    with pytest.raises(ValueError):
        ok(num_frames=int(fr[-1]) - 1)                             # num_frames < frames[-1]
    with pytest.raises(ValueError):
        ok(frames=None, num_frames=c['Fs'] - 1)                    # identity axis shorter than the rows
    # the batch form
    boxes, scores, _ = make_video(11)
    bo = ops.video_batch(torch.from_numpy(boxes).cuda(), torch.from_numpy(scores).cuda(), [0, 3, FS], overlap_thres=0.5, **TRACK_KW)
    frb = np.concatenate([FRAMES[:3], FRAMES[:FS - 3]])
    ops.interpolate_tracks_batch(bo, frb, [10, 20])
    with pytest.raises(ValueError):
        ops.interpolate_tracks_batch(bo, frb, [10])                # one count per video
    with pytest.raises(ValueError):
        ops.interpolate_tracks_batch(bo, frb, [7, 20])             # num_frames < the video's last frame
    with pytest.raises(ValueError):
        ops.interpolate_tracks_batch(bo, FRAMES[::-1].copy(), [30, 30])
    with pytest.raises(ValueError):
        ops.interpolate_tracks_batch(bo, frb[:-1], [10, 20])
    assert ok()['tracks'].shape[2] == F                            # the context still works
