"""-m gpu: the device TCN (ops.tcn_tracks / tcn_tracks_batch, TCNNet.forward_series, score_conv_cls_batched;
csrc/tcn_kernels.hpp) against the per-tubelet path (tracks_to_proto + score_conv_cls + TCNNet.forward, one launch per
layer and tubelet).  Both run the same f32 operation sequence on the same GPU, so the comparison is on the f32 bits;
against the oracle's numpy net the tolerance is the 1e-5 of test_pipeline_gpu.py (expf: GPU vs libm)."""
import contextlib
import copy
import io
import math
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F, B, C, T = 24, 96, 6, 4
# (class, first frame, one past the last frame): object lifetimes of the test video.  Classes 4..6 have no object.
OBJECTS = [(1, 0, F), (2, 3, 4), (2, 8, 10), (3, 2, F - 5), (1, 0, 7)]


def make_video(seed, nf=F, objects=OBJECTS):
    """Integer-valued proposals: 6 jittered copies of every object while it lives (scored 0.6 .. 0.99 for its class) +
    clutter scored < 0.05; the ground truth as an annotation proto."""
    rng = np.random.RandomState(seed)
    boxes = np.zeros((nf, B, 4), np.float32)
    scores = (0.05 * rng.rand(nf, B, C)).astype(np.float32)
    annot = {'video': 'tcn_%d' % seed, 'annotations': []}
    objs = []
    for k, (cls, f0, f1) in enumerate(objects):
        x, y = 60 + 190 * k, 50 + 60 * k
        w, h = rng.uniform(80, 160), rng.uniform(80, 160)
        objs.append((cls, f0, min(f1, nf), np.array([x, y, x + w, y + h]), rng.uniform(-2, 2, 2)))
        annot['annotations'].append({'id': str(k), 'track': []})
    for f in range(nf):
        cx, cy = rng.uniform(0, 1100, B), rng.uniform(620, 900, B)           # clutter lives below the objects
        boxes[f] = np.stack([cx, cy, cx + rng.uniform(20, 200, B), cy + rng.uniform(20, 150, B)], 1)
        for k, (cls, f0, f1, box, v) in enumerate(objs):
            if not f0 <= f < f1:
                continue
            gtb = np.round(box + np.tile(v, 2) * f)
            annot['annotations'][k]['track'].append({'frame': f + 1, 'bbox': [int(q) for q in gtb], 'class_index': cls,
                                                     'class': 'c%d' % cls})
            for j in range(6):
                boxes[f, k * 6 + j] = gtb + rng.randint(-4, 5, 4)
                scores[f, k * 6 + j, cls - 1] = 0.6 + 0.39 * rng.rand()
    annot['annotations'] = [a for a in annot['annotations'] if a['track']]
    return np.round(boxes).astype(np.float32), scores, annot


@pytest.fixture(scope="module")
def video():
    import torch
    from vdetlib_amd import ops
    boxes, scores, annot = make_video(7)
    tb, ts = torch.from_numpy(boxes).cuda(), torch.from_numpy(scores).cuda()
    _, _, tr, an, nt = ops.nms_track_volume(tb, ts, nms_thres=0.3, thres=0.5, max_tracks=T, link_thres=0.4)
    det, pooled, ob = ops.rescore_tracks(tr, nt, tb, ts, overlap_thres=0.5, window=3)
    return dict(annot=annot, tr=tr, an=an, nt=nt, det=det, pooled=pooled, ob=ob)


def _lengths(tr, nt):
    has = ~np.isnan(tr[..., 0])
    return [[int(has[c, t].sum()) for t in range(int(nt[c]))] for c in range(tr.shape[0])]


def test_video_has_the_shapes_the_checks_need(video):
    """Tubelets of differing lengths, of length 1 and 2, a class without tubelets, one touching frame 1 and one frame F."""
    tr, nt = video['tr'].cpu().numpy(), video['nt'].cpu().numpy()
    lens = [l for ls in _lengths(tr, nt) for l in ls]
    print("ntracks", nt.tolist(), "lengths", _lengths(tr, nt))
    assert (nt == 0).any() and (nt > 0).sum() >= 3
    assert 1 in lens and 2 in lens and len(set(lens)) >= 4
    has = ~np.isnan(tr[..., 0])
    live = np.arange(T)[None, :] < nt[:, None]
    assert (has[..., 0] & live).any() and (has[..., -1] & live).any()


def per_tubelet_reference(v, net, series='det', gt_overlap=None):
    """conv_score [C,T,F] f32 through the dict API: tracks_to_proto -> tubelets_proto_from_tracks_proto -> det_score
    (and gt_overlap) of the series -> score_conv_cls with the per-layer TCNNet.forward.  EVERY (c, t < ntracks[c])."""
    from vdetlib_amd import ops
    from vdetlib_amd.utils.protocol import tubelets_proto_from_tracks_proto
    from vdetlib_amd.vdet import tubelet_cls as TC
    tr, an, nt = (v[k].cpu().numpy() for k in ('tr', 'an', 'nt'))
    ser = v[series].cpu().numpy()
    go = None if gt_overlap is None else gt_overlap.cpu().numpy()
    nC, nT, nF = ser.shape
    want = np.full((nC, nT, nF), np.nan, np.float32)
    protos = []
    for c in range(nC):
        tp = ops.tracks_to_proto('vid', tr[c], an[c], int(nt[c]))
        tubs = tubelets_proto_from_tracks_proto(tp['tracks'], c + 1)
        assert len(tubs) == int(nt[c])
        for t, tub in enumerate(tubs):
            for box in tub['boxes']:
                box['det_score'] = float(ser[c, t, box['frame'] - 1])
                box['gt_overlap'] = float(go[c, t, box['frame'] - 1]) if go is not None else 0
        proto = {'video': 'vid', 'method': 'test', 'tubelets': tubs}
        with contextlib.redirect_stdout(io.StringIO()):
            out = TC.score_conv_cls(proto, net)
        for t, tub in enumerate(out['tubelets']):
            for box in tub['boxes']:
                want[c, t, box['frame'] - 1] = np.float32(box['conv_score'])
        protos.append(proto)
    return want, protos


def numpy_channels(tub, names):
    """The channel assembly of score_conv_cls restated in numpy (f64 -> one rounding to f32)."""
    boxes = tub['boxes']
    n = len(boxes)
    rel = np.asarray([b['anchor'] for b in boxes], dtype=np.float64) / n
    go = np.asarray([b['gt_overlap'] for b in boxes], dtype=np.float64)
    ch = {'det_scores': np.asarray([b['det_score'] for b in boxes], dtype=np.float64),
          'track_scores': np.asarray([b['track_score'] for b in boxes], dtype=np.float64),
          'anchors': rel, 'abs_anchors': np.abs(rel), 'gt_overlaps': go, 'labels': (go >= 0.5).astype(np.float64)}
    return np.stack([ch[n_].astype(np.float32) for n_ in names], 0)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    nan_a, nan_b = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(nan_a, nan_b) and np.array_equal(a.view(np.uint32)[~nan_a], b.view(np.uint32)[~nan_b])


BASE = ['det_scores', 'track_scores', 'anchors', 'abs_anchors']
NETS = {
    # name: (input names, hidden widths, K, seed)
    'k1_one_layer': (BASE, (), 1, 1),
    'k3_two_layers': (BASE, (16,), 3, 2),
    'k5_three_layers': (BASE, (8, 8), 5, 3),
    'k3_four_layers_odd_width': (['abs_anchors', 'det_scores', 'anchors', 'track_scores'], (7, 10, 5), 3, 4),
    'k5_reordered': (['anchors', 'track_scores', 'det_scores'], (16, 16), 5, 5),
    'k5_tiled_width_192': (BASE, (192, 24), 5, 6),          # 8 B * 192 * (24 + 12) > 48 KiB: tiled along the series
    'k5_global_width_512': (BASE, (512, 8), 5, 7),          # no 16-position tile fits: activations in global memory
    'k3_gt_channels': (['det_scores', 'gt_overlaps', 'labels', 'anchors'], (12, 6), 3, 8),
}


def make_net(key):
    from vdetlib_amd.vdet.tcn import TCNNet
    names, hidden, k, seed = NETS[key]
    return TCNNet.random([(n, 1) for n in names], hidden=hidden, kernel=k, seed=seed), names


@pytest.mark.parametrize("key", sorted(NETS))
def test_bit_equal_to_per_tubelet_path_and_close_to_oracle(video, oracle, key):
    from vdetlib_amd import ops
    net, names = make_net(key)
    go = None
    if 'gt_overlaps' in names:
        go, _, _ = ops.tubelets_overlap(ops.DetEvaluator(_gt_table(video)), video['annot']['video'], video['tr'], video['nt'])
    series = 'pooled' if key == 'k5_reordered' else 'det'
    got = ops.tcn_tracks(net, video['tr'], video['nt'], video['an'], video[series], gt_overlap=go).cpu().numpy()
    want, protos = per_tubelet_reference(video, net, series, go)
    assert got.dtype == np.float32 and same_bits(got, want)
    has = ~np.isnan(video['tr'][..., 0].cpu().numpy()) & (np.arange(T)[None, :, None] < video['nt'].cpu().numpy()[:, None, None])
    assert np.array_equal(~np.isnan(got), has)           # NaN exactly where there is no box
    # the oracle's numpy net on channels assembled in numpy, every tubelet
    worst = 0.0
    for c, proto in enumerate(protos):
        for t, tub in enumerate(proto['tubelets']):
            ref = oracle.tcn_forward(numpy_channels(tub, names), net.layers)[1]
            mine = np.array([got[c, t, b['frame'] - 1] for b in tub['boxes']])
            worst = max(worst, float(np.abs(mine - ref).max()))
            assert np.allclose(mine, ref, rtol=0, atol=1e-5), (c, t)
    print(key, "max |device - oracle| = %.3g" % worst)


def _gt_table(video):
    from vdetlib_amd import eval as vev
    return vev.gt_table_from_annots([video['annot']])


def test_f32_series_and_repeat_call_uploads_nothing(video):
    """A float32 score series gives what its float64 copy gives; the second call with the same net re-uploads nothing."""
    from vdetlib_amd import _lib, ops
    net, _ = make_net('k5_three_layers')
    cx = _lib.Context()
    try:
        d32 = video['det'].float()
        a = ops.tcn_tracks(net, video['tr'], video['nt'], video['an'], d32, ctx=cx)
        n_up = cx.query(10)
        b = ops.tcn_tracks(net, video['tr'], video['nt'], video['an'], d32.double(), ctx=cx)
        assert cx.query(10) == n_up == 1
        assert same_bits(a.cpu().numpy(), b.cpu().numpy())
    finally:
        cx.close()


def _ctx_with(env):
    from vdetlib_amd import _lib
    old = os.environ.get(env)
    os.environ[env] = "1"
    try:
        return _lib.Context()
    finally:
        if old is None:
            del os.environ[env]
        else:
            os.environ[env] = old


@pytest.mark.parametrize("key", ['k5_three_layers', 'k3_four_layers_odd_width', 'k5_tiled_width_192'])
def test_tiled_and_global_paths_equal_the_lds_path(video, key):
    from vdetlib_amd import ops
    net, _ = make_net(key)
    base = ops.tcn_tracks(net, video['tr'], video['nt'], video['an'], video['det']).cpu().numpy()
    for env in ('VDET_TCN_TILED', 'VDET_TCN_GLOBAL'):
        cx = _ctx_with(env)
        try:
            got = ops.tcn_tracks(net, video['tr'], video['nt'], video['an'], video['det'], ctx=cx).cpu().numpy()
            assert same_bits(got, base), env
            series = [np.random.RandomState(5).randn(len(net.inputs), n).astype(np.float32) for n in (1, 2, 17, 40, 131)]
            for x, y in zip(net.forward_series(series), net.forward_series(series, ctx=cx)):
                assert same_bits(x, y), env
        finally:
            cx.close()


def test_batch_equals_video_by_video():
    import torch
    from vdetlib_amd import ops
    nfs = [9, 24, 5, 17, 12, 30]
    vids = [make_video(20 + i, nf=nf, objects=[(1, 0, nf), (2, 1, 2), (3, 2, nf - 1), (2, 3, 5)]) for i, nf in enumerate(nfs)]
    boxes = torch.from_numpy(np.concatenate([v[0] for v in vids], 0)).cuda()
    scores = torch.from_numpy(np.concatenate([v[1] for v in vids], 0)).cuda()
    off = np.concatenate([[0], np.cumsum(nfs)])
    bo = ops.video_batch(boxes, scores, off, nms_thres=0.3, thres=0.5, max_tracks=T, link_thres=0.4, overlap_thres=0.5)
    assert int(bo['ntracks'].sum()) >= 2 * len(nfs)
    ev = ops.DetEvaluator(__import__('vdetlib_amd.eval', fromlist=['x']).gt_table_from_annots([v[2] for v in vids]))
    names = [v[2]['video'] for v in vids]
    flat, views, mean, flag = ops.tubelets_overlap_batch(ev, names, bo)
    for key in ('k5_three_layers', 'k3_gt_channels', 'k5_tiled_width_192'):
        net, _ = make_net(key)
        got = ops.tcn_tracks_batch(net, bo, gt_overlap=flat)
        for v in range(len(nfs)):
            go, m1, f1 = ops.tubelets_overlap(ev, names[v], bo['tracks'][v], bo['ntracks'][v])
            assert torch.equal(go.nan_to_num(-7.0), views[v].nan_to_num(-7.0))
            assert torch.equal(m1.nan_to_num(-7.0), mean[v].nan_to_num(-7.0)) and torch.equal(f1, flag[v])
            one = ops.tcn_tracks(net, bo['tracks'][v], bo['ntracks'][v], bo['anchors'][v], bo['det'][v], gt_overlap=go)
            assert tuple(got[v].shape) == (C, T, nfs[v])
            assert same_bits(got[v].cpu().numpy(), one.cpu().numpy()), (key, v)


def test_forward_series_and_batched_dict_entry(proto_golden):
    from vdetlib_amd.vdet import tubelet_cls as TC
    from vdetlib_amd.vdet.tcn import TCNNet
    inp = proto_golden['score_conv_cls']['inp']
    for names, hidden, k in ((BASE, (8, 8), 5), (['gt_overlaps', 'labels', 'det_scores'], (5,), 3)):
        net = TCNNet.random([(n, 1) for n in names], hidden=hidden, kernel=k, seed=11)
        with contextlib.redirect_stdout(io.StringIO()):
            want = TC.score_conv_cls(copy.deepcopy(inp), net)
            got = TC.score_conv_cls_batched(copy.deepcopy(inp), net)
        assert sorted(got) == sorted(want) and len(got['tubelets']) == len(want['tubelets']) > 0
        series = []
        for tw, tg in zip(want['tubelets'], got['tubelets']):
            a = np.array([b['conv_score'] for b in tw['boxes']], dtype=np.float32)
            b = np.array([b['conv_score'] for b in tg['boxes']], dtype=np.float32)
            assert all(isinstance(x['conv_score'], float) for x in tg['boxes']) and same_bits(a, b)
            series.append(numpy_channels(tw, names))
        for tw, p in zip(want['tubelets'], net.forward_series(series)):
            assert same_bits(p, np.array([b['conv_score'] for b in tw['boxes']], dtype=np.float32))
    with pytest.raises(TypeError):
        TC.score_conv_cls_batched(copy.deepcopy(inp), object())


def test_errors_leave_a_working_context(video):
    import ctypes
    import torch
    from vdetlib_amd import _lib, ops
    from vdetlib_amd.vdet.tcn import TCNNet
    net, _ = make_net('k5_three_layers')
    tr, nt, an, det = video['tr'], video['nt'], video['an'], video['det']
    with pytest.raises(ValueError):       # even kernel size, at the python net ...
        TCNNet([('det_scores', 1)], [(np.zeros((2, 1, 4), np.float32), np.zeros(2, np.float32))])
    with pytest.raises(ValueError):       # ... a last layer that does not have 2 channels
        TCNNet([('det_scores', 1)], [(np.zeros((3, 1, 3), np.float32), np.zeros(3, np.float32))])
    cx = _lib.get_context(torch.cuda.current_device())
    out = torch.empty_like(det, dtype=torch.float32)
    codes = np.zeros(1, np.int32)
    params = np.zeros(64, np.float32)

    def raw(layers):
        ly = np.array(layers, dtype=np.int32)
        return cx.lib.vdet_tcn_tracks(cx.h, params.ctypes.data, ly.ctypes.data, len(layers), codes.ctypes.data, 1, F, C, T,
                                      tr.data_ptr(), nt.data_ptr(), an.data_ptr(), det.data_ptr(), 1, None, out.data_ptr())
    for bad in ([(2, 1, 4)], [(3, 1, 3)], [(4, 1, 3), (2, 5, 3)], [(2, 1, 33)]):        # ... and at the C-ABI
        assert raw(bad) == _lib.VDET_EINVAL
        with pytest.raises(ValueError):
            cx.check(_lib.VDET_EINVAL)
    gnet, _ = make_net('k3_gt_channels')
    with pytest.raises(ValueError):
        ops.tcn_tracks(gnet, tr, nt, an, det)                                   # gt_overlaps without a buffer
    gcodes = np.array([4], np.int32)
    ly = np.array([(2, 1, 3)], dtype=np.int32)
    assert cx.lib.vdet_tcn_tracks(cx.h, params.ctypes.data, ly.ctypes.data, 1, gcodes.ctypes.data, 1, F, C, T, tr.data_ptr(),
                                  nt.data_ptr(), an.data_ptr(), det.data_ptr(), 1, None, out.data_ptr()) == _lib.VDET_EINVAL
    with pytest.raises(ValueError):
        ops.tcn_tracks(TCNNet.random([('feats', 1)], hidden=(4,)), tr, nt, an, det)   # a blob the device cannot assemble
    with pytest.raises(ValueError):
        ops.tcn_tracks(TCNNet.random([('det_scores', 2)], hidden=(4,)), tr, nt, an, det)
    with pytest.raises(ValueError):
        ops.tcn_tracks(net, tr.double(), nt, an, det)                           # dtype
    with pytest.raises(ValueError):
        ops.tcn_tracks(net, tr, nt.long(), an, det)
    with pytest.raises(ValueError):
        ops.tcn_tracks(net, tr, nt, an, det.half())
    with pytest.raises(ValueError):
        ops.tcn_tracks(net, tr, nt, an[:, :2], det)                             # shape
    with pytest.raises(ValueError):
        ops.tcn_tracks(net, tr, nt, an, det[:, :, :-1])
    with pytest.raises(ValueError):
        ops.tcn_tracks(net, tr, nt, an, det.cpu())                              # device
    with pytest.raises(ValueError):
        ops.tcn_tracks(net, tr.cpu(), nt, an, det)
    with pytest.raises(ValueError):
        ops.tcn_tracks(object(), tr, nt, an, det)
    with pytest.raises(ValueError):
        net.forward_series([np.zeros((3, 5), np.float32)])
    want, _ = per_tubelet_reference(video, net)
    assert same_bits(ops.tcn_tracks(net, tr, nt, an, det).cpu().numpy(), want)      # the context still works
    assert [len(p) for p in net.forward_series([])] == []
    assert ctypes.c_int(cx.lib.vdet_tcn_series_f32(cx.h, None, None, 1, 4, None, None, 0, None)).value == _lib.VDET_EINVAL


def test_async_call_never_waits_for_the_device(video):
    from vdetlib_amd import _lib, ops
    net, _ = make_net('k5_three_layers')
    net2, _ = make_net('k3_two_layers')
    cx = _lib.Context()
    try:
        want = ops.tcn_tracks(net, video['tr'], video['nt'], video['an'], video['det'], ctx=cx)
        before = cx.query(8)
        got = ops.tcn_tracks(net, video['tr'], video['nt'], video['an'], video['pooled'], sync=False, ctx=cx)
        got2 = ops.tcn_tracks(net, video['tr'], video['nt'], video['an'], video['det'], sync=False, ctx=cx)
        assert cx.query(8) == before, "an asynchronous tcn_tracks waited for the device"
        cx.sync()
        assert cx.query(8) == before + 1
        assert same_bits(got2.cpu().numpy(), want.cpu().numpy())
        ref, _ = per_tubelet_reference(video, net, 'pooled')
        assert same_bits(got.cpu().numpy(), ref)
        # another net: one wait for the copy of the previous parameters, and the right result
        other = ops.tcn_tracks(net2, video['tr'], video['nt'], video['an'], video['det'], ctx=cx)
        ref2, _ = per_tubelet_reference(video, net2)
        assert same_bits(other.cpu().numpy(), ref2)
    finally:
        cx.close()


@pytest.mark.parametrize("rule", ('voc', 'ilsvrc'))
def test_end_to_end_evaluator_takes_conv_score(video, rule):
    from vdetlib_amd import eval as vev, ops
    net, _ = make_net('k5_three_layers')
    tr, nt = video['tr'], video['nt']
    conv = ops.tcn_tracks(net, tr, nt, video['an'], video['det'])
    ev = ops.DetEvaluator(_gt_table(video), rule=rule)
    name = video['annot']['video']
    n = ev.add_tracks(name, tr, nt, scores=conv)
    want, _ = per_tubelet_reference(video, net)
    dets = vev.detections_from_tracks(name, tr.cpu().numpy(), nt.cpu().numpy(), want)
    assert n == len(dets) > 0
    aps_h, map_h = vev.evaluate(dets, vev.ground_truth_from_annots([video['annot']]), 0.5, rule=rule)
    aps_d, map_d = ev.compute()
    assert sorted(aps_d) == sorted(aps_h)
    for c in aps_h:
        assert (math.isnan(aps_h[c]) and math.isnan(aps_d[c])) or abs(aps_d[c] - aps_h[c]) <= 1e-12, (c, aps_d[c], aps_h[c])
    assert abs(map_d - map_h) <= 1e-12
