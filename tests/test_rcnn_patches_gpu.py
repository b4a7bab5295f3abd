"""GPU: the R-CNN window warp on the device (ops.rcnn_patches / ops.tubelet_patches and the dict level above them) against
tests/patch_spec.py, bit for bit (torch.equal everywhere)."""
import functools

import numpy as np
import pytest
import torch

import patch_spec as ps

pytestmark = pytest.mark.gpu

H, W = 37, 53
MEAN = (103.939, 116.779, 123.68)
DEV = 'cuda'


@functools.lru_cache(maxsize=None)
def images():
    """Two uint8 random images of 37 x 53: [2,H,W,3]."""
    return np.random.RandomState(5).randint(0, 256, size=(2, H, W, 3)).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def case_boxes():
    """Every geometry case of tests/test_rcnn_patches_cpu.py, a one-pixel box, fractional boxes and a few random ones (f64 [42,4])
    and the image each is cut from."""
    rng = np.random.RandomState(6)
    b = [[10, 8, 30, 25], [3, 3, 5, 5], [2, 2, 4, 4], [1, 1, 3, 3], [1, 1, 2, 2],                 # inside; corners on x.5 / -x.5
         [-5, 10, 10, 20], [10, -4, 20, 9], [45, 10, 60, 20], [10, 30, 20, 45],                 # overhanging each edge
         [-10, -10, 70, 50], [3.75, 11, 10.25, 18],                                            # larger than the image; the clamp
         [100, 100, 120, 120], [-50, -50, -30, -30], [30, 25, 10, 8],                          # outside; inverted
         [5, 10, 34, 19], [10, 5, 19, 34],                                                     # 3:1 and 1:3
         [20, 20, 20, 20], [1, 1, 1, 1], [53, 37, 53, 37],                                     # one pixel
         [10.3, 8.7, 30.2, 25.9], [3.5, 3.5, 6.5, 7.25], [10.9, 8.2, 30.7, 25.5], [0.5, 0.5, 53.5, 37.5], [0.5, 5, 10, 10],
         [1, 1, 53, 37], [0, 5, 10, 10], [5, 5, 54, 10], [5, 5, 10, 38], [-3, -2, 4, 3], [50, 33, 56, 40]]
    for _ in range(12):
        x1, y1 = rng.uniform(-8, 50), rng.uniform(-8, 34)
        b.append([x1, y1, x1 + rng.uniform(0, 30), y1 + rng.uniform(0, 25)])
    b = np.asarray(b, dtype=np.float64)
    return b, (np.arange(len(b)) % 2).astype(np.int32)


def g(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def spec_patches(imgs, boxes, idx, mode, S, p, mean):
    pat, ok = ps.rcnn_patches(imgs, boxes, idx, mode, S, p, None if mean is None else np.asarray(mean))
    return torch.from_numpy(pat), torch.from_numpy(ok)


@functools.lru_cache(maxsize=None)
def spec_case(S, p, mode, use_mean, f32):
    b, idx = case_boxes()
    b = b.astype(np.float32) if f32 else b
    return spec_patches(images(), b, idx, mode, S, p, MEAN if use_mean else None)


def check(out, want, what=''):
    wp, wok = want
    assert out['ok'].dtype == torch.uint8 and torch.equal(out['ok'].cpu().reshape(-1), wok), what
    got = out['patches'].cpu().reshape(wp.shape)
    assert got.dtype == wp.dtype
    assert torch.equal(got.view(torch.int32), wp.view(torch.int32)), what        # the bits: zero border and -0.0 included


@pytest.mark.parametrize('use_mean', [True, False], ids=['mean', 'nomean'])
@pytest.mark.parametrize('mode', ['warp', 'square'])
@pytest.mark.parametrize('S,p', [(8, 2), (12, 0), (10, 3), (224, 16)])
def test_parity_with_the_spec(S, p, mode, use_mean):
    from vdetlib_amd import ops
    b, idx = case_boxes()
    assert len(b) == 42
    for f32 in (False, True):
        want = spec_case(S, p, mode, use_mean, f32)
        out = ops.rcnn_patches(g(images()), g(b.astype(np.float32) if f32 else b), g(idx), crop_size=S, padding=p,
                               mean=MEAN if use_mean else None, mode=mode)
        assert tuple(out['patches'].shape) == (42, 3, S, S) and 'sboxes' not in out
        check(out, want, 'f32 boxes' if f32 else 'f64 boxes')
        n_ok = int(want[1].sum())
        assert 10 <= n_ok < 42          # both outcomes are exercised


def test_nonfinite_boxes_and_image_index_out_of_range():
    """Ordinary inputs the kernel bound-checks: ok = 0, a zero patch, and the neighbours intact."""
    from vdetlib_amd import ops
    good = [10, 8, 30, 25]
    b = np.array([good, [np.nan, 1, 5, 5], good, [1, 1, np.inf, 5], good, [-np.inf, 1, 5, 5], [1e300, 1, 2, 3], good,
                  [-1e308, 1, 1e308, 5], good, good, good], dtype=np.float64)
    idx = np.array([0, 0, 1, 0, 0, 1, 0, 1, 0, 2, -1, 0], dtype=np.int32)
    for S, p in ((8, 2), (12, 0)):
        out = ops.rcnn_patches(g(images()), g(b), g(idx), crop_size=S, padding=p)
        check(out, spec_patches(images(), b, idx, 'warp', S, p, MEAN))
        assert out['ok'].cpu().tolist() == [1, 0, 1, 0, 1, 0, 0, 1, 0, 0, 0, 1]
        assert not out['patches'][out['ok'] == 0].any()
        assert torch.equal(out['patches'][0], out['patches'][4]) and out['patches'][0].any()


def test_offsets_are_sampling_boxes():
    from vdetlib_amd import ops
    rng = np.random.RandomState(7)
    N, num = 5, 3
    b = np.array([[10, 8, 30, 25], [3.5, 3.5, 16.5, 17.25], [-5, 10, 10, 20], [20, 20, 20, 20], [1, 1, 53, 37]], dtype=np.float64)
    off = rng.uniform(-0.05, 0.05, (N, num, 4))
    idx = np.array([0, 1, 0, 1, 1], dtype=np.int32)
    w, h = b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]
    want_boxes = np.concatenate([b[:, None], b[:, None] + off * np.stack([w, h, w, h], 1)[:, None]], 1)      # numpy f64
    for f32 in (False, True):
        bb = b.astype(np.float32) if f32 else b
        wb = ps.sampling_boxes(bb, off)
        if not f32:
            assert np.array_equal(wb, want_boxes)
        out = ops.rcnn_patches(g(images()), g(bb), g(idx), offsets=g(off), crop_size=8, padding=2)
        assert tuple(out['patches'].shape) == (N, num + 1, 3, 8, 8) and tuple(out['ok'].shape) == (N, num + 1)
        assert out['sboxes'].dtype == torch.float64 and np.array_equal(out['sboxes'].cpu().numpy(), wb)
        plain = ops.rcnn_patches(g(images()), g(bb), g(idx), crop_size=8, padding=2)
        assert torch.equal(out['patches'][:, 0], plain['patches']) and torch.equal(out['ok'][:, 0], plain['ok'])
        check(out, spec_patches(images(), wb.reshape(-1, 4), np.repeat(idx, num + 1), 'warp', 8, 2, MEAN))


def test_many_windows_past_the_grid_axis_limit():
    from vdetlib_amd import ops
    M, S = 70000, 4
    box = np.array([[10, 8, 30, 25]], dtype=np.float64)
    out = ops.rcnn_patches(g(images()[:1]), g(np.repeat(box, M, 0)), crop_size=S, padding=1)
    wp, wok = spec_patches(images()[:1], box, None, 'warp', S, 1, MEAN)
    assert wok[0] == 1 and bool(out['ok'].all()) and tuple(out['patches'].shape) == (M, 3, S, S)
    pick = [0, M - 1] + np.random.RandomState(8).randint(0, M, 100).tolist()
    got = out['patches'][torch.tensor(pick, device=DEV)].cpu()
    assert torch.equal(got.view(torch.int32), wp.expand(len(pick), -1, -1, -1).contiguous().view(torch.int32))


@pytest.mark.parametrize('S,p', [(8, 2), (12, 0), (10, 3), (224, 16)])
def test_half_precision_outputs_round_the_f32_value_once(S, p):
    from vdetlib_amd import ops
    b, idx = case_boxes()
    gi, gb, gx = g(images()), g(b), g(idx)
    f32 = ops.rcnn_patches(gi, gb, gx, crop_size=S, padding=p)
    for dt in (torch.float16, torch.bfloat16):
        out = ops.rcnn_patches(gi, gb, gx, crop_size=S, padding=p, dtype=dt)
        assert out['patches'].dtype == dt and torch.equal(out['ok'], f32['ok'])
        assert torch.equal(out['patches'].view(torch.int16), f32['patches'].to(dt).view(torch.int16))


def tubelet_case(C, T, F, ntracks, seed, holes):
    """tracks f32 [C,T,F,5] with boxes in and around the 37 x 53 image -- also in the slots behind ntracks, which must be
    skipped -- and NaN rows at holes (c,t,f)."""
    rng = np.random.RandomState(seed)
    x1, y1 = rng.uniform(-4, 44, (C, T, F)), rng.uniform(-4, 30, (C, T, F))
    tr = np.stack([x1, y1, x1 + rng.uniform(1, 20, (C, T, F)), y1 + rng.uniform(1, 16, (C, T, F)), rng.rand(C, T, F)], -1).astype(np.float32)
    for c, t, f in holes:
        tr[c, t, f] = np.nan
    return tr, np.asarray(ntracks, dtype=np.int32)


def check_tubelets(tr, nt, imgs, f0, f1, out, S, p, cap):
    want = ps.tubelet_slots(tr, nt, f0, f1)
    n = len(want)
    assert out['count'].dtype == torch.int32 and out['count'].cpu().tolist() == [n]
    slot = out['slot'].cpu().numpy()
    k = min(n, cap)
    assert slot.dtype == np.int32 and slot.shape == (cap, 3)
    assert np.array_equal(slot[:k], want[:k]) and (slot[k:] == -1).all()
    boxes = np.stack([tr[c, t, f, :4] for c, t, f in want[:k]]) if k else np.zeros((0, 4), np.float32)
    wp, wok = spec_patches(imgs, boxes, want[:k, 2] - f0, 'warp', S, p, MEAN)
    assert torch.equal(out['ok'].cpu()[:k], wok) and not out['ok'][k:].any()
    assert torch.equal(out['patches'].cpu()[:k].view(torch.int32), wp.view(torch.int32)) and not out['patches'][k:].any()
    return n


@pytest.mark.parametrize('frames', [(0, 9), (2, 7)])
def test_tubelet_patches(frames):
    from vdetlib_amd import ops
    C, T, F = 3, 4, 9
    holes = [(0, 0, 0), (0, 1, 4), (0, 2, 8), (1, 0, 2), (1, 1, 4), (0, 3, 6), (1, 0, 8), (0, 0, 2), (1, 1, 6), (0, 3, 4)]
    tr, nt = tubelet_case(C, T, F, [4, 2, 0], 11, holes)
    f0, f1 = frames
    imgs = np.random.RandomState(12).randint(0, 256, size=(F, H, W, 3)).astype(np.uint8)
    n = len(ps.tubelet_slots(tr, nt, f0, f1))
    for src in (tr, np.ascontiguousarray(tr[..., :4])):            # tracks rows (5 wide) and tboxes rows (4 wide)
        out = ops.tubelet_patches(g(imgs[f0:f1]), g(src), g(nt), (f0, f1), n + 3, crop_size=8, padding=2)
        assert check_tubelets(tr, nt, imgs[f0:f1], f0, f1, out, 8, 2, n + 3) == n
    assert n == 6 * (f1 - f0) - sum(1 for c, t, f in holes if f0 <= f < f1)


def test_tubelet_patches_cap_and_ballot_chunks():
    """720-odd present slots of 1350: the compaction crosses its 64-lane ballots and its 1024-slot chunk.  cap one short raises
    at the sync with the first cap windows valid; cap exact does not."""
    from vdetlib_amd import _lib, ops
    C, T, F = 3, 50, 9
    holes = [(0, 7, 0), (0, 49, 3), (1, 29, 8), (1, 0, 0), (0, 20, 5)]
    tr, nt = tubelet_case(C, T, F, [50, 30, 0], 13, holes)
    imgs = np.random.RandomState(14).randint(0, 256, size=(F, H, W, 3)).astype(np.uint8)
    n = len(ps.tubelet_slots(tr, nt, 0, F))
    assert n == 80 * F - len(holes) and n > 64 and C * T * F > 1024
    gi, gt, gn = g(imgs), g(tr), g(nt)
    out = ops.tubelet_patches(gi, gt, gn, (0, F), n, crop_size=4, padding=1)
    check_tubelets(tr, nt, imgs, 0, F, out, 4, 1, n)
    ctx = _lib.get_context(gi.device.index)
    out = ops.tubelet_patches(gi, gt, gn, (0, F), n - 1, crop_size=4, padding=1, sync=False)
    with pytest.raises(ValueError):
        ctx.sync()
    ctx.sync()                                   # the error was reported once
    check_tubelets(tr, nt, imgs, 0, F, out, 4, 1, n - 1)
    with pytest.raises(ValueError):
        ops.tubelet_patches(gi, gt, gn, (0, F), n - 1, crop_size=4, padding=1)


def test_asynchronous_mode_gives_the_same_bytes():
    from vdetlib_amd import _lib, ops
    b, idx = case_boxes()
    gi, gb, gx = g(images()), g(b), g(idx)
    tr, nt = tubelet_case(3, 4, 9, [4, 2, 0], 11, [(0, 0, 0), (1, 1, 4)])
    imgs = g(np.random.RandomState(12).randint(0, 256, size=(9, H, W, 3)).astype(np.uint8))
    gt, gn = g(tr), g(nt)
    a = ops.rcnn_patches(gi, gb, gx, crop_size=10, padding=3)
    ta = ops.tubelet_patches(imgs, gt, gn, (0, 9), 60, crop_size=8, padding=2)
    ctx = _lib.get_context(gi.device.index)
    ctx.set_async(True)
    try:
        syncs = ctx.query(8)
        c = ops.rcnn_patches(gi, gb, gx, crop_size=10, padding=3, sync=False)
        tc = ops.tubelet_patches(imgs, gt, gn, (0, 9), 60, crop_size=8, padding=2, sync=False)
        assert ctx.query(8) == syncs             # no host wait inside the calls
        ctx.sync()
    finally:
        ctx.set_async(False)
    for k in ('patches', 'ok'):
        assert torch.equal(a[k].view(torch.uint8), c[k].view(torch.uint8))
    for k in ('patches', 'ok', 'slot', 'count'):
        assert torch.equal(ta[k].view(torch.uint8), tc[k].view(torch.uint8))


def test_host_checks():
    from vdetlib_amd import ops
    gi, gb = g(images()), g(case_boxes()[0])
    gx = g(case_boxes()[1])
    bad = [lambda: ops.rcnn_patches(gi, gb), lambda: ops.rcnn_patches(gi.float(), gb, gx), lambda: ops.rcnn_patches(gi, gb.half(), gx),
           lambda: ops.rcnn_patches(gi, gb, gx.long()), lambda: ops.rcnn_patches(gi, gb, gx, crop_size=0),
           lambda: ops.rcnn_patches(gi, gb, gx, crop_size=1025), lambda: ops.rcnn_patches(gi, gb, gx, crop_size=8, padding=4),
           lambda: ops.rcnn_patches(gi, gb, gx, mode='crop'), lambda: ops.rcnn_patches(gi, gb, gx, dtype=torch.float64),
           lambda: ops.rcnn_patches(gi, gb.cpu(), gx), lambda: ops.rcnn_patches(gi, gb[:, :3], gx),
           lambda: ops.rcnn_patches(gi, gb, gx, offsets=gb[:, None, :].float()), lambda: ops.rcnn_patches(gi, gb, gx, mean=(1., 2.)),
           lambda: ops.rcnn_patches(gi[..., :2], gb, gx), lambda: ops.rcnn_patches(gi.permute(0, 2, 1, 3), gb, gx)]
    tr, nt = tubelet_case(2, 2, 3, [2, 1], 1, [])
    gt, gn = g(tr), g(nt)
    bad += [lambda: ops.tubelet_patches(gi, gt, gn, (0, 3), 4), lambda: ops.tubelet_patches(gi, gt, gn, (1, 4), 4),
            lambda: ops.tubelet_patches(gi, gt, gn, (2, 2), 4), lambda: ops.tubelet_patches(gi, gt[..., :3], gn, (0, 2), 4),
            lambda: ops.tubelet_patches(gi, gt, gn.long(), (0, 2), 4), lambda: ops.tubelet_patches(gi, gt, gn, (0, 2), -1)]
    for i, fn in enumerate(bad):
        with pytest.raises(ValueError):
            fn()
            pytest.fail("case %d did not raise" % i)


def test_rcnn_img_crop_dict_level():
    from vdetlib_amd.utils.common import rcnn_img_crop
    img = images()[0]
    mean = np.asarray(MEAN)
    for box, mode, S, p in (([10, 8, 30, 25], 'warp', 8, 2), ([-5.5, 10, 10, 20.25], 'square', 10, 3), ([3, 3, 5, 5], 'warp', 224, 16)):
        got = rcnn_img_crop(img, np.asarray(box, dtype=np.float64), mode, S, p, mean)
        want, ok = ps.rcnn_window(img, box, mode, S, p, mean)
        assert ok == 1 and got.dtype == np.float32 and got.shape == (S, S, 3)
        assert np.array_equal(got.view(np.int32), want.view(np.int32))
    assert np.array_equal(rcnn_img_crop(img, np.array([10., 8., 30., 25.]), 'warp', 8, 2), ps.rcnn_window(img, [10, 8, 30, 25], 'warp', 8, 2)[0])
    with pytest.raises(ValueError):
        rcnn_img_crop(img, np.array([100., 100., 120., 120.]), 'warp', 8, 2, mean)


class _Blob(object):
    def __init__(self):
        self.data = np.zeros((1,), np.float32)

    def reshape(self, *shape):
        self.data = np.zeros(shape, np.float32)


class _Net(object):
    """pycaffe's blob protocol around a one-line 'net': pool5 = data.mean(axis=(2,3))."""

    def __init__(self):
        self.blobs = {'data': _Blob(), 'pool5': _Blob(), 'cls_score': _Blob()}
        self.shapes = []

    def forward(self):
        d = self.blobs['data'].data
        self.shapes.append(d.shape)
        self.blobs['pool5'].data = d.mean(axis=(2, 3))
        self.blobs['cls_score'].data = d.max(axis=(2, 3))


def test_googlenet_features_with_a_fake_net():
    from vdetlib_amd.vdet.image_det import googlenet_features, googlenet_rcnn
    rng = np.random.RandomState(15)
    img = images()[1]
    x1, y1 = rng.uniform(1, 35, 130), rng.uniform(1, 25, 130)
    boxes = np.stack([x1, y1, x1 + rng.uniform(2, 25, 130), y1 + rng.uniform(2, 18, 130)], 1)
    net = _Net()
    got = googlenet_features(img, boxes, net, 'pool5')
    assert net.shapes == [(128, 3, 224, 224), (2, 3, 224, 224)]
    wp, wok = ps.rcnn_patches(img[None], boxes, None, 'warp', 224, 16, np.asarray(MEAN))
    assert wok.all()
    ref = _Net()
    want = []
    for b0 in (0, 128):
        ref.blobs['data'].reshape(*wp[b0:b0 + 128].shape)
        ref.blobs['data'].data[...] = wp[b0:b0 + 128]
        ref.forward()
        want.append(np.copy(ref.blobs['pool5'].data))
    want = np.concatenate(want)
    assert got.shape == (130, 3) and got.dtype == np.float32 and np.array_equal(got.view(np.int32), want.view(np.int32))
    assert np.array_equal(googlenet_rcnn(img, boxes[:3], _Net()), wp[:3].max(axis=(2, 3)))
    with pytest.raises(ValueError):
        googlenet_features(img, np.array([[100., 100., 120., 120.]]), _Net(), 'pool5')


def test_end_to_end_tubelets_to_patches_to_rescore():
    """Anchor-route tubelets -> tubelet_patches -> a one-line torch 'net' -> scatter through slot -> rescore_tubelets(floor=...)
    equals tests/rescore_spec.py given a floor built the same way from the spec's patches."""
    import rescore_spec
    import synth
    from vdetlib_amd import ops
    F, B, C, T, S, p = 5, 40, 2, 3, 8, 2
    boxes, scores = synth.coherent_video(77, F, B, C)
    imgs = np.random.RandomState(16).randint(0, 256, size=(F, synth.H, synth.W, 3)).astype(np.uint8)
    tb, ts, gi = g(boxes), g(scores), g(imgs)
    fr, ab, sc, _ = ops.top_anchors(tb, ts, T)
    tr, an, nt = ops.track_from_anchors(tb, fr, ab, sc)
    out = ops.tubelet_patches(gi, tr, nt, (0, F), C * T * F, crop_size=S, padding=p)
    n = int(out['count'])
    assert n > F                                                      # tubelets that run through the video
    net = lambda patches: patches.mean((1, 2, 3))

    def floor_of(patches, slot):
        c, t, f = slot.long().unbind(1)
        series = torch.full((C, T, F), float('nan'), dtype=torch.float64, device=DEV)
        series[c, t, f] = net(patches).double()
        return series
    series = floor_of(out['patches'][:n], out['slot'][:n])
    det, pooled, tboxes, src = ops.rescore_tubelets(tr, nt, tb, ts, floor=series)
    # the same, from the spec's patches
    trn, ntn = tr.cpu().numpy(), nt.cpu().numpy()
    slots = ps.tubelet_slots(trn, ntn, 0, F)
    assert np.array_equal(out['slot'][:n].cpu().numpy(), slots)
    wp, wok = ps.rcnn_patches(imgs, np.stack([trn[c, t, f, :4] for c, t, f in slots]), slots[:, 2], 'warp', S, p, np.asarray(MEAN))
    assert wok.sum() > F and torch.equal(out['ok'][:n].cpu(), torch.from_numpy(wok))
    wseries = floor_of(g(wp), g(slots))
    assert torch.equal(torch.nan_to_num(series, nan=-7.0), torch.nan_to_num(wseries, nan=-7.0))
    wdet, wpooled, wtb, wsrc, eindex = rescore_spec.spec(trn, ntn, boxes, scores, floor=wseries.cpu().numpy())
    assert not eindex
    assert np.array_equal(det.cpu().numpy(), wdet, equal_nan=True) and np.array_equal(pooled.cpu().numpy(), wpooled, equal_nan=True)
    assert np.array_equal(tboxes.cpu().numpy(), wtb, equal_nan=True) and np.array_equal(src.cpu().numpy(), wsrc)
