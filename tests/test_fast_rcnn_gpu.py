"""GPU: the dict level of the Fast R-CNN route (vdet/image_det.py: im_detect, fast_rcnn_det; vdet/tubelet_cls.py: fast_rcnn_cls;
vdet/video_det.py: fast_rcnn_det_vid with im_detect as its det_fun) with a toy net: a fixed-weight 3 x 3 stride-4 convolution
as the backbone and a fixed linear head.  The head's matmul is not under test: the expected scores go through the identical
torch head, on the same device, on input pooled by tests/roipool_spec.py."""
import functools

import numpy as np
import pytest
import torch

import roipool_spec as rs

pytestmark = pytest.mark.gpu

DEV = 'cuda'
H, W, NCLS, K = 40, 56, 4, 5
CLASS_NAMES = ('__background__', 'a', 'b', 'c')


class ToyNet(object):
    spatial_scale = 0.25
    pooled = (3, 3)

    def __init__(self, roi_mode='max'):
        gen = torch.Generator().manual_seed(90)
        self.roi_mode = roi_mode
        self.w = (torch.randn(K, 3, 3, 3, generator=gen) * 0.05).to(DEV)
        self.ws = (torch.randn(K * 9, NCLS, generator=gen) * 0.01).to(DEV)
        self.wd = (torch.randn(K * 9, 4 * NCLS, generator=gen) * 0.002).to(DEV)
        self.mean = torch.tensor([103.939, 116.779, 123.68], device=DEV).view(1, 3, 1, 1)

    def prepare(self, img):
        """uint8 [H,W,3] -> ([1,3,2H,2W] minus the mean, 2.0): a nearest-neighbour doubling stands for the caller's resize."""
        x = torch.from_numpy(np.ascontiguousarray(img)).to(DEV).permute(2, 0, 1)[None].float() - self.mean
        return torch.nn.functional.interpolate(x, scale_factor=2, mode='nearest'), 2.0

    def backbone(self, x):
        return torch.nn.functional.conv2d(x, self.w, stride=4, padding=1)

    def head(self, pooled):
        flat = pooled.reshape(len(pooled), -1)
        return torch.softmax(flat @ self.ws, 1), flat @ self.wd


@functools.lru_cache(maxsize=None)
def frames():
    return np.random.RandomState(91).randint(0, 256, size=(3, H, W, 3)).astype(np.uint8)


def some_boxes(seed, n):
    rng = np.random.RandomState(seed)
    x1, y1 = rng.uniform(-3, W - 8, n), rng.uniform(-3, H - 8, n)
    return np.stack([x1, y1, x1 + rng.uniform(2, 30, n), y1 + rng.uniform(2, 24, n)], 1)


def expected(net, img, boxes):
    """Spec pooling of the net's own feature map + the same head on the same device + the loop decode."""
    with torch.no_grad():
        x, im_scale = net.prepare(img)
        feat = net.backbone(x)
        wp, wok = rs.roi_pool(feat.cpu().numpy(), boxes, None, net.spatial_scale, net.pooled, im_scale, net.roi_mode)
        assert wok.all()
        scores, deltas = net.head(torch.from_numpy(wp).to(DEV))
    scores, deltas = scores.cpu().numpy(), deltas.cpu().numpy()
    return scores, rs.clip_boxes_loop(rs.bbox_transform_inv_loop(boxes, deltas), img.shape)


@pytest.mark.parametrize('roi_mode', ['max', 'align'])
def test_im_detect_and_fast_rcnn_det(roi_mode):
    from vdetlib_amd.vdet.image_det import fast_rcnn_det, im_detect
    net = ToyNet(roi_mode)
    img, boxes = frames()[0], some_boxes(92, 17)
    scores, pred = im_detect(net, img, boxes)
    ws, wp = expected(net, img, boxes)
    assert scores.shape == (17, NCLS) and pred.shape == (17, 4 * NCLS) and pred.dtype == np.float64
    assert np.array_equal(scores, ws) and np.array_equal(pred, wp)
    assert pred.min() >= 0 and pred[:, 0::2].max() <= W - 1 and pred[:, 1::2].max() <= H - 1
    assert np.array_equal(fast_rcnn_det(img, boxes.tolist(), net), ws)
    with pytest.raises(ValueError):
        im_detect(net, img, np.array([[1, 2, np.nan, 4.]]))


def test_fast_rcnn_cls_returns_the_reference_structure():
    from vdetlib_amd.utils.protocol import bbox_hash
    from vdetlib_amd.vdet.tubelet_cls import fast_rcnn_cls
    net = ToyNet()
    imgs = frames()
    b = some_boxes(93, 7)
    vid = {'video': 'toy', 'frames': [{'frame': f, 'path': '%d.JPEG' % f} for f in (1, 2, 3)], 'root_path': '/nowhere'}
    # track 0 lives in frames 1-3, track 1 in 2 only, track 2 in 1 and 3, track 3 nowhere
    tracks = [[{'frame': 1, 'bbox': b[0].tolist()}, {'frame': 2, 'bbox': b[1].tolist()}, {'frame': 3, 'bbox': b[2].tolist()}],
              [{'frame': 2, 'bbox': b[3].tolist()}],
              [{'frame': 1, 'bbox': b[4].tolist()}, {'frame': 3, 'bbox': b[5].tolist()}], []]
    got = fast_rcnn_cls(vid, {'video': 'toy', 'tracks': tracks}, net, 2, images={f: imgs[f - 1] for f in (1, 2, 3)})
    assert [[box['frame'] for box in tr] for tr in got] == [[1, 2, 3], [2], [1, 3], []]
    for f in (1, 2, 3):
        rows = [(i, box['bbox']) for i, tr in enumerate(tracks) for box in tr if box['frame'] == f]
        ws, wp = expected(net, imgs[f - 1], np.asarray([r[1] for r in rows]))
        for (i, _), s, p in zip(rows, ws, wp):
            box = [x for x in got[i] if x['frame'] == f][0]
            assert sorted(box) == ['bbox', 'frame', 'hash', 'score']
            assert box['bbox'] == list(p) and box['score'] == s[2] and box['hash'] == bbox_hash('toy', f, p)


def test_fast_rcnn_det_vid_with_im_detect_as_det_fun(monkeypatch):
    from vdetlib_amd.vdet import video_det
    from vdetlib_amd.vdet.image_det import im_detect
    net = ToyNet()
    imgs = frames()
    vid = {'video': 'toy', 'frames': [{'frame': f, 'path': '%d' % f} for f in (1, 2, 3)], 'root_path': ''}
    monkeypatch.setattr(video_det, 'imread', lambda path: imgs[int(path) - 1])
    per_frame = {f: some_boxes(94 + f, 9) for f in (1, 2, 3)}
    box_proto = {'video': 'toy', 'boxes': [{'frame': f, 'bbox': bb.tolist()} for f in (1, 2, 3) for bb in per_frame[f]]}
    all_boxes = video_det.fast_rcnn_det_vid(net, vid, box_proto, im_detect, class_names=CLASS_NAMES, max_per_image=5, thresh=0.2)
    assert len(all_boxes) == NCLS and all(len(per_cls) == 3 for per_cls in all_boxes)
    filled = 0
    for i, f in enumerate((1, 2, 3)):
        ws, wp = expected(net, imgs[f - 1], per_frame[f])
        assert len(all_boxes[0][i]) == 0
        for j in range(1, NCLS):
            got = all_boxes[j][i]
            keep = np.flatnonzero(ws[:, j] > 0.2)
            assert got.dtype == np.float32 and got.shape == (min(len(keep), 5), 5)
            rows = {tuple(r) for r in np.concatenate((wp[keep, 4 * j:4 * j + 4], ws[keep, j, None]), 1).astype(np.float32)}
            assert {tuple(r) for r in got} <= rows
            filled += len(got)
    assert filled > 9
