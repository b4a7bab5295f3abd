"""GPU: the dict level of the device Fast R-CNN route (vdet/video_det.py: fast_rcnn_det_vid_device) against the host route
(fast_rcnn_det_vid with image_det.im_detect as its det_fun) with test_fast_rcnn_gpu.py's toy net (copied): the same rows, scores
bit for bit, box coordinates under the decode's condition -- at most one element in 10^4 differs, and then by one f32 ulp."""
import functools

import numpy as np
import pytest
import torch

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


NF = 5
COUNTS = (9, 14, 3, 14, 1)           # proposals per frame: the chunks are padded to their largest frame


@functools.lru_cache(maxsize=None)
def frames():
    return np.random.RandomState(91).randint(0, 256, size=(NF, H, W, 3)).astype(np.uint8)


def some_boxes(seed, n):
    rng = np.random.RandomState(seed)
    x1, y1 = rng.uniform(-3, W - 8, n), rng.uniform(-3, H - 8, n)
    return np.stack([x1, y1, x1 + rng.uniform(2, 30, n), y1 + rng.uniform(2, 24, n)], 1)


def protos():
    ids = tuple(range(1, NF + 1))
    vid = {'video': 'toy', 'frames': [{'frame': f, 'path': '%d' % f} for f in ids], 'root_path': ''}
    per_frame = {f: some_boxes(94 + f, COUNTS[f - 1]) for f in ids}
    box_proto = {'video': 'toy', 'boxes': [{'frame': f, 'bbox': bb.tolist()} for f in ids for bb in per_frame[f]]}
    return vid, box_proto


def rows_equal(got, want):
    """(rows compared, box elements that differ): same shape, scores bit for bit, a differing coordinate by one f32 ulp"""
    got, want = np.asarray(got, np.float32).reshape(-1, 5), np.asarray(want, np.float32).reshape(-1, 5)
    assert got.shape == want.shape
    assert np.array_equal(got[:, 4].view(np.int32), want[:, 4].view(np.int32))
    ne = got[:, :4] != want[:, :4]
    assert np.all(np.abs(got[:, :4][ne].view(np.int32) - want[:, :4][ne].view(np.int32)) == 1)
    return got[:, :4].size, int(ne.sum())


@pytest.mark.parametrize('chunk', [2, 8])
def test_device_route_equals_the_host_route(monkeypatch, chunk):
    from vdetlib_amd.vdet import video_det
    from vdetlib_amd.vdet.image_det import apply_image_nms, im_detect
    net = ToyNet()
    imgs = frames()
    vid, box_proto = protos()
    monkeypatch.setattr(video_det, 'imread', lambda path: imgs[int(path) - 1])
    total = differ = rows = 0
    for max_per_image, thresh in ((100, 0.2), (5, 0.2), (100, 0.26)):
        want = video_det.fast_rcnn_det_vid(net, vid, box_proto, im_detect, class_names=CLASS_NAMES, max_per_image=max_per_image,
                                           thresh=thresh)
        got = video_det.fast_rcnn_det_vid_device(net, vid, box_proto, class_names=CLASS_NAMES, max_per_image=max_per_image,
                                                 thresh=thresh, chunk=chunk)
        both, keeps = video_det.fast_rcnn_det_vid_device(net, vid, box_proto, class_names=CLASS_NAMES, max_per_image=max_per_image,
                                                         thresh=thresh, chunk=chunk, nms_thresh=0.3,
                                                         images={f: imgs[f - 1] for f in range(1, NF + 1)})
        assert len(got) == NCLS and all(len(per_cls) == NF for per_cls in got)
        for i in range(NF):
            assert len(got[0][i]) == 0
            for j in range(1, NCLS):
                assert got[j][i].dtype == np.float32 and got[j][i].ndim == 2
                n, d = rows_equal(got[j][i], want[j][i])
                total += n; differ += d; rows += len(got[j][i])
                assert np.array_equal(both[j][i], got[j][i])
                if len(got[j][i]):
                    assert keeps[j][i] == list(apply_image_nms(got[j][i][:, :4], got[j][i][:, 4], 0.3))
                else:
                    assert keeps[j][i] == []
    assert rows > 40 and differ * 10 ** 4 <= total


def test_device_route_errors(monkeypatch):
    from vdetlib_amd.vdet import video_det
    net = ToyNet()
    imgs = frames()
    vid, box_proto = protos()
    images = {f: imgs[f - 1] for f in range(1, NF + 1)}
    with pytest.raises(ValueError):
        video_det.fast_rcnn_det_vid_device(net, vid, box_proto, class_names=CLASS_NAMES, max_per_image=129, images=images)
    bad = dict(box_proto, boxes=box_proto['boxes'] + [{'frame': 2, 'bbox': [1, 2, float('nan'), 4]}])
    with pytest.raises(ValueError):
        video_det.fast_rcnn_det_vid_device(net, vid, bad, class_names=CLASS_NAMES, images=images)
    narrow = dict(images)
    narrow[3] = imgs[2][:, :40]
    with pytest.raises(ValueError):
        video_det.fast_rcnn_det_vid_device(net, vid, box_proto, class_names=CLASS_NAMES, images=narrow)
