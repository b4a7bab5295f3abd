"""GPU: the dict level of the Faster R-CNN route with a tiny seeded torch net (one strided conv backbone, a 3x3 + 1x1 RPN head, a
linear head; frames of 64 x 96): proposal.rpn_vid_proposals against the numpy rule (rpn_spec.py) applied to the net's own RPN
outputs, and video_det.faster_rcnn_det_vid_device against fast_rcnn_det_vid_device fed that box_proto."""
import functools

import numpy as np
import pytest
import torch

import rpn_spec

pytestmark = pytest.mark.gpu

DEV = 'cuda'
H, W, NCLS, K, A = 64, 96, 4, 6, 9
CLASS_NAMES = ('__background__', 'a', 'b', 'c')
NF = 5
RPN = dict(pre_nms_top_n=60, post_nms_top_n=30, nms_thresh=0.4, min_size=6)


class ToyNet(object):
    spatial_scale = 0.125
    feat_stride = 8
    pooled = (3, 3)
    roi_mode = 'max'

    def __init__(self):
        gen = torch.Generator().manual_seed(190)
        r = lambda *shape: torch.randn(*shape, generator=gen)
        self.w = (r(K, 3, 3, 3) * 0.05).to(DEV)
        self.w_rpn = (r(K, K, 3, 3) * 0.2).to(DEV)
        self.w_cls = (r(2 * A, K, 1, 1) * 0.5).to(DEV)
        self.w_box = (r(4 * A, K, 1, 1) * 0.05).to(DEV)
        self.ws = (r(K * 9, NCLS) * 0.01).to(DEV)
        self.wd = (r(K * 9, 4 * NCLS) * 0.002).to(DEV)
        self.mean = torch.tensor([103.939, 116.779, 123.68], device=DEV).view(1, 3, 1, 1)
        self.anchors = rpn_spec.generate_anchors(base_size=8, scales=(1, 2, 4))

    def prepare(self, img):
        """uint8 [H,W,3] -> ([1,3,2H,2W] minus the mean, 2.0): a nearest-neighbour doubling stands for the caller's resize."""
        x = torch.from_numpy(np.ascontiguousarray(img)).to(DEV).permute(2, 0, 1)[None].float() - self.mean
        return torch.nn.functional.interpolate(x, scale_factor=2, mode='nearest'), 2.0

    def backbone(self, x):
        return torch.nn.functional.conv2d(x, self.w, stride=8, padding=1)

    def rpn(self, feat):
        """the foreground half of the two-way softmax, as a strided slice, and the deltas"""
        mid = torch.relu(torch.nn.functional.conv2d(feat, self.w_rpn, padding=1))
        cls = torch.nn.functional.conv2d(mid, self.w_cls)
        prob = torch.softmax(cls.view(1, 2, A, *cls.shape[2:]), 1).view_as(cls)
        return prob[:, A:], torch.nn.functional.conv2d(mid, self.w_box)

    def head(self, pooled):
        flat = pooled.reshape(len(pooled), -1)
        return torch.softmax(flat @ self.ws, 1), flat @ self.wd


@functools.lru_cache(maxsize=None)
def frames():
    rng = np.random.RandomState(191)
    # blocks of 8 x 8 pixels: a feature map with some structure, so that the RPN's scores are not all alike
    coarse = rng.randint(0, 256, size=(NF, H // 8, W // 8, 3))
    return np.clip(np.kron(coarse, np.ones((1, 8, 8, 1))) + rng.randint(-20, 21, size=(NF, H, W, 3)), 0, 255).astype(np.uint8)


def video():
    ids = tuple(range(1, NF + 1))
    return {'video': 'toy', 'frames': [{'frame': f, 'path': '%d' % f} for f in ids], 'root_path': ''}, {f: frames()[f - 1] for f in ids}


@functools.lru_cache(maxsize=None)
def rule_proposals():
    """the rule on the net's own RPN outputs, frame by frame as the dict level runs the net: per frame f64 [n,4] boxes in the
    original image's coordinates"""
    net = ToyNet()
    out = []
    for img in frames():
        with torch.no_grad():
            x, scale = net.prepare(img)
            s, d = net.rpn(net.backbone(x).contiguous())
        want = rpn_spec.proposals(s.contiguous().cpu().numpy(), d.cpu().numpy(), net.anchors, tuple(x.shape[2:]), stride=net.feat_stride,
                                  **dict(RPN, min_size=RPN['min_size'] * scale))
        out.append(want['rois'][0, :want['count'][0]].astype(np.float64) / scale)
    return out


@pytest.mark.parametrize('chunk', [2, 8])
def test_rpn_vid_proposals_equals_the_rule(chunk, oracle):
    from vdetlib_amd.utils.protocol import bbox_hash, boxes_at_frame
    from vdetlib_amd.vdet import proposal
    import vdetlib.vdet.proposal as alias
    assert alias is proposal
    vid, images = video()
    want = rule_proposals()
    assert 5 < min(len(w) for w in want) and sum(len(w) for w in want) < NF * RPN['post_nms_top_n']     # neither empty nor all full
    net = ToyNet()
    exact = proposal.rpn_vid_proposals(net, vid, chunk=chunk, images=images, integer_boxes=False, **RPN)
    trunc = proposal.rpn_vid_proposals(net, vid, chunk=chunk, images=images, **RPN)
    assert exact['video'] == trunc['video'] == 'toy'
    for f in range(1, NF + 1):
        got = boxes_at_frame(exact, f)
        assert np.array_equal(np.array([b['bbox'] for b in got], np.float64).reshape(-1, 4), want[f - 1])
        assert all(b['hash'] == bbox_hash('toy', f, w) for b, w in zip(got, want[f - 1]))
        got = boxes_at_frame(trunc, f)
        assert [b['bbox'] for b in got] == [[int(v) for v in w] for w in want[f - 1]]
        assert all(type(v) is int for b in got for v in b['bbox'])
    with pytest.raises(RuntimeError):
        proposal.vid_proposals(vid)


@pytest.mark.parametrize('chunk', [2, 8])
def test_faster_route_equals_the_fast_route_on_its_own_proposals(chunk, oracle):
    from vdetlib_amd.vdet import proposal, video_det
    vid, images = video()
    net = ToyNet()
    box_proto = proposal.rpn_vid_proposals(net, vid, chunk=chunk, images=images, integer_boxes=False, **RPN)
    rpn = dict(RPN, rpn_nms_thresh=RPN['nms_thresh'])
    del rpn['nms_thresh']
    rows = 0
    for max_per_image, thresh in ((100, 0.2), (5, 0.2), (100, 0.26)):
        want, wkeeps = video_det.fast_rcnn_det_vid_device(net, vid, box_proto, class_names=CLASS_NAMES, max_per_image=max_per_image,
                                                          thresh=thresh, chunk=chunk, nms_thresh=0.3, images=images)
        got, keeps = video_det.faster_rcnn_det_vid_device(net, vid, class_names=CLASS_NAMES, max_per_image=max_per_image, thresh=thresh,
                                                          chunk=chunk, nms_thresh=0.3, images=images, **rpn)
        plain = video_det.faster_rcnn_det_vid_device(net, vid, class_names=CLASS_NAMES, max_per_image=max_per_image, thresh=thresh,
                                                     chunk=chunk, images=images, **rpn)
        assert len(got) == NCLS and all(len(per_cls) == NF for per_cls in got)
        for i in range(NF):
            assert len(got[0][i]) == 0
            for j in range(1, NCLS):
                assert got[j][i].dtype == np.float32 and got[j][i].shape == want[j][i].shape
                assert np.array_equal(got[j][i].view(np.int32), want[j][i].view(np.int32))
                assert np.array_equal(plain[j][i].view(np.int32), got[j][i].view(np.int32))
                assert keeps[j][i] == wkeeps[j][i]
                rows += len(got[j][i])
    assert rows > 40
    with pytest.raises(ValueError):
        video_det.faster_rcnn_det_vid_device(net, vid, class_names=CLASS_NAMES, max_per_image=129, images=images)
