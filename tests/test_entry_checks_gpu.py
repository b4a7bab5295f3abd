"""-m gpu: the device checks of ops.py's entry points with the first tensor ON the GPU.  nms_volume, det_nms_volume,
nms_volume_ordered, track_volume, nms_track_volume and video_batch used to look at ``boxes`` alone and hand the other tensors'
``data_ptr()`` to the kernels wherever they lived.  Every refusal here is provoked with a stand-in context (test_entry_checks_cpu)
through which nothing can be launched, so no kernel ever sees a host pointer; the valid calls that follow show that the guards
leave the results as they were.  Shapes: F = 2, B = 4, C = 2, T = 2, images [2,8,8,3]."""
import numpy as np
import pytest

import synth
from test_entry_checks_cpu import F, B, C, StandInCtx, entry_points, host_inputs, refused

pytestmark = pytest.mark.gpu


def _on_gpu(d, but=()):
    """the tensors of ``d`` on the GPU, except those named in ``but``"""
    import torch
    return {k: v.cuda() if torch.is_tensor(v) and k not in but else v for k, v in d.items()}


@pytest.mark.parametrize("name,host", [
    # the six that checked ``boxes`` alone
    ('nms_volume', 'scores'), ('nms_volume FCB', 'scores'), ('det_nms_volume', 'scores'), ('nms_volume_ordered', 'order'),
    ('nms_volume_ordered', 'ncand'), ('track_volume', 'scores'), ('nms_track_volume', 'scores'), ('video_batch', 'scores'),
    # one consumer of each reader: volume (alone, and behind tubelets), anchor slots, images
    ('top_anchors', 'scores'), ('rescore_tracks', 'scores'), ('rescore_tracks', 'ntracks'), ('track_from_anchors', 'aboxes'),
    ('track_from_anchors', 'ascores'), ('track_pixels', 'aframes'), ('track_pixels', 'images'), ('track_volume_pixels', 'boxes'),
    ('track_volume_pixels', 'images')])
def test_a_second_tensor_in_host_memory_is_refused_before_the_library(name, host):
    d = _on_gpu(host_inputs(), but=(host,))
    assert not d[host].is_cuda and d['ntracks' if host != 'ntracks' else 'boxes'].is_cuda
    assert 'same GPU' in refused(entry_points(d, StandInCtx())[name])


@pytest.fixture(scope="module")
def case():
    import torch
    boxes, scores = synth.coherent_video(4242, F, B, C)
    return boxes, scores, torch.from_numpy(boxes).cuda(), torch.from_numpy(scores).cuda()


def _eq(a, b):
    import torch
    if not a.is_floating_point():
        return torch.equal(a, b)
    return a.shape == b.shape and torch.equal(a.nan_to_num(-7.0), b.nan_to_num(-7.0))


def test_nms_volume_and_ordered_happy_path(oracle, case):
    from vdetlib_amd import ops
    boxes, scores, tb, ts = case
    idx, cnt = ops.nms_volume(tb, ts)
    widx, wcnt = oracle.nms_volume(boxes, scores, 0.3)
    assert np.array_equal(cnt.cpu().numpy(), wcnt) and np.array_equal(idx.cpu().numpy(), widx)
    idx2, cnt2 = ops.nms_volume(tb, ts.transpose(1, 2).contiguous(), layout='FCB')
    assert _eq(idx2, idx) and _eq(cnt2, cnt)
    order, ncand = ops.argsort_volume(ts)
    oidx, ocnt = ops.nms_volume_ordered(tb, order, ncand)
    assert _eq(oidx, idx) and _eq(ocnt, cnt)


def test_det_nms_volume_happy_path(oracle, case):
    import torch
    from vdetlib_amd import ops
    from test_detnms_gpu import _check_frame
    boxes, scores, _, ts = case
    BX = np.ascontiguousarray(np.stack([boxes, boxes + np.float32(2)], axis=2))            # [F,B,K,4]: every class its own boxes
    out = [t.cpu().numpy() for t in ops.det_nms_volume(torch.from_numpy(BX).cuda(), ts)]
    for f in range(F):
        _check_frame(oracle, f, scores, BX.reshape(F, B, 4 * C), out, 0.05, 100, 0.3)
    assert int(out[2][:, 1].sum()) > 0


def test_track_volume_and_nms_track_volume_happy_path(oracle, case):
    from vdetlib_amd import ops
    boxes, scores, tb, ts = case
    tr, an, nt = ops.track_volume(tb, ts)
    for c in range(C):
        wt, wa, wn = oracle.greedy_track_volume(boxes, scores[:, :, c], 0.3, 0.0, 10, 0.5, 0)
        assert int(nt[c]) == wn and wn > 0, (c, int(nt[c]), wn)
        assert np.array_equal(an[c, :wn].cpu().numpy(), wa[:wn]), c
        assert np.array_equal(tr[c, :wn].cpu().numpy(), wt[:wn], equal_nan=True), c
    idx, cnt = ops.nms_volume(tb, ts)
    ki, kc, tr2, an2, nt2 = ops.nms_track_volume(tb, ts)
    assert _eq(ki, idx) and _eq(kc, cnt) and _eq(tr2, tr) and _eq(an2, an) and _eq(nt2, nt)


def test_video_batch_happy_path(case):
    import torch
    from vdetlib_amd import ops
    _, _, tb, ts = case
    out = ops.video_batch(tb, ts, [0, F])
    ki, kc, tr, an, nt = ops.nms_track_volume(tb, ts)
    det, pool, bx = ops.rescore_tracks(tr, nt, tb, ts)
    assert torch.equal(out['keep_cnt'], kc) and torch.equal(out['keep_idx'], ki) and torch.equal(out['ntracks'][0], nt)
    for c in range(C):
        n = int(nt[c])
        assert n > 0 and _eq(out['anchors'][0, c, :n], an[c, :n]) and _eq(out['tracks'][0][c, :n], tr[c, :n]), c
        assert _eq(out['det'][0][c, :n], det[c, :n]) and _eq(out['pooled'][0][c, :n], pool[c, :n]), c
        assert _eq(out['tboxes'][0][c, :n], bx[c, :n]), c
