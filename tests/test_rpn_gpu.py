"""GPU: ops.rpn_proposals against the numpy rule (rpn_spec.py) on the shared case list (rpn_cases.py) -- every output bit for
bit, no tolerance --, the asynchronous form, independence of the calls before, the argument checks, and the hand-over to
ops.roi_pool and ops.det_nms_volume_deltas."""
import numpy as np
import pytest
import torch

import rpn_cases

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
OUTPUTS = ('rois', 'scores', 'index', 'count', 'cand_index', 'cand_cnt')


def g(a):
    return torch.from_numpy(np.array(a)).cuda()          # (a copy: the cases are read-only)


def bits(a):
    a = np.asarray(a)
    return a.view(np.int32) if a.dtype == F32 else a


def device_inputs(c):
    A = c['scores'].shape[1]
    scores = g(c['cls'])[:, A:] if c['cls'] is not None else g(c['scores'])
    return scores, g(c['deltas'])


def run(c, **extra):
    from vdetlib_amd import ops
    scores, deltas = device_inputs(c)
    kw = dict(c['kw'], return_candidates=True)
    kw.update(extra)
    return ops.rpn_proposals(scores, deltas, c['anchors'], c['im_size'], **kw)


def assert_equals_rule(got, name):
    want = rpn_cases.want(name)
    for k in OUTPUTS:
        a, b = got[k].cpu().numpy(), want[k]
        assert a.dtype == b.dtype and a.shape == b.shape, (name, k, a.dtype, a.shape)
        if not np.array_equal(bits(a), bits(b)):
            bad = np.argwhere(bits(a) != bits(b))
            raise AssertionError("%s: %s differs at %d places, first %s: got %s, want %s"
                                 % (name, k, len(bad), bad[0], a[tuple(bad[0])], b[tuple(bad[0])]))


@pytest.mark.parametrize('name', rpn_cases.names())
def test_every_output_equals_the_rule(name, oracle):
    c = rpn_cases.case(name)
    got = run(c)
    assert_equals_rule(got, name)
    if c['cls'] is not None:
        scores, _ = device_inputs(c)
        assert not scores.is_contiguous()        # the strided half went in as it is


def test_async_then_sync_gives_the_same_bits(oracle):
    from vdetlib_amd import _lib
    for name in ('random_small', 'tie_quant4', 'few_candidates'):
        got = run(rpn_cases.case(name), sync=False)
        _lib.get_context(torch.cuda.current_device()).sync()
        assert_equals_rule(got, name)


def test_a_small_call_after_a_large_one(oracle):
    """the context's scratch (keys, boxes, candidates, the NMS's graph) holds the large call's data when the small one starts"""
    for big, small in (('big_16384', 'knife_edge'), ('big_6000', 'few_candidates'), ('many_anchors', 'one_anchor'),
                       ('big_6000', 'empty_frame')):
        run(rpn_cases.case(big))
        assert_equals_rule(run(rpn_cases.case(small)), small)
    # ... and the same call twice, with another op of the prep cache's in between
    from vdetlib_amd import ops
    c = rpn_cases.case('random_small')
    first = run(c)
    boxes = first['rois'][:, :8].contiguous().nan_to_num(0.0)
    ops.nms_volume(boxes, torch.rand((boxes.shape[0], 8, 2), device='cuda'), 0.3)
    assert_equals_rule(run(c), 'random_small')


def test_without_candidates_output(oracle):
    from vdetlib_amd import ops
    c = rpn_cases.case('tie_quant4')
    scores, deltas = device_inputs(c)
    got = ops.rpn_proposals(scores, deltas, g(c['anchors']), c['im_size'], **c['kw'])
    assert sorted(got) == ['count', 'index', 'rois', 'scores']
    want = rpn_cases.want('tie_quant4')
    for k in got:
        assert np.array_equal(bits(got[k].cpu().numpy()), bits(want[k]))


def test_bad_arguments_raise_and_leave_the_context_usable(oracle):
    from vdetlib_amd import ops
    c = rpn_cases.case('random_small')
    s, d = device_inputs(c)
    an, im, kw = c['anchors'], c['im_size'], c['kw']
    F, A, Hf, Wf = s.shape
    z = lambda *shape: torch.zeros(shape, dtype=torch.float32, device='cuda')
    bad = [
        lambda: ops.rpn_proposals(s.double(), d, an, im, **kw),                              # dtypes
        lambda: ops.rpn_proposals(s, d.half(), an, im, **kw),
        lambda: ops.rpn_proposals(s, d, an.astype(F32), im, **kw),
        lambda: ops.rpn_proposals(s, d, g(an).float(), im, **kw),
        lambda: ops.rpn_proposals(s[0], d, an, im, **kw),                                    # shapes
        lambda: ops.rpn_proposals(s, d[:, :-4], an, im, **kw),
        lambda: ops.rpn_proposals(s, d[:1], an, im, **kw),
        lambda: ops.rpn_proposals(s, d, an[:8], im, **kw),
        lambda: ops.rpn_proposals(s, d, an, (0, 112), **kw),
        lambda: ops.rpn_proposals(s, d, an, 80, **kw),
        lambda: ops.rpn_proposals(s.cpu(), d.cpu(), an, im, **kw),                           # devices
        lambda: ops.rpn_proposals(s, d.cpu(), an, im, **kw),
        lambda: ops.rpn_proposals(z(1, 65, 2, 2), z(1, 260, 2, 2), np.zeros((65, 4)), im, **kw),      # limits
        lambda: ops.rpn_proposals(z(1, 1, 1, 1).expand(1, 64, 512, 512), z(1, 1, 1, 1).expand(1, 256, 512, 512), np.zeros((64, 4)), im, **kw),
        lambda: ops.rpn_proposals(z(1, 1, 0, 3), z(1, 4, 0, 3), np.zeros((1, 4)), im, **kw),
        lambda: ops.rpn_proposals(s, d, an, im, stride=0, **kw),
        lambda: ops.rpn_proposals(s, d, an, im, stride=1.5, **kw),
        lambda: ops.rpn_proposals(s, d, an, im, pre_nms_top_n=16385, post_nms_top_n=20),
        lambda: ops.rpn_proposals(s, d, an, im, pre_nms_top_n=10, post_nms_top_n=20),
        lambda: ops.rpn_proposals(s, d, an, im, pre_nms_top_n=10, post_nms_top_n=0),
        lambda: ops.rpn_proposals(s, d, an, im, min_size=float('nan'), **kw),
        lambda: ops.rpn_proposals(s, d, an, im, min_size=float('inf'), **kw),
        lambda: ops.rpn_proposals(s, d, an, im, offset=float('inf'), **kw),
        lambda: ops.rpn_proposals(s, d, an, im, dw_max=float('nan'), **kw),
    ]
    for i, fn in enumerate(bad):
        with pytest.raises(ValueError):
            fn()
            pytest.fail("case %d did not raise" % i)
    assert_equals_rule(run(c), 'random_small')
    # F = 0 is legal and launches nothing
    out = ops.rpn_proposals(s[:0], d[:0], an, im, **kw)
    assert tuple(out['rois'].shape) == (0, kw['post_nms_top_n'], 4) and tuple(out['count'].shape) == (0,)


def test_c_abi_limits_return_einval(oracle):
    """the C entry point refuses what the python front end refuses, by itself"""
    from vdetlib_amd import _lib
    ctx = _lib.get_context(torch.cuda.current_device())
    c = rpn_cases.case('random_small')
    s, d = device_inputs(c)
    an = g(c['anchors'])
    post, pre = 20, 100
    o = dict(rois=torch.empty((3, post, 4), device='cuda'), sc=torch.empty((3, post), device='cuda'),
             ix=torch.empty((3, post), dtype=torch.int32, device='cuda'), n=torch.empty(3, dtype=torch.int32, device='cuda'))

    def call(A=9, Hf=5, Wf=7, H=80, W=112, stride=16, pre=pre, post=post, min_size=16.0, sstride=315, F=3):
        return ctx.lib.vdet_rpn_proposals(ctx.h, s.data_ptr(), sstride, d.data_ptr(), an.data_ptr(), F, A, Hf, Wf, H, W, stride, pre, post,
                                          0.7, min_size, 1.0, 0, 0.0, o['rois'].data_ptr(), o['sc'].data_ptr(), o['ix'].data_ptr(),
                                          o['n'].data_ptr(), None, None)
    for kw in (dict(A=0), dict(A=65), dict(Hf=0), dict(Wf=0), dict(Hf=4096, Wf=4096), dict(F=2 ** 23), dict(stride=0), dict(pre=16385),
               dict(post=0), dict(post=101), dict(H=0), dict(W=0), dict(min_size=float('nan')), dict(sstride=314)):
        assert call(**kw) == _lib.VDET_EINVAL, kw
    assert call() == 0
    ctx.sync()
    assert_equals_rule(dict(rois=o['rois'], scores=o['sc'], index=o['ix'], count=o['n'], cand_index=run(c)['cand_index'],
                            cand_cnt=run(c)['cand_cnt']), 'random_small')


def test_result_feeds_roi_pool_and_the_per_class_nms(oracle):
    from vdetlib_amd import ops
    for name in ('few_candidates', 'empty_frame', 'random_small'):
        c = rpn_cases.case(name)
        out = run(c)
        F, post = out['index'].shape
        count = out['count'].cpu().numpy()
        H, W = c['im_size']
        gen = torch.Generator().manual_seed(5)
        feat = torch.randn((F, 6, H // 16, W // 16), generator=gen).cuda()
        img = torch.arange(F, dtype=torch.int32, device='cuda').repeat_interleave(post)
        full = ops.roi_pool(feat, out['rois'].view(-1, 4), img, pooled=(3, 3))
        valid = (torch.arange(post, device='cuda')[None, :] < out['count'][:, None]).reshape(-1)
        plain = torch.from_numpy(np.concatenate([rpn_cases.want(name)['rois'][f, :count[f]] for f in range(F)])).cuda()
        pidx = torch.from_numpy(np.repeat(np.arange(F), count).astype(np.int32)).cuda()
        compact = ops.roi_pool(feat, plain, pidx, pooled=(3, 3))
        assert torch.equal(full['ok'].bool(), valid) and compact['ok'].all()
        assert torch.equal(full['pooled'][valid], compact['pooled'])
        assert not full['pooled'][~valid].any()
        # the per-class NMS: the NaN-padded rois as they are (rows behind the count carry NaN scores, as documented there)
        K = 3
        scores = torch.rand((F, post, K), generator=gen).cuda()
        scores[~valid.view(F, post)] = float('nan')
        deltas = (torch.randn((F, post, 4 * K), generator=gen) * 0.1).cuda()
        got = ops.det_nms_volume_deltas(out['rois'], scores, deltas, c['im_size'], score_thresh=0.1, topk=16)
        for f in range(F):
            n = int(count[f])
            if n == 0:
                assert not got[2][f].any() and not got[4][f].any()
                continue
            rows = g(rpn_cases.want(name)['rois'][f:f + 1, :n])
            one = ops.det_nms_volume_deltas(rows, scores[f:f + 1, :n].contiguous(), deltas[f:f + 1, :n].contiguous(), c['im_size'],
                                            score_thresh=0.1, topk=16)
            for a, b in zip(got, one):
                assert torch.equal(a[f:f + 1].view(torch.int32) if a.dtype == torch.float32 else a[f:f + 1],
                                   b.view(torch.int32) if b.dtype == torch.float32 else b)
