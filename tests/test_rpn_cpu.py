"""CPU: the numpy rule of the RPN proposal layer (rpn_spec.py) -- the anchor table, the vectorised form against the plain loop on
every case of rpn_cases.py, the width term 1e-14 against decode_spec.decode, and the guards of the case list: conditions on
the rule's own output without which test_rpn_gpu.py could pass vacuously."""
import numpy as np
import pytest

import decode_cases
import decode_spec
import rpn_cases
import rpn_spec

F32, F64 = np.float32, np.float64
OUTPUTS = ('rois', 'scores', 'index', 'count', 'cand_index', 'cand_cnt', 'nms_cnt', 'tie_cut')

TABLE = [(-84, -40, 99, 55), (-176, -88, 191, 103), (-360, -184, 375, 199), (-56, -56, 71, 71), (-120, -120, 135, 135),
         (-248, -248, 263, 263), (-36, -80, 51, 95), (-80, -168, 95, 183), (-168, -344, 183, 359)]


def bits(a):
    a = np.asarray(a)
    return a.view(np.int32) if a.dtype == F32 else a


def test_generate_anchors_table():
    from vdetlib_amd import ops
    a = rpn_spec.generate_anchors()
    assert a.dtype == F64 and a.shape == (9, 4)
    assert np.array_equal(a, np.array(TABLE, F64))
    assert np.array_equal(ops.generate_anchors(), a)
    for kw in (dict(base_size=8), dict(ratios=(0.33, 1, 3.1), scales=(2, 5)), dict(base_size=15, ratios=(0.5,), scales=(1, 2, 4, 8))):
        assert np.array_equal(ops.generate_anchors(**kw), rpn_spec.generate_anchors(**kw))


@pytest.mark.parametrize('name', rpn_cases.names())
def test_vectorised_equals_loop(name, oracle):
    c = rpn_cases.case(name)
    if name == 'big_16384':
        # the inputs of big_6000 with another cut: the loop decodes every anchor again for nothing new but the sort's length, so
        # the loop runs on the first frame only
        sl = slice(0, 1)
    else:
        sl = slice(None)
    got = rpn_spec.proposals_loop(c['scores'][sl], c['deltas'][sl], c['anchors'], c['im_size'], **c['kw'])
    want = rpn_cases.want(name)
    for k in OUTPUTS:
        assert np.array_equal(bits(got[k]), bits(want[k][sl])), (name, k)


def test_offset_eps_is_the_fast_rcnn_decode():
    for name, rois, deltas, im_size in decode_cases.cases():
        r = np.asarray(rois, F64).reshape(-1, 4)
        d = np.asarray(deltas, F32).reshape(len(r), -1, 4)
        want = decode_spec.decode(rois, deltas, im_size).reshape(len(r), -1, 4)
        for k in range(d.shape[1]):
            got = rpn_spec.decode(r, d[:, k], im_size, offset=1e-14)
            assert np.array_equal(got.view(np.int32), want[:, k].view(np.int32)), (name, k)
            one = rpn_spec.decode_one(r[0], d[0, k], im_size, 1e-14, None)
            assert np.array_equal(np.array(one, F32).view(np.int32), want[0, k].view(np.int32)), (name, k)


def test_case_list_guards(oracle):
    w = {n: rpn_cases.want(n) for n in rpn_cases.names()}
    post = {n: rpn_cases.case(n)['kw']['post_nms_top_n'] for n in w}
    pre = {n: rpn_cases.case(n)['kw']['pre_nms_top_n'] for n in w}
    assert any((w[n]['nms_cnt'] > post[n]).any() for n in w)                                   # truncated at post
    assert any(((w[n]['count'] > 0) & (w[n]['count'] < post[n])).any() for n in w)             # 0 < count < post
    assert any(w[n]['tie_cut'].any() for n in w)                                               # the cut at pre inside a tie class
    assert w['tie_quant4']['tie_cut'].any() and w['tie_all_equal']['tie_cut'].all()
    assert any(((w[n]['cand_cnt'] > 0) & (4 * w[n]['nms_cnt'] <= 3 * w[n]['cand_cnt'])).any() for n in w)     # NMS removes a quarter
    assert any((w[n]['cand_cnt'] == pre[n]).all() for n in w)                                  # a full selection
    assert (w['few_candidates']['cand_cnt'][:2] < (post['few_candidates'], pre['few_candidates'])).all()
    assert w['few_candidates']['cand_cnt'][0] > 0
    assert w['empty_frame']['cand_cnt'][1] == 0 and w['empty_frame']['count'][1] == 0 and (w['empty_frame']['count'][[0, 2]] > 0).all()
    assert (w['pre_beyond_n']['cand_cnt'] < pre['pre_beyond_n']).all() and (w['pre_beyond_n']['cand_cnt'] > 0).all()
    # the knife edge falls on both sides: with one cell the flat index is the anchor's
    k = w['knife_edge']
    names = rpn_cases.KNIFE_NAMES
    assert sorted(k['cand_index'][0, :k['cand_cnt'][0]].tolist()) == [names.index('exact'), names.index('border_exact')]
    # the clamp changes the result, and so do the size filter and the width term
    assert not np.array_equal(bits(w['dw10_clamped']['rois']), bits(w['dw10_free']['rois']))
    assert (w['min_size_filter']['cand_cnt'] < w['pre_beyond_n']['cand_cnt']).all()
    assert not np.array_equal(bits(w['offset_eps']['rois']), bits(w['pre_beyond_n']['rois'][:, :post['offset_eps']]))
    # non-finite deltas give candidates with clipped coordinates and drop the NaN ones
    assert (w['nonfinite_deltas']['cand_cnt'] > 0).all()
    for n in w:
        cnt = w[n]['count']
        for f in range(len(cnt)):
            assert not np.isnan(w[n]['rois'][f, :cnt[f]]).any() and np.isnan(w[n]['rois'][f, cnt[f]:]).all()
            assert (w[n]['index'][f, cnt[f]:] == -1).all() and (w[n]['index'][f, :cnt[f]] >= 0).all()
