"""The one reader (ops._batch_read), field reader (ops._batch_field / ops._batch_flat) and view builder (ops._batch_views) of
video_batch's dict layout, on host tensors: every check is made on the host before anything is enqueued, so a wrong layout fails
as a layout and only a fully right one gets as far as the "same GPU" check.  V = 3 is the smallest batch with a middle view."""
import numpy as np
import pytest

OFF, C, T = (0, 1, 3, 6), 2, 3
PER = dict(tracks=5, det=1, pooled=1, tboxes=4)


def _host_batch(off=OFF):
    import torch
    from vdetlib_amd import ops
    off = np.asarray(off, dtype=np.int64)
    V, Ft = len(off) - 1, int(off[-1])
    dtype = dict(tracks=torch.float32, det=torch.float64, pooled=torch.float64, tboxes=torch.float32)
    bo = {k: ops._batch_views(torch.arange(C * T * Ft * per, dtype=dtype[k]), off, C, T, per) for k, per in PER.items()}
    bo.update(anchors=torch.zeros((V, C, T, 3)), ntracks=torch.zeros((V, C), dtype=torch.int32), frame_off=off)
    return bo


def _wrong_views(views, per):
    """name -> the list ``views`` (consecutive [C,T,F_v(,per)] views for OFF) made wrong in one way"""
    import torch
    tail = (per,) if per > 1 else ()
    n = C * T * per
    flat = torch.as_strided(views[0], (n * OFF[-1],), (1,))
    wide = torch.zeros((C, T, 4) + tail, dtype=views[1].dtype)
    other = torch.float64 if views[1].dtype == torch.float32 else torch.float32
    return {
        'middle view cloned': [views[0], views[1].clone(), views[2]],
        'first two re-split 2+1': [flat[:2 * n].view(C, T, 2, *tail), flat[2 * n:3 * n].view(C, T, 1, *tail), views[2]],
        'reversed': views[::-1],
        'one view not contiguous': [views[0], wide[:, :, ::2], views[2]],
        'one view of another dtype': [views[0], views[1].to(other), views[2]],
        'separate allocations': [x.clone() for x in views],
    }


WRONG = ('middle view cloned', 'first two re-split 2+1', 'reversed', 'one view not contiguous', 'one view of another dtype',
         'separate allocations')


def _layout_error(fn):
    with pytest.raises(ValueError) as e:
        fn()
    assert 'same GPU' not in str(e.value), str(e.value)
    return str(e.value)


@pytest.mark.parametrize("how", WRONG)
def test_reader_and_field_reader_refuse_wrong_views(how):
    import torch
    from vdetlib_amd import ops
    bo = _host_batch()
    b = ops._batch_read(bo, need=('anchors',))
    assert (b.V, b.Ft, b.C, b.T) == (3, 6, C, T) and b.off.dtype == np.int64 and b.tracks.data_ptr() == bo['tracks'][0].data_ptr()
    assert b.tracks.shape == (C * T * 6 * 5,) and b.anchors is bo['anchors'] and b.device == torch.device('cpu')
    _layout_error(lambda: ops._batch_read(dict(bo, tracks=_wrong_views(bo['tracks'], 5)[how])))
    for k, dt in (('det', torch.float64), ('tboxes', torch.float32)):
        assert ops._batch_field(b, bo[k], PER[k], (dt,), k, 'bo').data_ptr() == bo[k][0].data_ptr()
        msg = _layout_error(lambda: ops._batch_field(b, _wrong_views(bo[k], PER[k])[how], PER[k], (torch.float32, torch.float64), k, 'bo'))
        assert k in msg and 'bo' in msg


def test_batch_flat_compares_every_neighbour():
    """without shapes to go by (ops._batch_flat alone), a stray view anywhere in the list is still refused"""
    from vdetlib_amd import ops
    views = _host_batch()['det']
    assert ops._batch_flat(views, 1).data_ptr() == views[0].data_ptr()
    for how in ('middle view cloned', 'reversed', 'one view not contiguous', 'one view of another dtype', 'separate allocations'):
        _layout_error(lambda: ops._batch_flat(_wrong_views(views, 1)[how], 1))
    for bad in ([], None, views[0], [views[0], None]):
        _layout_error(lambda: ops._batch_flat(bad, 1))


def test_reader_refuses_wrong_frame_off_and_dicts():
    import torch
    from vdetlib_amd import ops
    bo = _host_batch()
    b4 = ops._batch_read(_host_batch((0, 1, 3, 5, 6)))
    assert b4.V == 4 and b4.anchors is None
    for off in ((0, 1, 3, 5, 6), (1, 3, 6), (1, 2, 4, 7), (0, 3, 3, 6), (0, 1, 3), (0,)):
        _layout_error(lambda: ops._batch_read(dict(bo, frame_off=np.asarray(off))))
    _layout_error(lambda: ops._batch_field(b4, bo['det'], 1, (torch.float64,), 'det', 'bo'))      # 3 views, frame_off of 5 entries
    for bad in (None, [], {k: v for k, v in bo.items() if k != 'ntracks'}, dict(bo, tracks=[]), dict(bo, tracks=bo['tracks'][0]),
                dict(bo, ntracks=bo['ntracks'].long()), dict(bo, ntracks=bo['ntracks'][:2]), dict(bo, ntracks=None)):
        assert "video_batch" in _layout_error(lambda: ops._batch_read(bad))
    for bad in ({k: v for k, v in bo.items() if k != 'anchors'}, dict(bo, anchors=bo['anchors'].double()),
                dict(bo, anchors=bo['anchors'][:, :, :2])):
        ops._batch_read(bad)                                                                      # fine where anchors are not needed
        _layout_error(lambda: ops._batch_read(bad, need=('anchors',)))
    assert "my_arg" in _layout_error(lambda: ops._batch_read(dict(bo, det=[]), 'my_arg', need=('det',)))


@pytest.mark.parametrize("per", [1, 4, 5])
def test_views_then_flat_is_the_identity(per):
    import torch
    from vdetlib_amd import ops
    off = np.asarray(OFF, dtype=np.int64)
    flat = torch.arange(C * T * 6 * per, dtype=torch.float32)
    views = ops._batch_views(flat, off, C, T, per)
    assert [tuple(x.shape) for x in views] == [(C, T, f) + ((per,) if per > 1 else ()) for f in (1, 2, 3)]
    for v, x in enumerate(views):
        assert x.is_contiguous() and x.data_ptr() == flat.data_ptr() + 4 * C * T * per * OFF[v]
    back = ops._batch_flat(views, per)
    assert back.data_ptr() == flat.data_ptr() and back.shape == flat.shape and torch.equal(back, flat)
    b = ops._batch_read(_host_batch())
    assert ops._batch_field(b, views, per, (torch.float32,), 'x', 'bo').data_ptr() == flat.data_ptr()
    if per == 1:                                                        # only the rows of a wide blob carry an axis of width 1
        rows = [x.unsqueeze(-1) for x in views]
        assert ops._batch_field(b, rows, 1, (torch.float32,), 'x', 'bo', axis=True).data_ptr() == flat.data_ptr()
        _layout_error(lambda: ops._batch_field(b, rows, 1, (torch.float32,), 'x', 'bo'))
        _layout_error(lambda: ops._batch_field(b, views, 1, (torch.float32,), 'x', 'bo', axis=True))
    two = ops._batch_views(torch.zeros(C * 2 * 6 * per), off, C, 2, per)                  # a field with its own slot count
    _layout_error(lambda: ops._batch_field(b, two, per, (torch.float32,), 'x', 'bo'))
    assert ops._batch_field(b, two, per, (torch.float32,), 'x', 'bo', T=2).numel() == C * 2 * 6 * per


def _consumers():
    import torch
    from vdetlib_amd import ops
    from vdetlib_amd.vdet.tcn import TCNNet
    boxes, scores = torch.zeros(OFF[-1], 4, 4), torch.zeros(OFF[-1], 4, C)
    net = TCNNet.random([('det_scores', 1)], hidden=(4,))
    return {
        'anchor_propagate_tracks_batch': (lambda bo: ops.anchor_propagate_tracks_batch(bo, boxes, scores), ('tracks',)),
        'tcn_tracks_batch': (lambda bo: ops.tcn_tracks_batch(net, bo, series='pooled'), ('tracks', 'pooled')),
        'interpolate_tracks_batch': (lambda bo: ops.interpolate_tracks_batch(bo, None, [1, 2, 3]), ('tracks', 'det', 'pooled', 'tboxes')),
        'merge_tracks_batch': (lambda bo: ops.merge_tracks_batch(_host_batch(), bo), ('tracks', 'det', 'pooled', 'tboxes')),
        'nms_tracks_batch': (lambda bo: ops.nms_tracks_batch(bo), ('tracks', 'pooled', 'tboxes')),
        'rescore_tubelets_batch': (lambda bo: ops.rescore_tubelets_batch(bo, boxes, scores), ('tracks',)),
    }


@pytest.mark.parametrize("name", ['anchor_propagate_tracks_batch', 'tcn_tracks_batch', 'interpolate_tracks_batch', 'merge_tracks_batch',
                                  'nms_tracks_batch', 'rescore_tubelets_batch'])
def test_consumers_check_the_layout_before_the_device(name):
    call, fields = _consumers()[name]
    for k in fields:                                   # a cloned middle view in any field the consumer reads: a layout error
        bo = _host_batch()
        bo[k] = [bo[k][0], bo[k][1].clone(), bo[k][2]]
        assert 'consecutive' in _layout_error(lambda: call(bo)), (name, k)
    _layout_error(lambda: call(dict(_host_batch(), frame_off=np.asarray((0, 3, 3, 6)))))
    with pytest.raises(ValueError, match="same GPU"):  # the intact dict passes every layout check; host tensors end there
        call(_host_batch())


def test_rescore_floor_list_is_used_in_place_or_gathered():
    import torch
    from vdetlib_amd import ops
    bo = _host_batch()
    b = ops._batch_read(bo)
    flat = torch.arange(C * T * 6, dtype=torch.float32)
    floor = ops._batch_views(flat, b.off, C, T, 1)
    read = lambda lst, **kw: ops._batch_field(b, lst, 1, (torch.float32, torch.float64), 'floor', 'rescore_tubelets_batch', **kw)
    assert read(floor, gather=True).data_ptr() == flat.data_ptr()                       # consecutive views: in place
    stray = [floor[0], floor[1].clone() + 1000, floor[2]]
    got = read(stray, gather=True)                                                      # a stray middle view: gathered
    want = flat.clone()
    want[C * T * 1: C * T * 3] += 1000
    assert got.data_ptr() != flat.data_ptr() and torch.equal(got, want)
    apart = [x.clone() for x in floor]
    assert torch.equal(read(apart, gather=True), flat) and read(apart, gather=True).data_ptr() != flat.data_ptr()
    _layout_error(lambda: read(stray))                                                  # every other field refuses it
    for bad in (floor[:2], [floor[0], floor[1].double(), floor[2]], [floor[0], floor[1][:, :, :1], floor[2]], floor[::-1]):
        _layout_error(lambda: read(bad, gather=True))                                   # wrong shapes are never gathered
