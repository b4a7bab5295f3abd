"""The checked readers of ops.py's entry points (ops._volume, ops._anchor_slots, ops._images, ops._pixel_settings), on host
tensors: a tensor the device cannot read is refused with ValueError BEFORE the library is touched -- every entry point is called
with a context whose ``lib`` fails the test on any access -- and a wrong layout is refused as a layout, naming the argument.
Shapes: F = 2 frames, B = 4 boxes, C = 2 classes, T = 2 slots, images [2,8,8,3]."""
import numpy as np
import pytest

F, B, C, T = 2, 4, 2, 2


class NoLib(object):
    def __getattr__(self, name):
        raise AssertionError("the library was reached: lib.%s" % name)


class StandInCtx(object):
    """what ``ctx=`` takes, with nothing behind it: no call of the library can be made through it"""
    lib, h = NoLib(), None

    def set_stream(self, stream):
        pass

    def __getattr__(self, name):            # check, sync, invalidate: only a launch gets that far
        raise AssertionError("the context was used: ctx.%s" % name)


def host_inputs():
    import torch
    from vdetlib_amd import ops
    g = torch.Generator().manual_seed(5)
    xy = torch.rand((F, B, 2), generator=g) * 4
    off = np.array([0, 1, 2], dtype=np.int64)
    batch = {k: ops._batch_views(torch.zeros(C * T * F * per, dtype=dt), off, C, T, per)
             for k, per, dt in (('tracks', 5, torch.float32), ('det', 1, torch.float64))}
    batch.update(anchors=torch.zeros((2, C, T, 3)), ntracks=torch.zeros((2, C), dtype=torch.int32), frame_off=off)
    return dict(
        boxes=torch.cat([xy, xy + 3], dim=2), scores=torch.rand((F, B, C), generator=g),
        images=torch.zeros((F, 8, 8, 3), dtype=torch.uint8), off=off, batch=batch,
        order=torch.zeros((F, C, B), dtype=torch.int16), ncand=torch.zeros((F, C), dtype=torch.int32),
        kboxes=torch.zeros((F, B, C, 4)),
        aframes=torch.ones((C, T), dtype=torch.int32), aboxes=torch.ones((C, T, 4)), ascores=torch.zeros((C, T)),
        tracks=torch.zeros((C, T, F, 5)), ntracks=torch.zeros((C,), dtype=torch.int32), anchors=torch.zeros((C, T, 3)))


def entry_points(d, ctx):
    """name -> the call of every public entry point that reads a volume, anchors or images, on the tensors of ``d``"""
    from vdetlib_amd import ops
    vb = lambda x: x.unsqueeze(0).expand((2,) + tuple(x.shape))           # the anchors of two videos
    return {
        'nms_volume': lambda: ops.nms_volume(d['boxes'], d['scores'], ctx=ctx),
        'nms_volume FCB': lambda: ops.nms_volume(d['boxes'], d['scores'].transpose(1, 2), layout='FCB', ctx=ctx),
        'det_nms_volume': lambda: ops.det_nms_volume(d['kboxes'], d['scores'], ctx=ctx),
        'nms_volume_ordered': lambda: ops.nms_volume_ordered(d['boxes'], d['order'], d['ncand'], ctx=ctx),
        'track_volume': lambda: ops.track_volume(d['boxes'], d['scores'], ctx=ctx),
        'nms_track_volume': lambda: ops.nms_track_volume(d['boxes'], d['scores'], ctx=ctx),
        'video_batch': lambda: ops.video_batch(d['boxes'], d['scores'], d['off'], ctx=ctx),
        'top_anchors': lambda: ops.top_anchors(d['boxes'], d['scores'], T, ctx=ctx),
        'top_anchors batch': lambda: ops.top_anchors(d['boxes'], d['scores'], T, frame_off=d['off'], ctx=ctx),
        'track_from_anchors': lambda: ops.track_from_anchors(d['boxes'], d['aframes'], d['aboxes'], d['ascores'], ctx=ctx),
        'track_from_anchors_batch': lambda: ops.track_from_anchors_batch(d['boxes'], d['off'], vb(d['aframes']), vb(d['aboxes']),
                                                                         vb(d['ascores']), ctx=ctx),
        'track_pixels': lambda: ops.track_pixels(d['images'], d['aframes'], d['aboxes'], d['ascores'], ctx=ctx),
        'track_pixels_scaled': lambda: ops.track_pixels_scaled(d['images'], d['aframes'], d['aboxes'], ctx=ctx),
        'track_volume_pixels': lambda: ops.track_volume_pixels(d['images'], d['boxes'], d['scores'], ctx=ctx),
        'track_volume_pixels_scaled': lambda: ops.track_volume_pixels_scaled(d['images'], d['boxes'], d['scores'], ctx=ctx),
        'rescore_tracks': lambda: ops.rescore_tracks(d['tracks'], d['ntracks'], d['boxes'], d['scores'], ctx=ctx),
        'anchor_propagate_tracks': lambda: ops.anchor_propagate_tracks(d['tracks'], d['ntracks'], d['anchors'], d['boxes'],
                                                                       d['scores'], ctx=ctx),
        'anchor_propagate_tracks_batch': lambda: ops.anchor_propagate_tracks_batch(d['batch'], d['boxes'], d['scores'], ctx=ctx),
        'rescore_tubelets': lambda: ops.rescore_tubelets(d['tracks'], d['ntracks'], d['boxes'], d['scores'], ctx=ctx),
        'rescore_tubelets_batch': lambda: ops.rescore_tubelets_batch(d['batch'], d['boxes'], d['scores'], ctx=ctx),
    }


ENTRY_POINTS = ('anchor_propagate_tracks', 'anchor_propagate_tracks_batch', 'det_nms_volume', 'nms_track_volume', 'nms_volume',
                'nms_volume FCB', 'nms_volume_ordered', 'rescore_tracks', 'rescore_tubelets', 'rescore_tubelets_batch', 'top_anchors',
                'top_anchors batch', 'track_from_anchors', 'track_from_anchors_batch', 'track_pixels', 'track_pixels_scaled',
                'track_volume', 'track_volume_pixels', 'track_volume_pixels_scaled', 'video_batch')


def refused(call, *names):
    """``call`` raises ValueError; the text names one of ``names``"""
    with pytest.raises(ValueError) as e:
        call()
    assert not names or any(n in str(e.value) for n in names), str(e.value)
    return str(e.value)


@pytest.mark.parametrize("name", ENTRY_POINTS)
def test_host_tensors_are_refused_before_the_library(name):
    """well-shaped inputs in host memory: every layout check passes, the device check refuses them"""
    assert 'same GPU' in refused(entry_points(host_inputs(), StandInCtx())[name])


def test_volume_reader():
    from vdetlib_amd import ops
    d = host_inputs()
    boxes, scores = d['boxes'], d['scores']
    assert ops._volume_layout(boxes, scores) == (F, B, C) and ops._volume_layout(boxes) == (F, B, None)
    assert ops._volume_layout(boxes, scores.transpose(1, 2), layout='FCB') == (F, B, C)
    assert ops._volume_layout(boxes, scores, F=F, C=C, nonempty=True) == (F, B, C)
    lay = ops._volume_layout
    refused(lambda: lay(boxes.double(), scores), 'boxes')                             # dtype
    refused(lambda: lay(boxes, scores.double()), 'scores')
    refused(lambda: lay(boxes.numpy(), scores), 'boxes')
    refused(lambda: lay(boxes[0], scores), 'boxes')                                   # rank
    refused(lambda: lay(boxes.unsqueeze(0), scores), 'boxes')
    refused(lambda: lay(boxes, scores[0]), 'scores')
    refused(lambda: lay(boxes, scores.unsqueeze(0)), 'scores')
    refused(lambda: lay(boxes[:, :, :3], scores), 'boxes')                            # not four coordinates
    refused(lambda: lay(boxes[:1], scores), 'scores')                                 # F, B, C against each other
    refused(lambda: lay(boxes, scores[:, :3]), 'scores')
    refused(lambda: lay(boxes, scores, layout='FCB'), 'scores')
    refused(lambda: lay(boxes, scores.transpose(1, 2)), 'scores')
    refused(lambda: lay(boxes, scores, layout='BFC'), 'layout')
    refused(lambda: lay(boxes, scores, F=3), 'boxes')                                 # ... and against the caller's
    refused(lambda: lay(boxes, scores, C=3), 'scores')
    for zb, zs in ((boxes[:0], scores[:0]), (boxes[:, :0], scores[:, :0]), (boxes, scores[:, :, :0])):
        assert 0 in lay(zb, zs)                                                       # an empty volume is a layout ...
        refused(lambda: lay(zb, zs, nonempty=True), 'boxes')                          # ... that most kernels do not take
    refused(lambda: lay(boxes[:0], nonempty=True), 'boxes')
    # the reader in full: layout first, then the device
    refused(lambda: ops._volume(boxes, scores[:, :3]), 'scores')
    assert 'same GPU' in refused(lambda: ops._volume(boxes, scores), 'boxes and scores')
    assert 'same GPU' in refused(lambda: ops._volume(boxes, scores, (d['tracks'],), 'tracks, boxes and scores'), 'tracks')
    assert 'same GPU' in refused(lambda: ops._same_gpu((boxes, None), 'boxes'))


def test_anchor_slot_reader():
    from vdetlib_amd import ops
    d = host_inputs()
    fr, bx, sc = d['aframes'], d['aboxes'], d['ascores']
    got = ops._anchor_slots(fr, bx, sc)
    assert got[3:] == (C, T) and [x.data_ptr() for x in got[:3]] == [fr.data_ptr(), bx.data_ptr(), sc.data_ptr()]
    assert ops._anchor_slots(fr, bx)[2:] == (None, C, T)
    v = lambda x: x.unsqueeze(0).expand((3,) + tuple(x.shape))
    got = ops._anchor_slots(v(fr), v(bx), v(sc), V=3)
    assert got[3:] == (C, T) and all(x.is_contiguous() and x.shape[0] == 3 for x in got[:3])
    rd = ops._anchor_slots
    refused(lambda: rd(fr.long(), bx, sc), 'anchor_frames')                           # dtype
    refused(lambda: rd(fr, bx.double(), sc), 'anchor_boxes')
    refused(lambda: rd(fr, bx, sc.double()), 'anchor_scores')
    refused(lambda: rd(fr[0], bx, sc), 'anchor_frames')                               # rank
    refused(lambda: rd(v(fr), v(bx), v(sc)), 'anchor_frames')
    refused(lambda: rd(fr, bx, sc, V=3), 'anchor_frames')
    refused(lambda: rd(v(fr), v(bx), v(sc), V=2), 'anchor_frames')                    # the videos of frame_off
    refused(lambda: rd(fr, bx[:, :1], sc), 'anchor_boxes')                            # C, T against each other
    refused(lambda: rd(fr, bx[:, :, :3], sc), 'anchor_boxes')
    refused(lambda: rd(fr, bx, sc[:1]), 'anchor_scores')
    refused(lambda: rd(fr[:0], bx[:0], sc[:0]), 'anchor_frames')                      # no class
    assert rd(fr[:, :0], bx[:, :0], sc[:, :0])[3:] == (C, 0)                          # no slot: the kernels take T = 0


def test_image_and_settings_readers():
    import torch
    from vdetlib_amd import ops
    im = host_inputs()['images']
    assert ops._images(im) == (F, 8, 8)
    for bad in (im.float(), im[0], im[..., :2], im[:, :, ::2], im.numpy(), im[:0], im[:, :0], im[:, :, :0],
                torch.zeros((1, 1, 32768, 3), dtype=torch.uint8), torch.zeros((1, 32768, 1, 3), dtype=torch.uint8)):
        refused(lambda: ops._images(bad), 'images')
    assert ops._pixel_settings(32, 8, 0.5, 0, 1) == (32, 8, 0.5, 0, 1)
    assert ops._pixel_settings(4.0, 16, 1, 7, 3) == (4, 16, 1.0, 7, 3)
    for bad, name in (((0, 8, 0.5, 0, 1), 'grid'), ((30, 8, 0.5, 0, 1), 'grid'), ((68, 8, 0.5, 0, 1), 'grid'),
                      ((32, 0, 0.5, 0, 1), 'radius'), ((32, 17, 0.5, 0, 1), 'radius'), ((32, 8, float('nan'), 0, 1), 'min_conf'),
                      ((32, 8, float('inf'), 0, 1), 'min_conf'), ((32, 8, 0.5, -1, 1), 'max_frames'), ((32, 8, 0.5, 0, 0), 'step')):
        refused(lambda: ops._pixel_settings(*bad), name)


def test_entry_points_refuse_a_layout_as_a_layout():
    """on host tensors a wrong layout is reported as such: the device check comes last"""
    d = host_inputs()
    ctx = StandInCtx()
    assert sorted(entry_points(d, ctx)) == sorted(ENTRY_POINTS)
    wrong = dict(scores=d['scores'][:, :3], aboxes=d['aboxes'][:, :1], images=d['images'].float(), order=d['order'][:1],
                 ntracks=d['ntracks'].long(), kboxes=d['kboxes'][:, :, :1], off=np.array([0, 3]))
    seen = set()
    for key, bad in wrong.items():
        for name, call in entry_points(dict(d, **{key: bad}), ctx).items():
            text = refused(call)
            if 'same GPU' not in text:
                seen.add(name)
    assert seen == set(ENTRY_POINTS), sorted(set(ENTRY_POINTS) - seen)
    refused(lambda: entry_points(dict(d, scores=d['scores'][:, :, :0]), ctx)['track_volume_pixels'](), 'at least one')


def test_track_outputs_have_two_fill_policies():
    import torch
    from vdetlib_amd import ops
    tr, an, nt = ops._track_outputs(C, T, F, 'cpu', True)
    assert (tr.shape, an.shape, nt.shape) == ((C, T, F, 5), (C, T, 3), (C,))
    assert (tr.dtype, an.dtype, nt.dtype) == (torch.float32, torch.float32, torch.int32)
    assert bool(torch.isnan(tr).all()) and not an.any() and not nt.any()
    tr, an, nt = ops._track_outputs(C, T, F, 'cpu', True, V=3)
    assert (tr.shape, an.shape, nt.shape) == ((C * T * F * 5,), (3, C, T, 3), (3, C)) and bool(torch.isnan(tr).all())
    for V in (None, 3):
        e = ops._track_outputs(C, T, F, 'cpu', False, V=V)
        f = ops._track_outputs(C, T, F, 'cpu', True, V=V)
        assert [(x.shape, x.dtype) for x in e] == [(x.shape, x.dtype) for x in f]
