"""-m gpu: the forms of the fused volume pass that ``Context.set_vpass`` selects -- the lean form (csrc/temporal_kernels.hpp:
volume_pass_lean_kernel -- 2 items per thread, half the tile, blocks that stride over the (tile, frame chunk) list) and the
current kernel held to one block per compute unit (its dynamic LDS padded: what the multi-video pipeline's contexts launch)
-- against the current form (volume_pass_kernel) on the same inputs, each forced: pooled and conv equal bit for bit, the
lists sorted from the keys each form leaves in the context equal, and all of it equal to the references by the rule of
tests/test_temporal_seams_gpu.py --
the float32 references of tests/temporal_cases.py and ``oracle.temporal_*``, equal values everywhere, NaN where the
reference has NaN, no tolerance.  The volumes are ``temporal_cases.seam_volume``: NaN, +inf, -inf, -0.0 and tied scores on
every frame.  Chunk seams are forced into the short videos with the ``fchunk`` argument of ``set_vpass``."""
import numpy as np
import pytest
import torch

import synth
import temporal_cases as tc
from vdetlib_amd import ops, _lib

pytestmark = pytest.mark.gpu

CURRENT, LEAN, ONE_PER_CU = 1, 2, 3       # include/vdet_hip.h: VDET_VPASS_CURRENT, VDET_VPASS_LEAN, VDET_VPASS_ONE_PER_CU
RAN = {CURRENT: 4, LEAN: 2, ONE_PER_CU: 104}   # what vdet_query 12 answers after a pass of each form
FRAMES = (1, 2, 3, 17)                    # the window at both video borders; 17 with chunks of 5: seams at 5, 10, 15
BOXES = (1, 15, 16, 17, 33, 100)          # partial tiles of 16 / 64 boxes, B % 4 != 0 (scalar key stores), several tiles
CLASSES = (4, 12, 200)                    # tile rows of 1, 3, 50 float4
FCHUNK = {1: 1, 2: 1, 3: 2, 17: 5}        # frames per chunk forced per F: every F > 1 has a seam
PM, PC = tc.FUSED_PADS


@pytest.fixture(scope="module")
def ctxs():
    """(a context with the cache on and timing, a context that knows nothing of any pass)"""
    cx = _lib.Context(torch.cuda.current_device())
    cx.set_cache(True)
    cx.set_timing(1)
    plain = _lib.Context(torch.cuda.current_device())
    yield cx, plain
    cx.close()
    plain.close()


def _bits(t):
    return t.view(torch.int32)


def _same(t, want):
    return np.array_equal(t.cpu().numpy(), want, equal_nan=True)


def _lists(order, ncand):
    n = ncand.cpu().numpy()
    return tc.canonical_tail(order.cpu().numpy().astype(np.int64) & 0xFFFF, n), n


def _run(cx, form, fchunk, scores, window, taps, thr, off):
    """one pass in the given form -> (pooled, conv, order, ncand); the lists come from THIS pass's keys.  A pass of the
    current form over the negated volume runs first and the output buffers start as 7.0: whatever this pass fails to
    write -- outputs or keys -- is then wrong, not a leftover of the form run before it."""
    cx.set_vpass(CURRENT, 0)
    cx.invalidate()
    ops.volume_pass(-scores, window, None, score_thresh=thr, ctx=cx, frame_off=off)
    out = (torch.full_like(scores, 7.0), torch.full_like(scores, 7.0))
    cx.set_vpass(form, fchunk)
    cx.invalidate()
    pooled, conv = ops.volume_pass(scores, window, taps, pad_max=PM, bias=tc.BIAS, pad_conv=PC, score_thresh=thr, ctx=cx,
                                   frame_off=off, out=out)
    assert cx.query(12) == RAN[form], "the forced form did not run"
    order, ncand = ops.argsort_volume(scores, score_thresh=thr, ctx=cx)
    assert cx.last_timing()["transpose_keys"][1] == 0, "the key transpose ran although the pass left keys"
    cx.set_vpass(0, 0)
    return pooled, conv, order, ncand


def _compare(cx, oracle, shape, window, with_taps, thr, off, fchunk):
    """lean == current and one block per unit == current bit for bit (outputs and the lists sorted from each pass's keys),
    and each == the references"""
    vol = tc.seam_volume(*shape, tc.seed_of(*shape))
    scores = torch.tensor(vol, device="cuda")
    taps = tc.taps_for(window) if with_taps else None
    cur = _run(cx, CURRENT, fchunk, scores, window, taps, thr, off)
    assert (cur[1] is None) == (not with_taps)
    want_pool = tc.ref_maxpool(vol, window, PM, off)
    want_conv = tc.ref_conv(vol, taps, tc.BIAS, PC, off) if with_taps else None
    want_o, want_n = tc.cached_keys_order(shape, thr)
    for form, name in ((LEAN, "lean"), (ONE_PER_CU, "one block per unit")):
        got = _run(cx, form, fchunk, scores, window, taps, thr, off)
        assert torch.equal(_bits(got[0]), _bits(cur[0])), "pooled: %s != current" % name
        assert (got[1] is None) == (not with_taps)
        if with_taps:
            assert torch.equal(_bits(got[1]), _bits(cur[1])), "conv: %s != current" % name
        assert torch.equal(got[2], cur[2]) and torch.equal(got[3], cur[3]), "sorted lists: %s != current" % name
        # the references (the seam tests' rule)
        assert _same(got[0], want_pool), "pooled, " + name
        if with_taps:
            assert _same(got[1], want_conv), "conv, " + name
        if off is None:
            assert _same(got[0], oracle.temporal_maxpool(vol, window, PM)), "pooled against the oracle, " + name
            if with_taps:
                assert _same(got[1], oracle.temporal_conv(vol, taps, tc.BIAS, PC)), "conv against the oracle, " + name
        o, n = _lists(got[2], got[3])
        assert np.array_equal(n, want_n) and np.array_equal(o, want_o), "lists from the keys of the pass, " + name


@pytest.mark.parametrize("C", CLASSES)
@pytest.mark.parametrize("F", FRAMES)
def test_lean_equals_current_and_references(F, C, ctxs, oracle):
    """every B of BOXES at this (F, C): window 3 with taps, no score threshold, chunks forced to FCHUNK[F] frames"""
    for B in BOXES:
        _compare(ctxs[0], oracle, (F, B, C), 3, True, None, None, FCHUNK[F])


@pytest.mark.parametrize("with_taps", [True, False])
@pytest.mark.parametrize("thr", [None, 0.25])
def test_lean_options(with_taps, thr, ctxs, oracle):
    """window 3 with and without taps, the score threshold on and off (NaN, +-inf and -0.0 sit on every frame of a
    seam_volume: score_key and the threshold test see each of them), with the host's own chunk formula and a forced one"""
    for shape in ((17, 33, 12), (3, 17, 200)):
        for fchunk in (0, 2):
            _compare(ctxs[0], oracle, shape, 3, with_taps, thr, None, fchunk)


@pytest.mark.parametrize("C", CLASSES)
def test_lean_batched_videos(C, ctxs, oracle):
    """frame_off: three videos of 1, 2 and 5 frames (the seg path), chunks of 3 frames: a seam inside the last video"""
    off = np.asarray([0, 1, 3, 8], dtype=np.int64)
    for B in (17, 100):
        for thr in (None, 0.25):
            _compare(ctxs[0], oracle, (8, B, C), 3, True, thr, off, 3)


def test_lean_takes_the_current_form_where_it_does_not_fit(ctxs):
    """window 5 and C = 400 (a 16-box tile of 100 float4 rows does not fit 512 x 2 items): a forced lean form runs the
    current kernel, same outputs"""
    cx = ctxs[0]
    for shape, window in (((6, 40, 200), 5), ((6, 40, 400), 3)):
        scores = torch.tensor(tc.seam_volume(*shape, tc.seed_of(*shape)), device="cuda")
        out = []
        for form in (CURRENT, LEAN):
            cx.set_vpass(form, 2)
            cx.invalidate()
            out.append(ops.volume_pass(scores, window, tc.taps_for(window), ctx=cx))
            assert cx.query(12) == 4
            cx.set_vpass(0, 0)
        assert torch.equal(_bits(out[0][0]), _bits(out[1][0])) and torch.equal(_bits(out[0][1]), _bits(out[1][1]))
    with pytest.raises(ValueError):
        cx.set_vpass(9, 0)


def test_automatic_choice_per_context():
    """VDET_VPASS_AUTO: the multi-video pipeline's contexts (cache on + asynchronous) take the current kernel held to one
    block per compute unit at the 512-thread tiling (query 12 == 104), every other context and tiling the current form;
    the outputs do not depend on it"""
    for shape, want_async in (((5, 40, 200), 104), ((5, 40, 12), 4)):
        scores = torch.tensor(tc.seam_volume(*shape, tc.seed_of(*shape)), device="cuda")
        got = {}
        for cache, asyn in ((False, False), (True, False), (True, True)):
            cx = _lib.Context(torch.cuda.current_device())
            cx.set_cache(cache)
            cx.set_async(asyn)
            pooled, conv = ops.volume_pass(scores, 3, tc.taps_for(3), ctx=cx)
            cx.sync()
            got[(cache, asyn)] = (cx.query(12), pooled, conv)
            cx.close()
        assert got[(False, False)][0] == 4 and got[(True, False)][0] == 4 and got[(True, True)][0] == want_async
        for k in got:
            assert torch.equal(_bits(got[k][1]), _bits(got[(False, False)][1]))
            assert torch.equal(_bits(got[k][2]), _bits(got[(False, False)][2]))


def test_lean_midsize_tracking_and_rescoring_identical(ctxs):
    """F=20, B=1000, C=200: nms_track_volume and rescore_tracks after the lean pass and after the pass held to one block
    per compute unit == after the current pass.  Chunks of 2
    frames make 10 x 63 = 630 work items for the lean form's 512 blocks (2 per compute unit on an MI355X): blocks take a
    second item, so the stride and the hand-over of the key tile between items are part of the case."""
    F, B, C = 20, 1000, 200
    boxes, scores = synth.coherent_video(5201, F, B, C)
    tb, ts = torch.from_numpy(boxes).cuda(), torch.from_numpy(scores).cuda()
    cx = ctxs[0]
    out = []
    for form in (CURRENT, LEAN, ONE_PER_CU):
        cx.set_vpass(CURRENT, 0)
        cx.invalidate()
        ops.volume_pass(-ts, 3, None, ctx=cx)               # (stale keys and outputs of the other form are wrong ones)
        cx.set_vpass(form, 2)
        cx.invalidate()
        pooled, conv = ops.volume_pass(ts, 3, [0.25, 0.5, 0.25], ctx=cx, out=(torch.full_like(ts, 7.0), torch.full_like(ts, 7.0)))
        assert cx.query(12) == RAN[form]
        keep_idx, keep_cnt, tracks, anchors, ntracks = ops.nms_track_volume(tb, ts, nms_thres=0.3, thres=0.5, max_tracks=4, ctx=cx)
        det, tpool, tboxes = ops.rescore_tracks(tracks, ntracks, tb, ts, overlap_thres=0.7, window=3, ctx=cx)
        out.append((pooled, conv, keep_idx, keep_cnt, tracks, anchors, ntracks, det, tpool, tboxes))
        cx.set_vpass(0, 0)
    for other in out[1:]:
        assert torch.equal(_bits(out[0][0]), _bits(other[0])) and torch.equal(_bits(out[0][1]), _bits(other[1]))
        for a, b in zip(out[0][2:], other[2:]):
            assert a.shape == b.shape and a.dtype == b.dtype
            if a.dtype.is_floating_point:       # (a track has NaN rows where it has no box)
                assert torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(a.nan_to_num(-7.0), b.nan_to_num(-7.0))
            else:
                assert torch.equal(a, b)
    # and one frame at a time (20 x 63 items: every block's items alternate between the two key buffers)
    cx.set_vpass(CURRENT, 0)
    cx.invalidate()
    p0, c0 = ops.volume_pass(ts, 3, [0.25, 0.5, 0.25], ctx=cx)
    o0, n0 = ops.argsort_volume(ts, ctx=cx)
    cx.invalidate()
    ops.volume_pass(-ts, 3, None, ctx=cx)
    cx.set_vpass(LEAN, 1)
    cx.invalidate()
    p1, c1 = ops.volume_pass(ts, 3, [0.25, 0.5, 0.25], ctx=cx, out=(torch.full_like(ts, 7.0), torch.full_like(ts, 7.0)))
    o1, n1 = ops.argsort_volume(ts, ctx=cx)
    cx.set_vpass(0, 0)
    assert torch.equal(_bits(p1), _bits(p0)) and torch.equal(_bits(c1), _bits(c0))
    assert torch.equal(o1, o0) and torch.equal(n1, n0)
