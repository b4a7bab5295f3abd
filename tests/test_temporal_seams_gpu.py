"""-m gpu: the frame-chunk seams and the video borders of the temporal kernels (csrc/temporal_kernels.hpp:
temporal_vec4_kernel, temporal_both_vec4_kernel, volume_pass_kernel, and the scalar kernel they fall back to).  A block
owns a chunk of frames and re-reads a W/2 halo across the chunk border; the fused pass double-buffers its key tile by frame
parity; the batched form cuts every window at its own video's ends.  Every shape here is split into several chunks
(tests/temporal_cases.py: ``chunk_plan`` guards that, tests/test_temporal_seams_cpu.py checks it for an MI355X), the
volume has NaN, +-inf, -0.0 and tied scores on every frame, and every output -- pooled, conv, and the lists sorted from the
keys the pass leaves -- is compared with the float32 references of temporal_cases.py: equal values everywhere, NaN where the
reference has NaN, no tolerance."""
import numpy as np
import pytest
import torch

import temporal_cases as tc
from vdetlib_amd import ops, _lib

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cached_ctx():
    cx = _lib.Context(torch.cuda.current_device())
    cx.set_cache(True)
    cx.set_timing(1)
    yield cx
    cx.close()


@pytest.fixture(scope="module")
def plain_ctx():
    cx = _lib.Context(torch.cuda.current_device())
    yield cx
    cx.close()


def _seamed(kind, shape):
    """the plan of this shape on the device at hand; a shape that no longer has a seam there is skipped, loudly"""
    n_cu = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    plan = tc.chunk_plan(kind, shape[0], shape[1], shape[2], n_cu)
    if plan[0] < 2:
        pytest.skip(tc.REPICK % ("%s %s on %d compute units" % (kind, shape, n_cu)))
    return plan


def _vol(shape):
    return torch.tensor(tc.seam_volume(*shape, tc.seed_of(*shape)), device="cuda")


def _same(t, want):
    return np.array_equal(t.cpu().numpy(), want, equal_nan=True)


def _lists(order, ncand):
    n = ncand.cpu().numpy()
    return tc.canonical_tail(order.cpu().numpy().astype(np.int64) & 0xFFFF, n), n


def _check_keys(scores, shape, thr, cached_ctx, plain_ctx, transposes):
    """the lists sorted in the context the pass ran in (from its keys: ``transposes`` == 0; after a fallback the transpose
    runs: 1) and the lists of a context that knows nothing of the pass, both against the reference"""
    want_o, want_n = tc.cached_keys_order(shape, thr)
    o, n = _lists(*ops.argsort_volume(scores, score_thresh=thr, ctx=cached_ctx))
    assert cached_ctx.last_timing()["transpose_keys"][1] == transposes
    assert np.array_equal(n, want_n) and np.array_equal(o, want_o), "lists from the pass's keys"
    o2, n2 = _lists(*ops.argsort_volume(scores, score_thresh=thr, ctx=plain_ctx))
    assert np.array_equal(n2, want_n) and np.array_equal(o2, want_o), "lists from the key transpose"


# ------------------------------------------------------------------------------------------------
# standalone kernels
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", tc.POOL_WINDOWS)
@pytest.mark.parametrize("shape", tc.STANDALONE)
def test_maxpool_across_chunk_seams(shape, W):
    _seamed("standalone", shape)
    v = _vol(shape)
    for pm, _ in tc.PAD_PAIRS:
        assert _same(ops.temporal_maxpool(v, W, pad=pm), tc.cached_maxpool(shape, W, pm, None)), pm


@pytest.mark.parametrize("K", tc.CONV_WINDOWS)
@pytest.mark.parametrize("shape", tc.STANDALONE)
def test_conv_across_chunk_seams(shape, K):
    _seamed("standalone", shape)
    v = _vol(shape)
    for _, pc in tc.PAD_PAIRS:
        assert _same(ops.temporal_conv(v, tc.taps_for(K), bias=tc.BIAS, pad=pc), tc.cached_conv(shape, K, pc, None)), pc


def _both(v, shape, W, pm, pc):
    """the one-pass call == the two separate calls == the references"""
    pooled, conv = ops.temporal_maxpool_conv(v, W, tc.taps_for(W), pad_max=pm, bias=tc.BIAS, pad_conv=pc)
    assert _same(pooled, tc.cached_maxpool(shape, W, pm, None)), (pm, pc)
    assert _same(conv, tc.cached_conv(shape, W, pc, None)), (pm, pc)
    assert _same(ops.temporal_maxpool(v, W, pad=pm), pooled.cpu().numpy())
    assert _same(ops.temporal_conv(v, tc.taps_for(W), bias=tc.BIAS, pad=pc), conv.cpu().numpy())


@pytest.mark.parametrize("W", tc.BOTH_WINDOWS)
@pytest.mark.parametrize("shape", tc.STANDALONE)
def test_maxpool_conv_across_chunk_seams(shape, W):
    _seamed("standalone", shape)
    v = _vol(shape)
    for pm, pc in tc.PAD_PAIRS:
        _both(v, shape, W, pm, pc)


@pytest.mark.parametrize("shape", tc.WIDE)
def test_windows_of_the_scalar_kernel(shape):
    v = _vol(shape)
    pm, pc = tc.PAD_PAIRS[1]
    for W in tc.WIDE_POOL_WINDOWS:
        assert _same(ops.temporal_maxpool(v, W, pad=pm), tc.cached_maxpool(shape, W, pm, None)), W
    for K in tc.WIDE_CONV_WINDOWS:
        assert _same(ops.temporal_conv(v, tc.taps_for(K), bias=tc.BIAS, pad=pc), tc.cached_conv(shape, K, pc, None)), K
        _both(v, shape, K, pm, pc)


@pytest.mark.parametrize("W", tc.POOL_WINDOWS)
@pytest.mark.parametrize("shape", tc.ODD_S)
def test_series_count_of_the_scalar_kernel(shape, W):
    v = _vol(shape)
    for pm, pc in tc.PAD_PAIRS:
        _both(v, shape, W, pm, pc)


@pytest.mark.parametrize("W", tc.SHORT_WINDOWS)
@pytest.mark.parametrize("shape", tc.SHORT)
def test_window_wider_than_the_video(shape, W):
    v = _vol(shape)
    for pm, pc in tc.PAD_PAIRS:
        _both(v, shape, W, pm, pc)


# ------------------------------------------------------------------------------------------------
# the fused pass
# ------------------------------------------------------------------------------------------------
def _pass(scores, shape, window, with_taps, thr, border, cx, out=None):
    """one volume_pass against the references; the context's caches are dropped first, so that what is sorted afterwards
    can only come from THIS pass's keys"""
    pm, pc = tc.FUSED_PADS
    cx.invalidate()
    off = None if border is None else tc.border_table(border, shape[0])
    pooled, conv = ops.volume_pass(scores, window, tc.taps_for(window) if with_taps else None, pad_max=pm, bias=tc.BIAS,
                                   pad_conv=pc, score_thresh=thr, ctx=cx, frame_off=off, out=out)
    assert _same(pooled, tc.cached_maxpool(shape, window, pm, border)), "pooled"
    if with_taps:
        assert _same(conv, tc.cached_conv(shape, window, pc, border)), "conv"
    else:
        assert conv is None
    return pooled, conv


@pytest.mark.parametrize("window", tc.FUSED_WINDOWS)
@pytest.mark.parametrize("shape", tc.FUSED)
def test_fused_pass_across_chunk_seams(shape, window, cached_ctx, plain_ctx):
    chunks, fchunk, tiling = _seamed("fused", shape)
    assert tiling == tc.FUSED_TILINGS[shape[2]], tc.REPICK % str(shape)
    scores = _vol(shape)
    for with_taps in (True, False):
        for thr in tc.FUSED_THR:
            _pass(scores, shape, window, with_taps, thr, None, cached_ctx)
            _check_keys(scores, shape, thr, cached_ctx, plain_ctx, 0)


@pytest.mark.parametrize("border", tc.BORDER_SETS)
@pytest.mark.parametrize("shape", tc.FUSED)
def test_batched_fused_pass_across_seams_and_borders(shape, border, cached_ctx, plain_ctx):
    _seamed("fused", shape)
    scores = _vol(shape)
    for window in tc.FUSED_WINDOWS:
        for with_taps in (True, False):
            for thr in tc.FUSED_THR:
                _pass(scores, shape, window, with_taps, thr, border, cached_ctx)
                _check_keys(scores, shape, thr, cached_ctx, plain_ctx, 0)
        if border == "one":         # one video of F frames == the unbatched call, bit for bit
            pooled, conv = _pass(scores, shape, window, True, None, border, plain_ctx)
            p1, c1 = _pass(scores, shape, window, True, None, None, plain_ctx)
            assert torch.equal(p1.view(torch.int32), pooled.view(torch.int32))
            assert torch.equal(c1.view(torch.int32), conv.view(torch.int32))


@pytest.mark.parametrize("border", tc.BORDER_SETS)
@pytest.mark.parametrize("case", tc.BATCH_FALLBACK, ids=lambda c: "%dx%dx%d-W%d-%s" % (c[0], c[1], c[2], c[3], c[5]))
def test_batched_fallbacks_across_seams_and_borders(case, border, cached_ctx, plain_ctx):
    F, B, C, window, with_taps, kernel = case
    shape = (F, B, C)
    if kernel != "scalar":
        _seamed("standalone", shape)
    scores = _vol(shape)
    pooled, conv = _pass(scores, shape, window, with_taps, None, border, cached_ctx)
    _check_keys(scores, shape, None, cached_ctx, plain_ctx, 1)         # a fallback leaves no keys
    if border == "one":
        p1, c1 = _pass(scores, shape, window, with_taps, None, None, plain_ctx)
        assert torch.equal(p1.view(torch.int32), pooled.view(torch.int32))
        assert conv is None or torch.equal(c1.view(torch.int32), conv.view(torch.int32))


# ------------------------------------------------------------------------------------------------
# a contiguous volume that does not start on a 16-byte boundary
# ------------------------------------------------------------------------------------------------
def _off_by_4_bytes(n):
    """a contiguous float32 buffer of n elements whose pointer sits 4 bytes behind a 16-byte boundary"""
    big = torch.empty(n + 4, dtype=torch.float32, device="cuda")
    view = big[1:1 + n]
    assert big.data_ptr() % 16 == 0 and view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


@pytest.mark.parametrize("shape", tc.ALIGN)
def test_alignment_fallback(shape, cached_ctx, plain_ctx):
    """the vec4 and the fused kernels need 16-byte aligned pointers; the host takes the scalar kernels for anything else,
    inputs or ``out=`` buffers alike, and leaves no keys behind"""
    W = tc.ALIGN_WINDOW
    pm, pc = tc.FUSED_PADS
    n = shape[0] * shape[1] * shape[2]
    aligned = _vol(shape)
    scores = _off_by_4_bytes(n).view(shape)
    scores.copy_(aligned)
    assert scores.is_contiguous() and scores.data_ptr() % 16 == 4
    assert _same(ops.temporal_maxpool(scores, W, pad=pm), tc.cached_maxpool(shape, W, pm, None))
    _both(scores, shape, W, pm, pc)
    # volume_pass: a control on aligned memory (fused kernel, keys left), then every way of being off
    _pass(aligned, shape, W, True, None, None, cached_ctx, out=(torch.empty(n, device="cuda"), torch.empty(n, device="cuda")))
    _check_keys(aligned, shape, None, cached_ctx, plain_ctx, 0)
    for src, out in ((scores, None),
                     (scores, (_off_by_4_bytes(n), _off_by_4_bytes(n))),
                     (aligned, (_off_by_4_bytes(n), _off_by_4_bytes(n))),
                     (aligned, (torch.empty(n, device="cuda"), _off_by_4_bytes(n)))):
        for with_taps in (True, False):
            if out is not None and not with_taps and out[0].data_ptr() % 16 == 0 and src is aligned:
                continue            # (without taps the conv buffer is not used: that call is aligned)
            pooled, conv = _pass(src, shape, W, with_taps, None, None, cached_ctx, out=out)
            if out is not None:
                assert pooled.data_ptr() == out[0].data_ptr() and (conv is None or conv.data_ptr() == out[1].data_ptr())
            _check_keys(src, shape, None, cached_ctx, plain_ctx, 1)
