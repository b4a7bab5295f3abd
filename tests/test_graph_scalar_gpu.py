"""-m gpu: graph_lists_kernel with one sign per pair (csrc/graphlists_kernels.hpp, pred_sign in csrc/nms_kernels.hpp).

The kernel decides a pair by the sign of ONE folded margin (tests/test_onesign_cpu.py states the rule) and never redoes a block
with the IEEE quotient.  What can go wrong is in the shapes and in the kinds of frame:
  * B = 385 and 450 end in a partial last column block, 1025 reaches a fifth row tile that holds one row (the direct lists
    start above 384 boxes per frame);
  * the last column block of the LAST frame of a volume lies partly behind the volume's last box: every volume here ends in
    such a frame, B = 385 leaves 63 of that block's 64 columns behind it (the case was set for a column table read through
    scalar loads, which was measured slower and is not in the library; the shapes stay);
  * three kinds of frame in one volume: integer boxes (kFlagU16: x2 + 1 / y2 + 1 formed once per box), fractional boxes
    (the + 1 stays in the pair arithmetic), and a grid of knife-edge pairs from tests/golden/knife_pairs.npz -- UP pairs,
    which only the quotient's rounding suppresses, and BAND pairs just below -- each pair in a cell of its own, scored so
    that one box of a pair stands directly above the other in class 0 and the other way round in class 1.
Every keep list must equal the oracle's, and the same call through the bit matrix (VDET_DIRECT_LISTS=0), whose
iou_bits_sym_kernel takes the same predicate."""
import functools
import os

import numpy as np
import pytest

import knife_spec as K
import synth

pytestmark = pytest.mark.gpu

PAIRS = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'knife_pairs.npz')
SIZES = (385, 450, 1025)
THRESHOLDS = (0.3, 0.5)
C = 2


@functools.lru_cache(maxsize=None)
def _video(B):
    """(boxes [3, B, 4], scores [3, B, 2]): an integer frame, a fractional frame, the knife-edge frame LAST."""
    bi, si = synth.video(1000 + B, 1, B, C)
    bf, sf = synth.video(2000 + B, 1, B, C, frac=True)
    assert np.array_equal(bi, np.trunc(bi)) and not np.array_equal(bf, np.trunc(bf))
    P = K.load_pairs(PAIRS)
    a = np.concatenate([P[('int', t)][0] for t in THRESHOLDS])
    b = np.concatenate([P[('int', t)][1] for t in THRESHOLDS])
    n = a.shape[0]
    assert 2 * n < 385
    for t in THRESHOLDS:        # the frame is no idle passenger: pairs in the rounding band at every threshold it is run at
        c = K.classify(a, b, t)
        assert c['BAND'].sum() >= 1 and (c['UP'].sum() >= 1 or t in K.POW2)
    fk = K.grid_frame(a, b, K.INT_CELL, K.INT_BOX, B - 2 * n, 3000 + B, 16)
    sk = K.pair_scores(n, B - 2 * n, 3000 + B)[:, :C]
    boxes = np.stack([bi[0], bf[0], fk]).astype(np.float32)
    scores = np.stack([si[0], sf[0], sk]).astype(np.float32)
    boxes.setflags(write=False); scores.setflags(write=False)
    return boxes, scores


@functools.lru_cache(maxsize=None)
def _want(B, t):
    from oracle import oracle as o
    o.build()
    boxes, scores = _video(B)
    return o.nms_volume(boxes, scores, t, cap=B)


def _run(monkeypatch, boxes, scores, t, direct):
    import torch
    from vdetlib_amd import ops, _lib
    monkeypatch.setenv("VDET_DIRECT_LISTS", direct)
    cx = _lib.Context(torch.cuda.current_device())
    try:
        idx, cnt = ops.nms_volume(torch.tensor(boxes).cuda(), torch.tensor(scores).cuda(), t, cap=boxes.shape[1], ctx=cx)
        return idx.cpu().numpy(), cnt.cpu().numpy(), cx.query(2), cx.query(15)
    finally:
        cx.close()


@pytest.mark.parametrize("t", THRESHOLDS)
@pytest.mark.parametrize("B", SIZES)
def test_direct_lists_against_oracle_and_bit_matrix(B, t, monkeypatch):
    boxes, scores = _video(B)
    widx, wcnt = _want(B, t)
    idx, cnt, reg, direct = _run(monkeypatch, boxes, scores, t, "1")
    idx0, cnt0, reg0, direct0 = _run(monkeypatch, boxes, scores, t, "0")
    assert reg == 1 and reg0 == 1                       # every frame regular
    assert direct == 1 and direct0 == 0                 # graph_lists_kernel built the first graph, the bit matrix the second
    assert np.array_equal(cnt, wcnt) and np.array_equal(idx, widx)
    assert np.array_equal(cnt0, wcnt) and np.array_equal(idx0, widx)
    assert np.array_equal(cnt, cnt0) and np.array_equal(idx, idx0)


# Far-apart and huge boxes.  frame_flags_kernel lets a regular frame hold coordinates up to 2^60 in magnitude, so that inter and
# uni are finite for every pair and pred_sign's margin is never inf - inf (a NaN with a clear sign bit would read as "suppress").
#   far    (0, 0, 10, 10) above (0, 1e17, 10, 1e17): regular, h hugely negative, the second box must survive
#   huge   a box from -2^60 to 2^60 above its duplicate and above everything else: regular, areas of 2^122; only the duplicate goes
#   beyond (0, 0, 10, 10) above (0, 3e38, 10, 3e38): w * h overflows, the frame is NOT regular and takes the general kernel
HUGE = {
    'far': ([[0, 0, 10, 10], [0, 1e17, 10, 1e17]], True),
    'huge': ([[-2.0 ** 60, -2.0 ** 60, 2.0 ** 60, 2.0 ** 60], [-2.0 ** 60, -2.0 ** 60, 2.0 ** 60, 2.0 ** 60]], True),
    'beyond': ([[0, 0, 10, 10], [0, 3e38, 10, 3e38]], False),
}


@pytest.mark.parametrize("t", THRESHOLDS)
@pytest.mark.parametrize("name", sorted(HUGE))
def test_far_apart_and_huge_boxes(name, t, monkeypatch):
    planted, regular = HUGE[name]
    B = 450
    boxes, scores = synth.video(4000 + len(name), 2, B, C)
    boxes, scores = boxes.astype(np.float32), scores.astype(np.float32)
    boxes[1, :2] = np.asarray(planted, np.float32)              # the LAST frame holds the planted pair
    scores[1, 0] = 2.0; scores[1, 1] = 1.5                      # ... first above second, both above every other box
    from oracle import oracle as o
    o.build()
    widx, wcnt = o.nms_volume(boxes, scores, t, cap=B)
    kept = [set(widx[1, c, :wcnt[1, c]].tolist()) for c in range(C)]
    assert all(0 in k and (1 in k) == (name != 'huge') for k in kept)       # (what the reference does with the pair)
    idx, cnt, reg, direct = _run(monkeypatch, boxes, scores, t, "1")
    idx0, cnt0, reg0, direct0 = _run(monkeypatch, boxes, scores, t, "0")
    assert reg == int(regular) and reg0 == int(regular) and direct == 1 and direct0 == 0
    assert np.array_equal(cnt, wcnt) and np.array_equal(idx, widx)
    assert np.array_equal(cnt0, wcnt) and np.array_equal(idx0, widx)
