"""-m gpu: the wide filter of the packed walk's sparse tail (walk_list_packed in csrc/nms_kernels.hpp).

Once a pass of 64 candidates queued fewer than the switch count, the walk tests four chunks per pass, compacts the wanted
candidates in list order, loads their records with one gather and queues them one pass later; a block that wants more than 64
is queued slice by slice.  Only WHEN a candidate's dead bit is looked at changes, so every keep list must be the oracle's and the
narrow-only walk's (VDET_WALK_WIDE=0, a context of its own).  What can go wrong sits in the shapes:
  * B = 385 is the smallest frame that takes walk_kernel (up to 384 boxes take the lane-per-list kernel); 2 600 gives several
    wide passes and a ragged last one;
  * list lengths of 64 k, 64 k + 1, 256 k - 1 and 256 k + 1, as B itself and as the count a score threshold leaves (ncand < B);
  * an integer frame (16-byte records) and a fractional frame (32-byte records) in every volume;
  * a frame whose density rises again after the switch (near-duplicates on top, then disjoint boxes: every wide block overflows);
  * the knife-edge pairs of tests/golden/knife_pairs.npz between duplicated fillers, so that the pairs reach their groups
    through the wide filter.
Dense frames are the bench's recipe (synth.boxes_1) with the corner positions drawn on a shrunken canvas; the test asserts with
the oracle that at most 15 % of a list survive.  vdet_query 18 / 19 = lists that went wide / wide passes that overflowed."""
import functools
import os

import numpy as np
import pytest

import knife_spec as K
import synth

pytestmark = pytest.mark.gpu

PAIRS = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'knife_pairs.npz')
THRESHOLDS = (0.3, 0.5)
C = 3
CANVAS = 0.02                           # of the recipe's 1280 x 720 (checked below: at most 15 % of a list survive)
DENSE_B = (385, 448, 449, 511, 513, 1023, 1025, 2600)
NCAND = (511, 513)                      # through a score threshold on frames of 640 boxes


def _dense_frame(rng, B, frac):
    x1 = rng.uniform(0, (synth.W - 50) * CANVAS, B)
    y1 = rng.uniform(0, (synth.H - 50) * CANVAS, B)
    w = rng.uniform(10, 300, B)
    h = rng.uniform(10, 300, B)
    b = np.stack([x1, y1, x1 + w, y1 + h], 1)
    return (b if frac else np.round(b)).astype(np.float32)


def _perm_scores(rng, F, B):
    ranks = np.argsort(np.argsort(rng.rand(F, B, C), axis=1), axis=1)
    return ((ranks + 0.5) / B).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _dense(B):
    """(boxes [2, B, 4], scores [2, B, 3]): a dense integer frame and a dense fractional frame."""
    rng = np.random.RandomState(5000 + B)
    boxes = np.stack([_dense_frame(rng, B, False), _dense_frame(rng, B, True)])
    assert np.array_equal(boxes[0], np.trunc(boxes[0])) and not np.array_equal(boxes[1], np.trunc(boxes[1]))
    scores = _perm_scores(rng, 2, B)
    boxes.setflags(write=False); scores.setflags(write=False)
    return boxes, scores


@functools.lru_cache(maxsize=None)
def _overflow():
    """Two frames (integer, fractional) of 200 near-duplicates of one box, ranked first in every class, above 632 pairwise disjoint
    small boxes: one survivor among the first 200, the passes behind it queue nothing (the switch), then every candidate is alive."""
    rng = np.random.RandomState(77)
    ndup, nsmall = 200, 632
    dup = np.array([2000, 2000, 2400, 2400], np.float32) + rng.randint(-3, 4, (ndup, 4)).astype(np.float32)
    g = np.arange(nsmall)
    x, y = (g % 26) * 20.0, (g // 26) * 20.0
    small = np.stack([x, y, x + 9, y + 9], 1).astype(np.float32)
    fi = np.concatenate([dup, small])
    boxes = np.stack([fi, fi + np.float32(0.25)]).astype(np.float32)
    B = ndup + nsmall
    scores = np.empty((2, B, C), np.float32)
    for f in range(2):
        for c in range(C):
            r = np.concatenate([nsmall + rng.permutation(ndup), rng.permutation(nsmall)])
            scores[f, :, c] = (r + 0.5) / B
    boxes.setflags(write=False); scores.setflags(write=False)
    return boxes, scores


@functools.lru_cache(maxsize=None)
def _knife(B=450):
    """A dense integer frame, and the knife-edge frame of tests/test_graph_scalar_gpu.py with its fillers replaced by copies of
    eight of them: the fillers die in their first group, the passes behind queue next to nothing, and in the third class (a random
    permutation) the pairs lie all over the list."""
    P = K.load_pairs(PAIRS)
    a = np.concatenate([P[('int', t)][0] for t in THRESHOLDS])
    b = np.concatenate([P[('int', t)][1] for t in THRESHOLDS])
    n = a.shape[0]
    assert 2 * n < 385
    for t in THRESHOLDS:
        c = K.classify(a, b, t)
        assert c['BAND'].sum() >= 1 and (c['UP'].sum() >= 1 or t in K.POW2)
    fk = K.grid_frame(a, b, K.INT_CELL, K.INT_BOX, B - 2 * n, 3000 + B, 16).copy()
    fk[2 * n:] = fk[2 * n + (np.arange(B - 2 * n) % 8)]
    sk = K.pair_scores(n, B - 2 * n, 3000 + B)[:, :C]
    db, ds = _dense(B)
    boxes = np.stack([db[0], fk]).astype(np.float32)
    scores = np.stack([ds[0], sk]).astype(np.float32)
    boxes.setflags(write=False); scores.setflags(write=False)
    return boxes, scores


@functools.lru_cache(maxsize=None)
def _want(name, B, t, score_thresh=None):
    from oracle import oracle as o
    o.build()
    boxes, scores = {'dense': _dense, 'knife': _knife}[name](B) if name != 'overflow' else _overflow()
    return o.nms_volume(boxes, scores, t, score_thresh=score_thresh, cap=boxes.shape[1])


def _run(monkeypatch, boxes, scores, t, wide, score_thresh=None):
    import torch
    from vdetlib_amd import ops, _lib
    monkeypatch.setenv("VDET_WALK_WIDE", wide)
    cx = _lib.Context(torch.cuda.current_device())
    try:
        idx, cnt = ops.nms_volume(torch.tensor(boxes).cuda(), torch.tensor(scores).cuda(), t, score_thresh=score_thresh,
                                  cap=boxes.shape[1], ctx=cx)
        return idx.cpu().numpy(), cnt.cpu().numpy(), cx.query(2), cx.query(18), cx.query(19)
    finally:
        cx.close()


def _check(monkeypatch, boxes, scores, t, want, score_thresh=None):
    widx, wcnt = want
    idx, cnt, reg, went, ovf = _run(monkeypatch, boxes, scores, t, "1", score_thresh)
    idx0, cnt0, reg0, went0, ovf0 = _run(monkeypatch, boxes, scores, t, "0", score_thresh)
    print("lists %d  went wide %d  overflow passes %d  (narrow-only context: %d / %d)" % (cnt.size, went, ovf, went0, ovf0))
    assert reg == 1 and reg0 == 1                       # every frame regular: the packed walk
    assert went0 == -1 and ovf0 == -1                   # the second context cannot go wide
    assert np.array_equal(cnt, wcnt) and np.array_equal(idx, widx)
    assert np.array_equal(cnt0, wcnt) and np.array_equal(idx0, widx)
    assert np.array_equal(cnt, cnt0) and np.array_equal(idx, idx0)
    return went, ovf


@pytest.mark.parametrize("t", THRESHOLDS)
@pytest.mark.parametrize("B", DENSE_B)
def test_dense_frames(B, t, monkeypatch):
    boxes, scores = _dense(B)
    want = _want('dense', B, t)
    assert want[1].max() <= 0.15 * B                    # dense: at most 15 % of any list survive
    went, ovf = _check(monkeypatch, boxes, scores, t, want)
    assert went > 0                                     # lists entered the wide filter


@pytest.mark.parametrize("t", THRESHOLDS)
@pytest.mark.parametrize("ncand", NCAND)
def test_threshold_leaves_a_partial_pass(ncand, t, monkeypatch):
    B = 640
    boxes, scores = _dense(B)
    st = (B - ncand) / B                                # scores are (rank + 0.5) / B: ranks B - ncand and up pass
    assert int((scores[0, :, 0] > np.float32(st)).sum()) == ncand
    want = _want('dense', B, t, st)
    went, ovf = _check(monkeypatch, boxes, scores, t, want, st)
    assert went > 0


@pytest.mark.parametrize("t", THRESHOLDS)
def test_overflow_blocks_are_queued_slice_by_slice(t, monkeypatch):
    boxes, scores = _overflow()
    want = _want('overflow', 0, t)
    assert np.all(want[1] == 1 + 632)                   # one of the near-duplicates and every small box
    went, ovf = _check(monkeypatch, boxes, scores, t, want)
    assert went == want[1].size and ovf > 0


@pytest.mark.parametrize("t", THRESHOLDS)
def test_knife_edge_pairs_through_the_wide_filter(t, monkeypatch):
    boxes, scores = _knife()
    want = _want('knife', 450, t)
    went, ovf = _check(monkeypatch, boxes, scores, t, want)
    assert went > C                                     # more lists than the dense frame has: the knife-edge frame's went wide
