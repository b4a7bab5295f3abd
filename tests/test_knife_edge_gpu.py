"""-m gpu: every divide-free threshold predicate on box pairs that sit on the knife edge of the IoU test.

The reference suppresses iff RN(inter / uni) >= t32; the hot paths take the sign of one fma and fall back to the quotient in a
narrow band (pred_margins / pred_regular in csrc/nms_kernels.hpp, margin_block in csrc/graphlists_kernels.hpp, the packed
walk's in-group test, the tracker's link scans, and the x-reach culling that decides which pairs are evaluated at all).
tests/golden/knife_pairs.npz (tests/knife_spec.py, tests/test_knife_edge_cpu.py) holds pairs of every class per threshold:
UP (only the quotient says "suppress"), BAND (the fallback must say "keep"), one ulp above, exact zero margin, and the
closed-form families that sit exactly on the reach bound.  Frames are built with every pair in a cell of its own and run
through every site at the smallest shapes that select it; the oracle is the referee everywhere.
"""
import functools
import os

import numpy as np
import pytest

import knife_spec as K

pytestmark = pytest.mark.gpu

F32 = np.float32
PAIRS = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'knife_pairs.npz')
SMALL, LARGE = 300, 600          # iou_bits_sym_kernel + the small-list walk / graph_lists_kernel (> 384) + the packed walk
KNOBS = ["VDET_DIRECT_LISTS=0", "VDET_WAVE_TRANSPOSE=0", "VDET_ADJ_ROWS=0", "VDET_NO_INDEX=1", "VDET_SMALL_LISTS=0",
         "VDET_FORCE_GENERAL=1"]
ODD = (0.0, -0.1, 1e-31, 1e-20, 1.0, 1.5)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


@functools.lru_cache(maxsize=None)
def _pairs():
    return K.load_pairs(PAIRS)


def _own_then_others(form, ts, part, nparts, n):
    """n pairs: the pairs of the thresholds ts (part `part` of `nparts` of them) first, then pairs of the other thresholds."""
    P = _pairs()
    own_a = np.concatenate([P[(form, t)][0] for t in ts] + [np.zeros((0, 4), F32)])
    own_b = np.concatenate([P[(form, t)][1] for t in ts] + [np.zeros((0, 4), F32)])
    if len(ts) > 1:          # (several thresholds share the frame: a fixed shuffle, so that a cut takes from all of them)
        p = np.random.RandomState(17).permutation(own_a.shape[0])
        own_a, own_b = own_a[p], own_b[p]
    own_a, own_b = own_a[part::nparts], own_b[part::nparts]
    rest = [t for t in K.THRESHOLDS if t not in ts]
    a = np.concatenate([own_a] + [P[(form, t)][0][part::nparts] for t in rest])[:n]
    b = np.concatenate([own_b] + [P[(form, t)][1][part::nparts] for t in rest])[:n]
    return a, b


@functools.lru_cache(maxsize=None)
def _volume(ts, B):
    """boxes [7, B, 4], scores [7, B, 3]: an all-integer frame, two fractional frames, an integer frame with a single
    coordinate of 65536 (the float form on integer values), the fixture's reach-tight families among narrow fillers, and
    two frames built rank by rank so that the reach table decides their pairs (K.reach_frame, of ts[0]).  ts: the
    thresholds whose knife-edge pairs come first (highest scores); pair cells of other thresholds fill up."""
    seed = 100 * B + int(1000 * sum(ts))
    npi = 130 if B < 384 else 256
    boxes, scores = [], []

    def add(fr, npairs, s):
        assert fr.shape == (B, 4)
        boxes.append(fr); scores.append(K.pair_scores(npairs, B - 2 * npairs, s))
    for k in (0, 3):
        a, b = _own_then_others('int', ts, 0, 1, npi)
        fr = K.grid_frame(a, b, K.INT_CELL, K.INT_BOX, B - 2 * a.shape[0], seed + k, 16)
        if k == 3:
            fr[B - 1] = [65500, 4000, 65536, 4010]       # (a filler in the last cell's strip)
        add(fr, a.shape[0], seed + k)
        if k == 0:
            for part in (0, 1):
                a, b = _own_then_others('frac', ts, part, 2, 64)
                add(K.grid_frame(a, b, K.FRAC_CELL, K.FRAC_BOX, B - 2 * a.shape[0], seed + 1 + part, 8), a.shape[0], seed + 1 + part)
    P = _pairs()
    a = np.concatenate([P[('reach', t)][0] for t in ts])
    b = np.concatenate([P[('reach', t)][1] for t in ts])
    add(K.band_frame(a, b, B - 2 * a.shape[0], seed + 4), a.shape[0], seed + 4)
    for s in K.REACH_SEEDS:          # the frames on which the reach table decides (one set per threshold of ts)
        for t in ts[:1]:
            fr, pr = K.reach_frame(t, B, s)
            add(fr, pr.shape[0], seed + 5 + s)
    boxes, scores = np.stack(boxes), np.stack(scores)
    u16 = [bool(np.all((f >= 0) & (f <= 65535) & (f == np.rint(f)))) for f in boxes]
    assert u16 == [True, False, False, False, True, True, True] and boxes[3].max() == 65536 and np.array_equal(boxes[3], np.rint(boxes[3]))
    boxes.setflags(write=False); scores.setflags(write=False)
    return boxes, scores


_WANT = {}


def _want(oracle, key, boxes, scores, t):
    """oracle.nms_volume, computed once per (volume, threshold) and shared by the tests."""
    k = key + (float(t),)
    if k not in _WANT:
        _WANT[k] = oracle.nms_volume(boxes, scores, t)
    return _WANT[k]


def _check(torch, oracle, key, t, ctx=None, thresh=None, dev=None):
    from vdetlib_amd import ops
    boxes, scores = _volume(*key)
    thresh = t if thresh is None else thresh
    tb, ts = dev if dev is not None else (torch.from_numpy(boxes.copy()).cuda(), torch.from_numpy(scores.copy()).cuda())
    idx, cnt = ops.nms_volume(tb, ts, thresh, ctx=ctx)
    widx, wcnt = _want(oracle, key, boxes, scores, thresh)
    assert np.array_equal(cnt.cpu().numpy(), wcnt), (key, thresh)
    assert np.array_equal(idx.cpu().numpy(), widx), (key, thresh)


@pytest.mark.parametrize("t", K.THRESHOLDS)
@pytest.mark.parametrize("B", [SMALL, LARGE])
def test_volume_on_the_knife_edge(torch_cuda, oracle, t, B):
    """Small frames (iou_bits_sym_kernel + the small-list walk) and large ones (graph_lists_kernel's margin_block, the packed
    walk's in-group test, off-diagonal tiles): keep lists and counts equal to the oracle's."""
    boxes, scores = _volume((t,), B)
    # the frames do hold what they are built for: pairs the quotient alone suppresses / the fallback must keep
    c = K.classify(boxes[0, 0:2 * 130:2], boxes[0, 1:2 * 130:2], t)
    assert int(c['BAND'].sum()) >= 16 and int(c['ABOVE1'].sum()) >= 16 and (t in K.POW2 or int(c['UP'].sum()) >= 16)
    _check(torch_cuda, oracle, ((t,), B), t)


@pytest.mark.parametrize("knob", KNOBS)
def test_large_frames_on_every_alternative_path(torch_cuda, oracle, monkeypatch, knob):
    """The large-frame volumes again in a context created under each diagnostic switch (read at vdet_create)."""
    from vdetlib_amd import _lib
    name, _, val = knob.partition('=')
    monkeypatch.setenv(name, val or '1')
    cx = _lib.Context(torch_cuda.cuda.current_device())
    try:
        for t in K.THRESHOLDS:
            _check(torch_cuda, oracle, ((t,), LARGE), t, ctx=cx)
    finally:
        cx.close()


@pytest.mark.parametrize("B", [SMALL, LARGE])
def test_cached_graph_follows_the_threshold(torch_cuda, oracle, B):
    """vdet_set_cache(1): the same volume twice at one threshold, then twice at another, and back -- the cached graph and
    the threshold the walk tests with must both follow."""
    from vdetlib_amd import _lib
    cx = _lib.Context(torch_cuda.cuda.current_device())
    cx.set_cache(True)
    try:
        for ts in ((0.3, 0.7), (0.45, 0.9), (0.5, 0.1)):
            boxes, scores = _volume(ts, B)
            # the contract of the cache: the same device buffers, unchanged between the calls
            dev = (torch_cuda.from_numpy(boxes.copy()).cuda(), torch_cuda.from_numpy(scores.copy()).cuda())
            for t in (ts[0], ts[0], ts[1], ts[1], ts[0]):
                _check(torch_cuda, oracle, (ts, B), None, ctx=cx, thresh=t, dev=dev)
            cx.invalidate()          # (the next volume may land in the buffers this one frees)
    finally:
        cx.close()


@functools.lru_cache(maxsize=None)
def _odd_volume(B):
    """An integer grid frame whose fillers repeat pair boxes (duplicates), the identical pairs of threshold 1 among the
    reach-tight pairs of 1e-3, and the fractional near-duplicates whose quotient is exactly 1."""
    P = _pairs()
    npi = 120 if B < 384 else 250
    a, b = _own_then_others('int', (0.3, 0.7), 0, 1, npi)
    f0 = K.grid_frame(a, b, K.INT_CELL, K.INT_BOX, B - 2 * npi, 5 * B, 16)
    f0[2 * npi:] = f0[np.random.RandomState(B).randint(0, 2 * npi, B - 2 * npi)]
    frames, scores = [f0], [K.pair_scores(npi, B - 2 * npi, 5 * B)]
    for k, keys in enumerate(((('reach', 1.0), ('unit', 'same'), ('reach', 1e-3)), (('unit', 'near'), ('unit', 'same')))):
        a = np.concatenate([P[q][0] for q in keys]); b = np.concatenate([P[q][1] for q in keys])
        frames.append(K.band_frame(a, b, B - 2 * a.shape[0], 5 * B + 1 + k))
        scores.append(K.pair_scores(a.shape[0], B - 2 * a.shape[0], 5 * B + 1 + k))
    boxes, scores = np.stack(frames), np.stack(scores)
    boxes.setflags(write=False); scores.setflags(write=False)
    return boxes, scores


@pytest.mark.parametrize("t", ODD)
@pytest.mark.parametrize("B", [SMALL, LARGE])
def test_odd_thresholds(torch_cuda, oracle, t, B):
    """0, a negative one, 1e-31 (below the 1e-30 routing cut), 1e-20, 1 and 1.5 on frames that also hold duplicates."""
    from vdetlib_amd import ops
    boxes, scores = _odd_volume(B)
    inter, uni, q = K.quotient(boxes[2, 0:24:2], boxes[2, 1:24:2])
    assert np.all(q == 1) and not np.array_equal(boxes[2, 0:24:2], boxes[2, 1:24:2])
    idx, cnt = ops.nms_volume(torch_cuda.from_numpy(boxes.copy()).cuda(), torch_cuda.from_numpy(scores.copy()).cuda(), t)
    widx, wcnt = oracle.nms_volume(boxes, scores, t)
    assert np.array_equal(cnt.cpu().numpy(), wcnt) and np.array_equal(idx.cpu().numpy(), widx)


@functools.lru_cache(maxsize=None)
def _reach_volume(t, B):
    """The fixture's reach-tight family of threshold t among narrow fillers, and the two frames on which the reach table
    decides, for thresholds that have no searched pairs."""
    a, b = _pairs()[('reach', t)]
    frames, scores = [K.band_frame(a, b, B - 2 * a.shape[0], 7 * B)], [K.pair_scores(a.shape[0], B - 2 * a.shape[0], 7 * B)]
    for s in K.REACH_SEEDS:
        fr, pr = K.reach_frame(t, B, s)
        frames.append(fr); scores.append(K.pair_scores(pr.shape[0], B - 2 * pr.shape[0], 7 * B + s))
    boxes, scores = np.stack(frames), np.stack(scores)
    boxes.setflags(write=False); scores.setflags(write=False)
    return boxes, scores


@pytest.mark.parametrize("knob", [None, "VDET_DIRECT_LISTS=0", "VDET_ADJ_ROWS=0"])
@pytest.mark.parametrize("B", [SMALL, LARGE])
def test_reach_frames_at_one_thousandth(torch_cuda, oracle, monkeypatch, B, knob):
    """Threshold 1e-3, where (1 - t) * W is nearly the whole width: the closed-form family and the rank-built frames, small and
    large, on the default path, through the bit matrix (the block and tile-pair tests of iou_bits_sym_kernel) and through
    adj_build_kernel."""
    from vdetlib_amd import ops, _lib
    if knob:
        name, _, val = knob.partition('=')
        monkeypatch.setenv(name, val)
    cx = _lib.Context(torch_cuda.cuda.current_device())
    try:
        boxes, scores = _reach_volume(1e-3, B)
        assert K.classify(boxes[0, 0:48:2], boxes[0, 1:48:2], 1e-3)['sup'].all()
        idx, cnt = ops.nms_volume(torch_cuda.from_numpy(boxes.copy()).cuda(), torch_cuda.from_numpy(scores.copy()).cuda(), 1e-3, ctx=cx)
        widx, wcnt = oracle.nms_volume(boxes, scores, 1e-3)
        assert np.array_equal(cnt.cpu().numpy(), wcnt) and np.array_equal(idx.cpu().numpy(), widx)
    finally:
        cx.close()


# ---- the paths that divide: they are expected to pass, and guard against a build flag that loosens the division ---------
from test_nms_gpu import cnms  # noqa: E402,F401  (utils.cython_nms as one fused launch, and under VDET_NO_FUSED=1)


def test_small_frames_through_cython_nms(oracle, cnms):
    for t in K.THRESHOLDS:
        boxes, scores = _volume((t,), SMALL)
        for f in range(boxes.shape[0]):
            for c in range(scores.shape[2]):
                d = np.hstack([boxes[f], scores[f, :, c:c + 1]]).astype(F32)
                assert cnms.nms(d, t) == oracle.nms(d, t), (t, f, c)


def test_small_frames_through_det_nms_volume(torch_cuda, oracle):
    """Every class suppresses its own copy of the boxes.  The kernel takes at most 128 rows per (frame, class), i.e. the
    first 64 pairs of score columns 0 and 1; the integer frames hold up to 86 pairs of their own threshold, so a second
    pass gives the scores of those pairs to them in reverse order and brings the last ones to the top."""
    from vdetlib_amd import ops
    from test_detnms_gpu import _check_frame
    for t in K.THRESHOLDS:
        boxes, scores = _volume((t,), SMALL)
        F, B, C = scores.shape
        own = _pairs()[('int', t)][0].shape[0]
        assert own <= 128 and _pairs()[('frac', t)][0].shape[0] <= 128            # (frac: two frames, half each)
        BX = np.ascontiguousarray(np.repeat(boxes[:, :, None, :], C + 1, axis=2))
        S = np.concatenate([np.zeros((F, B, 1), F32), scores], 2)
        S2 = S.copy()
        rev = np.arange(2 * own).reshape(own, 2)[::-1].ravel()
        for f in (0, 3):
            S2[f, :2 * own] = S[f, rev]
        for Sx in (S, S2):
            out = [x.cpu().numpy() for x in ops.det_nms_volume(torch_cuda.from_numpy(BX).cuda(), torch_cuda.from_numpy(Sx).cuda(),
                                                               score_thresh=None, topk=128, nms_thresh=t)]
            for f in range(F):
                _check_frame(oracle, f, Sx, BX, out, -np.inf, 128, t)


def test_small_frames_through_nms_tracks(torch_cuda, oracle):
    """The still-image source alone (T = 0): every box of a frame as a candidate list in descending score order."""
    from vdetlib_amd import ops
    from test_nms_tracks_cpu import expected, outputs_equal
    torch = torch_cuda
    for t in K.THRESHOLDS:
        boxes, scores = _volume((t,), SMALL)
        F, B, C = scores.shape
        ki = np.empty((F, C, B), np.int32)
        for f in range(F):
            for c in range(C):
                ki[f, c] = oracle.argsort_desc(scores[f, :, c])
        kc = np.full((F, C), B, np.int32)
        tracks, ntracks, score = np.zeros((C, 0, F, 5), F32), np.zeros(C, np.int32), np.zeros((C, 0, F))
        still = (boxes, scores, ki, kc)
        want = expected(tracks, ntracks, score, None, still, thresh=t, top_still=B)
        out = ops.nms_tracks(torch.from_numpy(tracks).cuda(), torch.from_numpy(ntracks).cuda(), torch.from_numpy(score).cuda(),
                             still=tuple(torch.from_numpy(np.array(x)).cuda() for x in still), thresh=t, top_still=B)
        got = {k: out[k].cpu().numpy() for k in ('tracks', 'score', 'src', 'cnt', 'ntracks')}
        assert outputs_equal(got, want), t


# ---- linking ------------------------------------------------------------------------------------------------------------
LINK_CLASSES = ('UP', 'BAND', 'BELOW1', 'ABOVE1', 'ZERO')


@functools.lru_cache(maxsize=None)
def _link_video(t, B, seed, wide):
    """Three frames.  The middle one holds isolated anchors, the outer boxes of the integer pairs of threshold t, each in
    a cell of its own; frames 0 and 2 hold, per anchor, the pair's other box (IoU on the knife edge), a decoy of a third of
    that IoU, and for every second pair a twin of the other box -- the same size at the mirrored place inside the anchor, so
    its float32 IoU is exactly equal and the lower index must win.  Score column c makes anchors of the pairs of class
    LINK_CLASSES[c] (the only scores above the stop threshold 0.5).  wide: one coordinate of 65536 in frames 0 and 2 (the
    float4 index instead of the compact u16 one).  Returns boxes [3, B, 4], scores [3, B, 5], the classes' masks."""
    a, b = _pairs()[('int', t)]
    n = a.shape[0]
    rng = np.random.RandomState(seed)
    off = K.cell_offsets(rng, n, K.INT_CELL, 16)
    A, Bx = a + off, b + off
    W = a[:, 2] - a[:, 0] + 1
    decoy = A.copy()
    decoy[:, 2] = A[:, 0] + np.maximum(1, np.floor(W * t / 3)) - 1                 # full height, a third of t wide
    twin = Bx.copy()
    twin[:, 0], twin[:, 2] = A[:, 0] + (A[:, 2] - Bx[:, 2]), A[:, 2] - (Bx[:, 0] - A[:, 0])
    twin[:, 1], twin[:, 3] = A[:, 1] + (A[:, 3] - Bx[:, 3]), A[:, 3] - (Bx[:, 1] - A[:, 1])
    has_twin = (np.arange(n) % 2 == 0) & np.any(twin != Bx, 1)
    for x, y in zip(K.quotient(A, Bx), K.quotient(A[has_twin], twin[has_twin])):
        assert np.array_equal(x[has_twin], y)
    c = K.classify(A, Bx, t)
    assert np.array_equal(c['q'], K.classify(a, b, t)['q'])
    boxes = np.zeros((3, B, 4), F32)
    scores = np.zeros((3, B, len(LINK_CLASSES)), F32)
    for f in range(3):
        rows = [A] if f == 1 else [Bx, decoy, twin[has_twin]]
        rows = np.concatenate(rows)
        fill = K.strip_fillers(rng, B - rows.shape[0], K.INT_CELL, K.INT_BOX, 16)
        if wide and f != 1:
            fill[0] = [65500, 4000, 65536, 4010]
        perm = rng.permutation(B)
        boxes[f, perm] = np.concatenate([rows, fill])
        scores[f] = (rng.permutation(B * 5).reshape(B, 5) + 1).astype(F32) / F32(B * 5 * 4)       # all below 0.25
        if f == 1:
            for k, name in enumerate(LINK_CLASSES):
                m = c[name] & ~c['BELOW1'] if name == 'BAND' else c[name]
                ids = np.flatnonzero(m)
                assert ids.size <= 64
                scores[1, perm[ids], k] = F32(0.95) - np.arange(ids.size, dtype=F32) / F32(256)
    boxes.setflags(write=False); scores.setflags(write=False)
    return boxes, scores, {k: int(c[k].sum()) for k in LINK_CLASSES}


def _check_tracks(oracle, boxes, scores, link_thres, tr, an, nt, counts):
    assert counts['BAND'] >= 16 and counts['ABOVE1'] >= 16 and (link_thres == 0.5 or counts['UP'] >= 16)
    for k, name in enumerate(LINK_CLASSES):
        wt, wa, wn = oracle.greedy_track_volume(boxes, scores[:, :, k], 0.3, 0.5, 64, link_thres, 0)
        assert wn == (counts['BAND'] - counts['BELOW1'] if name == 'BAND' else counts[name]), name       # every anchor of the class
        assert int(nt[k]) == wn, (name, int(nt[k]), wn)
        assert np.array_equal(an[k, :wn], wa[:wn]), name
        assert np.array_equal(tr[k, :wn], wt[:wn], equal_nan=True), name
        linked = ~np.isnan(tr[k, :wn, 0, 0])
        assert np.array_equal(linked, ~np.isnan(tr[k, :wn, 2, 0]))
        # the chain continues on UP / ABOVE1 / ZERO and stops on the pairs the fallback must keep apart
        assert linked.all() if name in ('UP', 'ABOVE1', 'ZERO') else not linked.any(), name


@pytest.mark.parametrize("link_thres,B,wide", [(0.3, 1100, False), (0.7, 1100, True), (0.5, 300, False), (0.45, 300, False)])
def test_links_on_the_knife_edge(torch_cuda, oracle, link_thres, B, wide):
    """B = 1 100: frames too large for the up-front link table, every chain scans (link_scan16 on the compact u16 index,
    link_scan on the float4 one); B = 300: link_fill_frame's table.  Rows, anchors and counts bit-equal to the oracle's."""
    from vdetlib_amd import ops
    torch = torch_cuda
    boxes, scores, counts = _link_video(link_thres, B, 31, wide)
    tr, an, nt = ops.track_volume(torch.from_numpy(boxes.copy()).cuda(), torch.from_numpy(scores.copy()).cuda(), nms_thres=0.3, thres=0.5,
                                  max_tracks=64, link_thres=link_thres)
    _check_tracks(oracle, boxes, scores, link_thres, tr.cpu().numpy(), an.cpu().numpy(), nt.cpu().numpy(), counts)


def test_links_without_the_index(torch_cuda, oracle, monkeypatch):
    from vdetlib_amd import ops, _lib
    torch = torch_cuda
    monkeypatch.setenv("VDET_NO_INDEX", "1")
    cx = _lib.Context(torch.cuda.current_device())
    try:
        boxes, scores, counts = _link_video(0.3, 1100, 31, False)
        tr, an, nt = ops.track_volume(torch.from_numpy(boxes.copy()).cuda(), torch.from_numpy(scores.copy()).cuda(), nms_thres=0.3, thres=0.5,
                                      max_tracks=64, link_thres=0.3, ctx=cx)
        _check_tracks(oracle, boxes, scores, 0.3, tr.cpu().numpy(), an.cpu().numpy(), nt.cpu().numpy(), counts)
    finally:
        cx.close()


@pytest.mark.parametrize("link_thres", [0.3, 0.5, 0.7, 0.45])
def test_links_in_a_video_batch(torch_cuda, oracle, link_thres):
    """Two such videos in one vdet_video_batch call: the batch tracker's table scan."""
    from vdetlib_amd import ops
    torch = torch_cuda
    vids = [_link_video(link_thres, 300, 41 + v, False) for v in range(2)]
    boxes = np.concatenate([v[0] for v in vids]); scores = np.concatenate([v[1] for v in vids])
    out = ops.video_batch(torch.from_numpy(boxes).cuda(), torch.from_numpy(scores).cuda(), [0, 3, 6], nms_thres=0.3, thres=0.5,
                          max_tracks=64, link_thres=link_thres, rescore=False)
    for v in range(2):
        _check_tracks(oracle, vids[v][0], vids[v][1], link_thres, out['tracks'][v].cpu().numpy(), out['anchors'][v].cpu().numpy(),
                      out['ntracks'][v].cpu().numpy(), vids[v][2])
    widx, wcnt = oracle.nms_volume(boxes, scores, 0.3)
    assert np.array_equal(out['keep_cnt'].cpu().numpy(), wcnt) and np.array_equal(out['keep_idx'].cpu().numpy(), widx)
