"""-m gpu: the x-bucket windows -- which boxes of a regular frame a stage looks at AT ALL -- at every site that takes one,
against the oracle, on frames whose true partners sit on the window's edge and on a 64-rank word boundary.

A regular frame is walked through its x-sorted index: 256 x1-buckets (frame_index_kernel, xbucket in csrc/nms_kernels.hpp)
and a lo / hi bound derived from the IoU threshold.  A window that is too tight drops a suppression, a link or a re-scoring
candidate without a fault.  The window is written three times:
  A  adj_build_kernel (csrc/nms_kernels.hpp): float32, 1.001 relative + 2 px, read at the granularity of 64-rank words;
  B  xwindow() (csrc/nms_kernels.hpp): float64, 1.001 + 1 px, by rank -- rescore_one_scan (ops.rescore_tracks),
     rescore_tubelets_spatial_kernel (ops.rescore_tubelets[_batch]) and the tracker's first-visit sweep over a list of
     more than 2048 candidates (track_suppress in csrc/track_kernels.hpp, under VDET_NO_LAZY=1);
  C  the link scans (csrc/track_kernels.hpp): float32, omt = (1 - t) * 1.002 + 1e-6, + 2 px, the current box truncated --
     link_fill_frame (frames of at most 1024 boxes) and track_link_memo_body (larger ones), and their batch forms.
tests/knife_spec.py builds the frames (window_frame: families unit, top, wmaxcap, coarse, frac, flat) and restates the three
windows (window_model); tests/test_knife_edge_cpu.py shows that the windows as written hold every pinned pair and that each
of these single-token mistakes loses one: own width on the left, cum[b1], r1 >> 6, (r0 + 63) >> 6, the clamp at bucket 254,
one pixel inward.  (Two more, wmax without its + 1 and the link scans' 2 px replaced by 0, cannot lose a pair on any frame:
K.WINDOW_UNKILLABLE.)  Here the kernels run those frames; every comparison is exact.

ops.track_from_anchors takes no window (anchor_link_kernel scans whole frames); it is run on the link videos as a second
statement of the rows the windowed scans have to produce.
"""
import functools

import numpy as np
import pytest

import knife_spec as K
import rescore_spec as R

pytestmark = pytest.mark.gpu

F32 = np.float32
TS = K.WINDOW_THRESHOLDS
FAMILIES = K.WINDOW_FAMILIES
SEED = K.WINDOW_SEED
# 322: one block per 256-row tile (nmax <= 384) and link_fill_frame (B <= 1024); 642: adj_build_kernel<kAdjRows>;
# 1026: track_link_memo_body; 2114: a candidate list of more than 2048 entries
TILE, HALVES, SCAN, SWEEP = K.WINDOW_B
FILL = TILE


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


def g(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def n_(x):
    return x.cpu().numpy()


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind == 'f')


def _context(torch, monkeypatch, knobs):
    from vdetlib_amd import _lib
    for knob in knobs:
        name, _, val = knob.partition('=')
        monkeypatch.setenv(name, val)
    return _lib.Context(torch.cuda.current_device())


@functools.lru_cache(maxsize=None)
def _frames(t, B, strict):
    """[(boxes [B, 4], pair rows)] of every family, in the order of FAMILIES."""
    return [K.window_frame(t, B, fam, SEED, strict) for fam in FAMILIES]


# ---- site A: the adjacency rows ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _volume(t, B):
    """boxes [7, B, 4], scores [7, B, 3]: one frame per family and, last, the 'unit' frame with a NaN box in place of its last
    filler (irregular: the general predicate kernel and adj_build_kernel's own rows, in the launch that skips -- or builds --
    the regular frames).  Score columns (K.pair_scores): O directly above I, I directly above O, a random permutation."""
    frames = _frames(t, B, False)
    boxes = [fr for fr, _ in frames] + [frames[0][0].copy()]
    boxes[-1][B - 1] = [np.nan, 5.0, 50.0, 60.0]
    scores = [K.pair_scores(pr.shape[0], B - 2 * pr.shape[0], 900 + k) for k, (_, pr) in enumerate(frames)]
    scores.append(scores[0])
    boxes, scores = np.stack(boxes), np.stack(scores)
    boxes.setflags(write=False); scores.setflags(write=False)
    return boxes, scores


@functools.lru_cache(maxsize=None)
def _want_nms(t, B):
    from oracle import oracle
    oracle.build()
    boxes, scores = _volume(t, B)
    widx, wcnt = oracle.nms_volume(boxes, scores, t)
    # the pins decide: in the column where a pair's first box scores directly above the second, the second is not kept
    for f, (fr, pr) in enumerate(_frames(t, B, False)):
        for c in (0, 1):
            kept = set(widx[f, c, :wcnt[f, c]].tolist())
            assert all(int(p[c]) in kept and int(p[1 - c]) not in kept for p in np.sort(pr, 1)), (f, c)
    return widx, wcnt


A_KNOBS = {
    'default': (),
    'lane_per_row': ('VDET_DIRECT_LISTS=0', 'VDET_ADJ_ROWS=0'),
    'lane_per_row_large_walk': ('VDET_DIRECT_LISTS=0', 'VDET_ADJ_ROWS=0', 'VDET_SMALL_LISTS=0'),
    'no_index': ('VDET_NO_INDEX=1',),
}


@pytest.mark.parametrize("knobs", sorted(A_KNOBS))
@pytest.mark.parametrize("B", [TILE, HALVES])
@pytest.mark.parametrize("t", TS)
def test_adjacency_rows_read_the_whole_window(torch_cuda, oracle, monkeypatch, t, B, knobs):
    """Site A.  Keep lists and counts of ops.nms_volume equal to oracle.nms_volume on all families in one volume.
    B = 642 with VDET_DIRECT_LISTS=0 + VDET_ADJ_ROWS=0 ('lane_per_row'): adj_build_kernel<kAdjRows> builds the rows of the
    regular frames (two blocks per 256-row tile; skip_regular = 0) from the bit matrix of iou_bits_sym_kernel.
    B = 322 (nmax <= 384, any switches): adj_build_kernel<kRowsPerTile>, one block per tile; VDET_SMALL_LISTS=0
    ('lane_per_row_large_walk') sends its lists through the large-list sort and walk instead of the small-list walk.
    'default' at B = 642: the direct lists (graph_lists_kernel + adj_finish_kernel), adj_build_kernel<kAdjRows> with
    skip_regular = 1 for the irregular frame only.  'no_index': VDET_NO_INDEX=1 (the graph build keeps its index; the
    switch is the tracker's and re-scoring's, the volume must not change).
    The last frame holds a NaN box: skip_regular and the general rows share the launch."""
    from vdetlib_amd import ops
    boxes, scores = _volume(t, B)
    widx, wcnt = _want_nms(t, B)
    cx = _context(torch_cuda, monkeypatch, A_KNOBS[knobs])
    try:
        idx, cnt = ops.nms_volume(g(boxes), g(scores), t, ctx=cx)
        assert np.array_equal(n_(cnt), wcnt), (t, B, knobs)
        assert np.array_equal(n_(idx), widx), (t, B, knobs)
    finally:
        cx.close()


# ---- site B: xwindow() ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _rescore_case(t, B):
    """boxes [6, B, 4] (the strict frames: float64 IoU > t for every pinned pair), scores [6, B, 2] (O above I / I above O),
    tracks [2, T, 6, 5] caller-supplied hole-free tubelets, the same in both classes.  Slots 0 .. npin - 1: per frame a pinned
    box (pinned row s modulo the frame's number).  Then O of pair 0 moved right by a quarter pixel and I of pair 0 moved left
    by half a pixel.  Then eight slots of free boxes that can hit nothing -- wholly left of xmin, wholly right of xmax, wider
    than wmax / t, one pixel; each kind twice -- alternating from frame to frame with a pinned box that hits: one slot of a
    kind has its misses on frames 0, 2, 4, the other on 1, 3, 5, so that every kind meets every family and completion sees
    leading, interior and trailing gaps but no tubelet of misses alone."""
    frames = _frames(t, B, True)
    boxes = np.stack([fr for fr, _ in frames])
    scores = np.stack([K.pair_scores(pr.shape[0], B - 2 * pr.shape[0], 950 + k)[:, :2] for k, (_, pr) in enumerate(frames)])
    npin = max(2 * pr.shape[0] for _, pr in frames)
    T = npin + 2 + 8
    tracks = np.full((2, T, len(frames), 5), np.nan, F32)
    tracks[..., 4] = 0.5
    for f, (fr, pr) in enumerate(frames):
        for s in range(npin):
            tracks[:, s, f, :4] = fr[s % (2 * pr.shape[0])]
        O, I = fr[pr[0, 0]], fr[pr[0, 1]]
        tracks[:, npin, f, :4] = O + np.array([0.25, 0, 0.25, 0], F32)
        tracks[:, npin + 1, f, :4] = I - np.array([0.5, 0, 0.5, 0], F32)
        xmin, xmax, wmax = fr[:, 0].min(), fr[:, 0].max(), (fr[:, 2] - fr[:, 0] + 1).max()
        free = [[xmin - 300, 0, xmin - 200, 30], [xmax + 400, 0, xmax + 450, 30],
                [xmin - 50, 0, xmin - 50 + np.ceil(wmax / t) + 200, 30], [I[0], I[1], I[0], I[1]]]
        for j in range(8):
            tracks[:, npin + 2 + j, f, :4] = free[j % 4] if (f + j // 4) % 2 == 0 else fr[j % (2 * pr.shape[0])]
    for x in (boxes, scores, tracks):
        x.setflags(write=False)
    return boxes, scores, tracks, np.full(2, T, np.int32), npin


@functools.lru_cache(maxsize=None)
def _want_rescore(t, B, complete):
    from oracle import oracle
    oracle.build()
    boxes, scores, tracks, nt, npin = _rescore_case(t, B)
    want = R.spec(tracks, nt, boxes, scores, overlap_thres=t, window=3, complete=complete)
    assert not want[4]
    # the pins decide: the box of a pair that scores lower is re-scored by its partner, the other by itself
    src = want[3]
    for f, (fr, pr) in enumerate(_frames(t, B, True)):
        for s in range(2 * pr.shape[0]):
            for c in (0, 1):
                first = s - s % 2 + c
                assert src[c, s, f] == first, (f, s, c, src[c, s, f])
        for j in range(8):          # ... and the free boxes hit nothing, their neighbours in the slot do
            assert np.all((src[:, npin + 2 + j, f] == -1) == ((f + j // 4) % 2 == 0)), (f, j)
    return want


@pytest.mark.parametrize("B", [TILE, HALVES])
@pytest.mark.parametrize("t", TS)
def test_rescore_tubelets_reads_the_whole_window(torch_cuda, oracle, t, B):
    """Site B, rescore_tubelets_spatial_kernel (csrc/rescore_kernels.hpp; the window of xwindow() on every regular frame with
    an index -- index_matches() fails for these boxes, so the call builds flags and index itself, for any B here): det,
    pooled, tboxes and src of ops.rescore_tubelets, raw (complete=False), bit-equal to tests/rescore_spec.py.  Queries: the
    pinned boxes of every family, fractional neighbours of them, free boxes left of xmin, right of xmax
    (b0 = b1 = 0 / 255), wider than wmax / t, one pixel."""
    from vdetlib_amd import ops
    boxes, scores, tracks, nt, _ = _rescore_case(t, B)
    want = _want_rescore(t, B, False)
    got = ops.rescore_tubelets(g(tracks), g(nt), g(boxes), g(scores), overlap_thres=t, window=3, complete=False)
    for k, x, w in zip(('det', 'pooled', 'tboxes', 'src'), got, want):
        assert same(n_(x), w), (k, t, B)


@pytest.mark.parametrize("B", [TILE, HALVES])
@pytest.mark.parametrize("t", TS)
def test_rescore_tracks_reads_the_whole_window(torch_cuda, oracle, t, B):
    """Site B, rescore_spatial_kernel<false> -> rescore_one_scan (csrc/track_kernels.hpp): nodes_match() fails for
    caller-supplied track tensors, so no candidate comes from the graph and every (class, track, frame) takes the window
    scan; index_matches() fails for these boxes, so flags and index are rebuilt for them.  The same queries as
    ops.rescore_tubelets gets, the free boxes included (clamped windows, the all-covering window, the one-pixel query);
    the call completes the gaps they leave.  det, pooled and boxes bit-equal to the specification."""
    from vdetlib_amd import ops
    boxes, scores, tracks, nt, _ = _rescore_case(t, B)
    want = _want_rescore(t, B, True)
    det, pooled, ob = ops.rescore_tracks(g(tracks), g(nt), g(boxes), g(scores), overlap_thres=t, window=3)
    assert same(n_(det), want[0]) and same(n_(pooled), want[1]) and same(n_(ob), want[2]), (t, B)


def test_rescore_tubelets_batch_offsets_the_bucket_tables(torch_cuda, oracle):
    """Site B, the batch form (rescore_tubelets_spatial_kernel with one grid row per video: xwindow() of group
    vd.f0 + f): two videos of three frames whose frames come from different families (unit, top, wmaxcap / coarse, frac,
    flat), so that a cum / info row taken from the wrong group is a window of the wrong frame."""
    from vdetlib_amd import ops
    from test_rescore_tubelets_gpu import batch_dict, check_views
    t, B, off = 0.5, TILE, [0, 3, 6]
    boxes, scores, tracks, nt, _ = _rescore_case(t, B)
    tv = [np.ascontiguousarray(tracks[:, :, off[v]:off[v + 1]]) for v in range(2)]
    ntv = np.stack([nt, nt])
    want, eindex = R.spec_batch(tv, ntv, boxes, scores, off, overlap_thres=t, window=3, complete=False)
    assert not eindex
    out = ops.rescore_tubelets_batch(batch_dict(tv, ntv, off), g(boxes), g(scores), overlap_thres=t, window=3, complete=False)
    check_views(out, want, 'window frames')


@functools.lru_cache(maxsize=None)
def _sweep_video(t):
    """Two frames of 2114 boxes: 'coarse' and 'top'.  Class 0 scores every O directly above its I, class 1 the other way
    round; the second frame's scores are half the first's (no ties across frames)."""
    fams = ('coarse', 'top')
    frames = [K.window_frame(t, SWEEP, fam, SEED, False) for fam in fams]
    boxes = np.stack([fr for fr, _ in frames])
    scores = np.stack([K.pair_scores(pr.shape[0], SWEEP - 2 * pr.shape[0], 970 + k)[:, :2] * F32(1.0 / (k + 1))
                       for k, (_, pr) in enumerate(frames)])
    boxes.setflags(write=False); scores.setflags(write=False)
    return boxes, scores, sum(pr.shape[0] for _, pr in frames)


@functools.lru_cache(maxsize=None)
def _want_sweep(t):
    from oracle import oracle
    oracle.build()
    boxes, scores, npairs = _sweep_video(t)
    T = npairs + 2
    widx, wcnt = oracle.nms_volume(boxes, scores, t)
    tracks = []
    for c in range(2):
        wt, wa, wn = oracle.greedy_track_volume(boxes, scores[:, :, c], t, 0.0, T, 0.5, 0)
        # (the fixture: the first anchors are the higher box of every pair, never the partner it suppresses)
        assert wn == T and np.all(wa[:npairs, 1] % 2 == c) and np.all(wa[:npairs, 1] < 12), wa
        tracks.append((wt, wa, wn))
    return widx, wcnt, tracks


@pytest.mark.parametrize("t", TS)
def test_first_visit_sweep_reads_the_whole_window(torch_cuda, oracle, monkeypatch, t):
    """Site B, the tracker's round-1 sweep (track_suppress, csrc/track_kernels.hpp): under VDET_NO_LAZY=1 the eager
    track_det_nms pass runs on regular frames too, and the first visit of a list of more than 2048 candidates (B = 2114,
    thres = 0: every box is one) sweeps the xwindow() of the track box instead of the list.  Every pinned box that scores
    higher is an anchor; its partner on the window's edge has to die in the sweep, or it becomes the next anchor.
    B > 1024 also means track_link_memo_body links (warm-up <256, 1, 8>, materialisation <64, 2, 8>, the loop).
    Keep lists, tubelets, anchors and counts equal to the oracle's."""
    from vdetlib_amd import ops
    boxes, scores, npairs = _sweep_video(t)
    T = npairs + 2
    cx = _context(torch_cuda, monkeypatch, ('VDET_NO_LAZY=1',))
    try:
        ki, kc, tr, an, nt = ops.nms_track_volume(g(boxes), g(scores), nms_thres=t, thres=0.0, max_tracks=T, link_thres=0.5,
                                                  ctx=cx)
        ki, kc, tr, an, nt = n_(ki), n_(kc), n_(tr), n_(an), n_(nt)
    finally:
        cx.close()
    widx, wcnt, tracks = _want_sweep(t)
    assert np.array_equal(kc, wcnt) and np.array_equal(ki, widx)
    for c, (wt, wa, wn) in enumerate(tracks):
        assert int(nt[c]) == wn and np.array_equal(an[c, :wn], wa[:wn]), (t, c)
        assert np.array_equal(tr[c, :wn], wt[:wn], equal_nan=True), (t, c)


# ---- site C: the link scans ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _link_videos(t, B):
    """Per family two videos of three frames, boxes [3, B, 4], scores [3, B, 2], and the rows of (O, I) per pair.  The middle
    frame holds the CURRENT boxes: the window frame with every pinned box replaced by K.link_query() of it ('frac': moved
    right by 0.75 px, which truncation takes back -- towards the side without a partner for O).  One neighbour frame holds the
    window frame with every O shrunk to one pixel (x1 kept: ranks, buckets and words stay), so that the only candidate
    overlapping O at all is I at the extreme right offset; the other holds it with every I shrunk, so that the only candidate
    of I is O at the extreme left offset (wmax unchanged).  Video 0: (I only, current, O only), video 1 the mirror image --
    either side is scanned forwards once and backwards once.  Class 0 makes anchors of the O, class 1 of the I (the only
    scores above the stop threshold 0.5)."""
    out = []
    for k, (fr, pr) in enumerate(_frames(t, B, False)):
        rng = np.random.RandomState(990 + k)
        cur = fr.copy()
        for r in pr.ravel():
            cur[r] = K.link_query(fr[r]) if FAMILIES[k] == 'frac' else fr[r]
        only = []
        for col in (0, 1):          # shrink the O (col 0) / the I (col 1)
            x = fr.copy()
            x[pr[:, col], 2] = x[pr[:, col], 0]
            x[pr[:, col], 3] = x[pr[:, col], 1]
            only.append(x)
        scores = (rng.permutation(3 * B * 2).reshape(3, B, 2) + 1).astype(F32) / F32(3 * B * 2 * 4)        # all below 0.25
        for c in (0, 1):
            scores[1, pr[:, c], c] = F32(0.95) - np.arange(pr.shape[0], dtype=F32) / F32(256)
        for first, last in ((only[0], only[1]), (only[1], only[0])):
            b = np.stack([first, cur, last])
            b.setflags(write=False)
            out.append((b, scores, pr))
        scores.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _want_links(t, B):
    from oracle import oracle
    oracle.build()
    want = []
    for v, (boxes, scores, pr) in enumerate(_link_videos(t, B)):
        m = pr.shape[0]
        per_class = []
        for c in (0, 1):
            wt, wa, wn = oracle.greedy_track_volume(boxes, scores[:, :, c], 0.3, 0.5, 16, t, 0)
            # every pinned box of the class is an anchor, in the order of its pair, and links to BOTH neighbour frames: to
            # its partner on the window's edge in one, to its own copy in the other
            assert wn == m and np.array_equal(wa[:m, 1], pr[:, c]) and not np.isnan(wt[:m, :, 0]).any(), (v, c)
            side = 0 if (v % 2 == 0) == (c == 0) else 2          # the frame that holds only the partner
            assert np.array_equal(wt[:m, side, :4], np.trunc(boxes[side][pr[:, 1 - c]])), (v, c)
            for k in range(m):      # ... and the rows are the plug-in tracker's from the (truncated) anchor box
                rows = oracle.iou_link_rows_box(boxes, 1, np.trunc(boxes[1, pr[k, c]]), t, 0)
                assert np.array_equal(rows, wt[k], equal_nan=True)
            per_class.append((wt, wa, wn))
        want.append(per_class)
    return want


def _check_links(got, want, what):
    tr, an, nt = got
    for c, (wt, wa, wn) in enumerate(want):
        assert int(nt[c]) == wn, (what, c)
        assert np.array_equal(an[c, :wn], wa[:wn]), (what, c)
        assert np.array_equal(tr[c, :wn], wt[:wn], equal_nan=True), (what, c)


@pytest.mark.parametrize("B", [FILL, SCAN])
@pytest.mark.parametrize("t", TS)
def test_link_scans_read_the_whole_window(torch_cuda, oracle, t, B):
    """Site C, ops.track_volume on every family, both sides, both directions.  B = 322 (<= kLinkFillMax with an index):
    link_fill_frame_kernel fills the whole link table from LDS.  B = 1026: track_link_memo_kernel -- the warm-up
    <256, 1, 8>, the materialisation <64, 2, 8> and the loop's scans -- with link_scan16 on the compact u16 index of the
    whole-pixel families and link_scan on the float4 index of 'frac'.  Tubelets, anchors and counts equal to
    oracle.greedy_track_volume, whose rows are oracle.iou_link_rows_box's; ops.track_from_anchors (no window) from the same
    anchor boxes gives the same rows."""
    from vdetlib_amd import ops
    want = _want_links(t, B)
    for v, (boxes, scores, pr) in enumerate(_link_videos(t, B)):
        tb = g(boxes)
        tr, an, nt = ops.track_volume(tb, g(scores), nms_thres=0.3, thres=0.5, max_tracks=16, link_thres=t)
        _check_links((n_(tr), n_(an), n_(nt)), want[v], (t, B, FAMILIES[v // 2], v % 2))
        m = pr.shape[0]
        af = np.ones((2, m), np.int32) * 2                                       # (1-based: the middle frame)
        ab = np.stack([boxes[1, pr[:, c]] for c in (0, 1)])
        rows = n_(ops.track_from_anchors(tb, g(af), g(ab), link_thres=t)[0])
        for c in (0, 1):
            assert np.array_equal(rows[c, :m], want[v][c][0][:m], equal_nan=True), (t, B, v, c)


@pytest.mark.parametrize("t,B", [(0.5, FILL), (0.7, SCAN)])
def test_link_scans_in_a_video_batch(torch_cuda, oracle, t, B):
    """Site C, the batch form: the twelve videos in one ops.video_batch call -- batch_link_fill_frame_kernel (B = 322) /
    batch_link_kernel<256, 1> and <64, 2> (B = 1026), each video with the bucket tables of its own frames."""
    from vdetlib_amd import ops
    vids = _link_videos(t, B)
    want = _want_links(t, B)
    boxes = np.concatenate([v[0] for v in vids]); scores = np.concatenate([v[1] for v in vids])
    off = [3 * v for v in range(len(vids) + 1)]
    out = ops.video_batch(g(boxes), g(scores), off, nms_thres=0.3, thres=0.5, max_tracks=16, link_thres=t, rescore=False)
    for v in range(len(vids)):
        _check_links((n_(out['tracks'][v]), n_(out['anchors'][v]), n_(out['ntracks'][v])), want[v], (t, B, v))
