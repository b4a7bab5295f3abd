"""-m gpu: the argument checks of the per-video entry points of libvdet_hip.so, called through the C ABI with NULL for every
device pointer, so that no call can reach a launch whichever way a check falls (host work only: milliseconds).  Host tables
(frame offsets, net parameters) are real and tiny.

Every limit of the library is "a product of caller-supplied sizes stays below (or at) 2^31 - 16".  For each entry point one
named product is put at the largest value the library accepts -- the call is then refused with "null buffer": the limit check
passed -- and one step above it, where the call is refused with the site's own limit text.  Batch symbols take the offsets
[0, 1] and [0, 1, 3] with B = 1; with three frames the products move in steps of 3, so "at the boundary" is the largest
multiple below it.  The single-video symbols take the frame count itself as the free factor.

THE WRAPPING CASE of every entry point (C = 2^44 with T = 2^20, or three factors whose product is 2^64) is the defect the one
overflow-safe limit check closes: the factors used to be multiplied before they were compared, C * T == 0 in int64_t passed
every limit, and only the null-buffer check stood between such a call and a launch -- these calls used to end in "null
buffer".  They are refused with the text of the first limit they break.  (Where the entry point also limits V*C on its own --
vdet_nms_tracks, vdet_rescore_tubelets -- or guarded its products by division already -- vdet_seq_nms -- the limit text is what
the call got before as well; the case pins it.)

Bad offsets (not from 0, decreasing, an empty video, V = 0, V = 65536) are refused with check_frame_off's texts by every batch
symbol.  vdet_top_anchors reads its offsets behind its null-buffer check, so they cannot be reached without device memory; the
two evaluation forms need a ground-truth table on the device before any limit is looked at.  Both are left out here.

Last, the anchor route's single-video symbols are the batch symbols with frame_off = [0, F]: bit-identical outputs on device
tensors, and neither stages a per-video table (vdet_query 11)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

L = 0x7FFFFFF0                    # 2^31 - 16
N = None                          # a null device pointer
NULL, LIMIT, SHAPE = r"null buffer", r"2\^31|too many|too large", r"bad shape"
OFF1, OFF2 = [0, 1], [0, 1, 3]
THIRD = (L - 1) // 3              # 3 * THIRD == L - 1: the largest C with C*1*3 below L, and not above it either


@pytest.fixture(scope="module")
def cx():
    from vdetlib_amd import _lib
    c = _lib.Context()
    yield c
    c.close()


def _off(off):
    return np.asarray(off, dtype=np.int64)


# ---- one caller per symbol: (ctx, offsets or F, sizes...) -> rc.  Thresholds, windows and flags are valid constants.
def interp_b(cx, off, C, T, V=None):
    o, V = _off(off), len(off) - 1 if V is None else V
    return cx.lib.vdet_interp_tracks_batch(cx.h, o.ctypes.data, o.ctypes.data, V, N, C, T, N, N, N, N, N, 0, 0, N, N, N, N, N, N)


def interp_1(cx, F, C, T):
    return cx.lib.vdet_interp_tracks(cx.h, F, F, N, C, T, N, N, N, N, N, 0, 0, N, N, N, N, N, N)


def track_b(cx, off, C, T, B=1, V=None):
    o, V = _off(off), len(off) - 1 if V is None else V
    return cx.lib.vdet_track_from_anchors_batch(cx.h, N, o.ctypes.data, V, B, N, N, N, C, T, 0.5, 0, N, N, N)


def track_1(cx, F, C, T, B=1):
    return cx.lib.vdet_track_from_anchors(cx.h, N, F, B, N, N, N, C, T, 0.5, 0, N, N, N)


def prop_b(cx, off, C, T, B=1, V=None):
    o, V = _off(off), len(off) - 1 if V is None else V
    return cx.lib.vdet_anchor_propagate_tracks_batch(cx.h, N, N, N, N, N, o.ctypes.data, V, B, C, T, N, N)


def prop_1(cx, F, C, T, B=1):
    return cx.lib.vdet_anchor_propagate_tracks(cx.h, N, N, N, N, N, F, B, C, T, N, N)


def top_1(cx, F, C, T, B=1):
    return cx.lib.vdet_top_anchors(cx.h, N, N, F, B, C, T, 0, 0, 0.0, N, 0, N, N, N, N)


def merge_b(cx, off, C, T, V=None):             # 'combine' of Ta = T and Tb = 0 slots: the output's T is T
    o, V = _off(off), len(off) - 1 if V is None else V
    return cx.lib.vdet_merge_tracks_batch(cx.h, 0, o.ctypes.data, V, C, T, 0, N, N, N, N, N, N, N, N, N, N, 1, N, N, N, N, N, N)


def merge_1(cx, F, C, T):
    return cx.lib.vdet_merge_tracks(cx.h, 0, F, C, T, 0, N, N, N, N, N, N, N, N, N, N, 1, N, N, N, N, N, N)


def nms_b(cx, off, C, T, R=1, V=None):
    o, V = _off(off), len(off) - 1 if V is None else V
    return cx.lib.vdet_nms_tracks_batch(cx.h, o.ctypes.data, V, C, T, N, N, N, 0, N, N, N, 1, N, N, 0, 0, 0.5, R, N, N, N, N, N)


def nms_1(cx, F, C, T, R=1):
    return cx.lib.vdet_nms_tracks(cx.h, F, C, T, N, N, N, 0, N, N, N, 1, N, N, 0, 0, 0.5, R, N, N, N, N, N)


def rescore_b(cx, off, C, T, B=1, V=None):
    o, V = _off(off), len(off) - 1 if V is None else V
    return cx.lib.vdet_rescore_tubelets_batch(cx.h, o.ctypes.data, V, B, C, T, N, N, N, N, N, 0, 0.5, 0, 3, N, N, N, N)


def rescore_1(cx, F, C, T, B=1):
    return cx.lib.vdet_rescore_tubelets(cx.h, F, B, C, T, N, N, N, N, N, 0, 0.5, 0, 3, N, N, N, N)


def seq_b(cx, off, C, R, S=1, V=None):
    o, V = _off(off), len(off) - 1 if V is None else V
    return cx.lib.vdet_seq_nms_batch(cx.h, o.ctypes.data, V, C, R, N, N, N, 0, 0.5, 0.3, 0, S, 0.0, N, N, N, N, N, N, N, N, N)


def seq_1(cx, F, C, R, S=1):
    return cx.lib.vdet_seq_nms(cx.h, F, C, R, N, N, N, 0, 0.5, 0.3, 0, S, 0.0, N, N, N, N, N, N, N, N, N)


# a net of one layer, 1 -> 2 channels, kernel 1, on the track-score channel (code 1: no ground truth, no detection scores)
_PARAMS = np.zeros(4, dtype=np.float32)
_LAYERS = np.asarray([2, 1, 1], dtype=np.int32)
_CHANNELS = np.asarray([1], dtype=np.int32)


def tcn_b(cx, off, C, T, V=None):
    o, V = _off(off), len(off) - 1 if V is None else V
    return cx.lib.vdet_tcn_tracks_batch(cx.h, _PARAMS.ctypes.data, _LAYERS.ctypes.data, 1, _CHANNELS.ctypes.data, 1, o.ctypes.data,
                                        V, C, T, N, N, N, N, 0, N, N)


def tcn_1(cx, F, C, T):
    return cx.lib.vdet_tcn_tracks(cx.h, _PARAMS.ctypes.data, _LAYERS.ctypes.data, 1, _CHANNELS.ctypes.data, 1, F, C, T, N, N, N, N, 0,
                                  N, N)


BATCH = dict(interp=interp_b, track=track_b, propagate=prop_b, merge=merge_b, nms=nms_b, rescore=rescore_b, seq=seq_b, tcn=tcn_b)

# (caller, positional sizes after ctx, keyword sizes, the text the refusal must match)
CASES = {
    # ---- C*T*F, accepted up to L (">"): interpolation, the anchor route, the TCN.  Interpolation and the TCN look at C*T alone
    # first and call that "bad shape", so their C*T*F boundary shows with three frames only
    'interp_b F=3 at': (interp_b, (OFF2, THIRD, 1), {}, NULL), 'interp_b F=3 above': (interp_b, (OFF2, THIRD + 1, 1), {}, LIMIT),
    'interp_b C*T at': (interp_b, (OFF1, L, 1), {}, NULL), 'interp_b C*T above': (interp_b, (OFF1, L + 1, 1), {}, SHAPE),
    'interp_1 at': (interp_1, (L, 1, 1), {}, NULL), 'interp_1 above': (interp_1, (L + 1, 1, 1), {}, LIMIT),
    'tcn_b F=3 at': (tcn_b, (OFF2, THIRD, 1), {}, NULL), 'tcn_b F=3 above': (tcn_b, (OFF2, THIRD + 1, 1), {}, LIMIT),
    'tcn_b C*T at': (tcn_b, (OFF1, L, 1), {}, NULL), 'tcn_b C*T above': (tcn_b, (OFF1, L + 1, 1), {}, SHAPE),
    'tcn_1 at': (tcn_1, (L, 1, 1), {}, NULL), 'tcn_1 above': (tcn_1, (L + 1, 1, 1), {}, LIMIT),
    'track_b F=1 at': (track_b, (OFF1, L, 1), {}, NULL), 'track_b F=1 above': (track_b, (OFF1, L + 1, 1), {}, LIMIT),
    'track_b F=3 at': (track_b, (OFF2, THIRD, 1), {}, NULL), 'track_b F=3 above': (track_b, (OFF2, THIRD + 1, 1), {}, LIMIT),
    'track_1 F*B at': (track_1, (L, 1, 1), {}, NULL), 'track_1 F*B above': (track_1, (L + 1, 1, 1), {}, LIMIT),
    'track_1 C*T*F at': (track_1, (2, L // 2, 1), {}, NULL), 'track_1 C*T*F above': (track_1, (2, L // 2 + 1, 1), {}, LIMIT),
    'prop_b F=1 at': (prop_b, (OFF1, L, 1), {}, NULL), 'prop_b F=1 above': (prop_b, (OFF1, L + 1, 1), {}, LIMIT),
    'prop_b F=3 at': (prop_b, (OFF2, THIRD, 1), {}, NULL), 'prop_b F=3 above': (prop_b, (OFF2, THIRD + 1, 1), {}, LIMIT),
    'prop_1 F*B at': (prop_1, (L, 1, 1), {}, NULL), 'prop_1 F*B above': (prop_1, (L + 1, 1, 1), {}, LIMIT),
    'prop_1 C*T*F at': (prop_1, (2, L // 2, 1), {}, NULL), 'prop_1 C*T*F above': (prop_1, (2, L // 2 + 1, 1), {}, LIMIT),
    # ---- F*B, accepted up to L: the anchor selection (its slots are counted behind the null-buffer check)
    'top at': (top_1, (L, 1, 1), {}, NULL), 'top above': (top_1, (L + 1, 1, 1), {}, LIMIT),
    # ---- C*T*F (nms: and C*R*F), accepted below L (">="): merge, tubelet NMS, re-scoring
    'merge_b F=1 at': (merge_b, (OFF1, L - 1, 1), {}, NULL), 'merge_b F=1 above': (merge_b, (OFF1, L, 1), {}, LIMIT),
    'merge_b F=3 at': (merge_b, (OFF2, THIRD, 1), {}, NULL), 'merge_b F=3 above': (merge_b, (OFF2, THIRD + 1, 1), {}, LIMIT),
    'merge_1 at': (merge_1, (L - 1, 1, 1), {}, NULL), 'merge_1 above': (merge_1, (L, 1, 1), {}, LIMIT),
    'nms_b C*T*F at': (nms_b, (OFF1, L - 1, 1), {}, NULL), 'nms_b C*T*F above': (nms_b, (OFF1, L, 1), {}, LIMIT),
    'nms_b C*R*F at': (nms_b, (OFF2, (L - 1) // 6, 1), dict(R=2), NULL), 'nms_b C*R*F above': (nms_b, (OFF2, (L - 1) // 6 + 1, 1), dict(R=2), LIMIT),
    'nms_1 at': (nms_1, (L - 1, 1, 1), {}, NULL), 'nms_1 above': (nms_1, (L, 1, 1), {}, LIMIT),
    'rescore_b F=1 at': (rescore_b, (OFF1, L - 1, 1), {}, NULL), 'rescore_b F=1 above': (rescore_b, (OFF1, L, 1), {}, LIMIT),
    'rescore_b F=3 at': (rescore_b, (OFF2, THIRD, 1), {}, NULL), 'rescore_b F=3 above': (rescore_b, (OFF2, THIRD + 1, 1), {}, LIMIT),
    'rescore_1 at': (rescore_1, (L - 1, 1, 1), {}, NULL), 'rescore_1 above': (rescore_1, (L, 1, 1), {}, LIMIT),
    # ---- Seq-NMS, all below L: boxes C*R*F, link words C*R*F*ceil(R/32) (R = 33: two words), sequences C*max_seqs*V
    'seq_b boxes at': (seq_b, (OFF1, L - 1, 1), {}, NULL), 'seq_b boxes above': (seq_b, (OFF1, L, 1), {}, r"too many boxes"),
    'seq_b words at': (seq_b, (OFF1, (L - 1) // 66, 33), {}, NULL), 'seq_b words above': (seq_b, (OFF1, (L - 1) // 66 + 1, 33), {}, r"too many link words"),
    'seq_b seqs at': (seq_b, (OFF2, (L - 1) // 4, 1), dict(S=2), NULL), 'seq_b seqs above': (seq_b, (OFF2, (L - 1) // 4 + 1, 1), dict(S=2), r"too many sequences"),
    'seq_1 at': (seq_1, (L - 1, 1, 1), {}, NULL), 'seq_1 above': (seq_1, (L, 1, 1), {}, r"too many boxes"),
    # ---- products that wrap int64_t: 2^44 * 2^20 == 0, 2^22 * 2^42 == 0, 2^50 * 2^14 == 0, 2^62 * 4 == 0
    'wrap interp_b': (interp_b, (OFF2, 1 << 44, 1 << 20), {}, SHAPE), 'wrap interp_1': (interp_1, (1 << 42, 1 << 22, 1), {}, LIMIT),
    'wrap tcn_b': (tcn_b, (OFF2, 1 << 44, 1 << 20), {}, SHAPE), 'wrap tcn_1': (tcn_1, (1 << 42, 1 << 22, 1), {}, LIMIT),
    'wrap track_b': (track_b, (OFF2, 1 << 44, 1 << 20), {}, LIMIT), 'wrap track_1': (track_1, (1, 1 << 44, 1 << 20), {}, LIMIT),
    'wrap track_1 F*B': (track_1, (1 << 50, 1, 1), dict(B=1 << 14), LIMIT),
    'wrap prop_b': (prop_b, (OFF2, 1 << 44, 1 << 20), {}, LIMIT), 'wrap prop_1': (prop_1, (1, 1 << 44, 1 << 20), {}, LIMIT),
    'wrap top': (top_1, (1 << 50, 1, 1), dict(B=1 << 14), LIMIT),
    'wrap merge_b': (merge_b, (OFF2, 1 << 44, 1 << 20), {}, LIMIT), 'wrap merge_1': (merge_1, (1, 1 << 44, 1 << 20), {}, LIMIT),
    'wrap nms_b': (nms_b, (OFF1, 1 << 62, 4), dict(R=4), LIMIT), 'wrap nms_1': (nms_1, (1 << 31, 1 << 31, 4), dict(R=4), LIMIT),
    'wrap rescore_b': (rescore_b, (OFF2, 1 << 44, 1 << 20), {}, LIMIT), 'wrap rescore_1': (rescore_1, (1, 1 << 44, 1 << 20), {}, LIMIT),
    'wrap seq_b': (seq_b, (OFF1, 1 << 62, 4), {}, LIMIT), 'wrap seq_1': (seq_1, (1 << 31, 1 << 31, 4), {}, LIMIT),
}


def _refusal(cx, rc):
    from vdetlib_amd import _lib
    assert rc == _lib.VDET_EINVAL, rc           # never VDET_OK: with null pointers that would be a launch
    return cx.error()


@pytest.mark.parametrize("name", sorted(CASES))
def test_limit_boundaries_and_wrapping_products(cx, name):
    import re
    fn, sizes, kw, want = CASES[name]
    msg = _refusal(cx, fn(cx, *sizes, **kw))
    assert re.search(want, msg), (name, msg)
    if want != NULL:
        assert "null buffer" not in msg, (name, msg)


BAD_OFFSETS = {
    'not from 0': ([1, 2], 1, r"frame_off must start at 0"),
    'decreasing': ([0, 2, 1], 2, r"frame_off must be strictly increasing"),
    'an empty video': ([0, 1, 1], 2, r"frame_off must be strictly increasing"),
    'no video': ([0, 1], 0, r"at least one video with its frame offsets"),
    'too many videos': (list(range(65537)), 65536, r"at most 65535 videos in one call"),
}


@pytest.mark.parametrize("sym", sorted(BATCH))
@pytest.mark.parametrize("what", sorted(BAD_OFFSETS))
def test_batch_symbols_refuse_bad_offsets(cx, sym, what):
    import re
    off, V, want = BAD_OFFSETS[what]
    msg = _refusal(cx, BATCH[sym](cx, off, 1, 1, V=V))
    assert re.search(want, msg), (sym, what, msg)


def _bits(t):
    import torch
    return t.contiguous().view(torch.int64 if t.element_size() == 8 else torch.int32)


def test_anchor_route_single_is_the_batch_of_one(cx):
    """F = 3, B = 5, C = 2, T = 2; class 0 has an anchor on the last frame and an empty slot, class 1 two live slots."""
    import torch
    from vdetlib_amd import ops
    F, B, C, T = 3, 5, 2, 2
    g = torch.Generator().manual_seed(77)
    xy = torch.rand((F, B, 2), generator=g) * 40.0
    boxes = torch.cat([xy, xy + 20.0 + torch.rand((F, B, 2), generator=g) * 20.0], dim=2).float().cuda()
    scores = torch.rand((F, B, C), generator=g).float().cuda()
    aframes = torch.tensor([[3, 0], [1, 2]], dtype=torch.int32).cuda()
    pick = torch.tensor([[4, 0], [1, 2]])
    aboxes = torch.stack([torch.stack([boxes[max(int(aframes[c, t]) - 1, 0), int(pick[c, t])] for t in range(T)]) for c in range(C)])
    aboxes[0, 1] = 0.0
    ascores = torch.tensor([[0.9, 0.0], [0.7, 0.6]], dtype=torch.float32).cuda()
    uploads = cx.query(11)
    tracks, anchors, ntracks = ops.track_from_anchors(boxes, aframes, aboxes, ascores, ctx=cx)
    det, best = ops.anchor_propagate_tracks(tracks, ntracks, anchors, boxes, scores, ctx=cx)
    out = ops.track_from_anchors_batch(boxes, [0, F], aframes[None], aboxes[None], ascores[None], ctx=cx)
    bdet, bbest = ops.anchor_propagate_tracks_batch(out, boxes, scores, ctx=cx)
    assert cx.query(11) == uploads                  # one video travels in the kernel arguments: no table is staged
    assert torch.isnan(tracks[0, 1]).all() and not torch.isnan(tracks[0, 0, F - 1]).any() and ntracks.tolist() == [1, 2]
    assert torch.equal(_bits(out['tracks'][0]), _bits(tracks))
    assert torch.equal(_bits(out['anchors'][0]), _bits(anchors)) and torch.equal(out['ntracks'][0], ntracks)
    assert torch.equal(_bits(bdet[0]), _bits(det)) and torch.equal(bbest[0], best)
    assert torch.isnan(det[0, 1]).all() and best[0, 1].item() == -1
