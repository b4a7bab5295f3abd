"""Shared by tests/test_temporal_seams_cpu.py and tests/test_temporal_seams_gpu.py (imports no torch): float32 references of
the temporal operators written from their definition, the sort-key reference, a score volume whose special values do not
depend on where a frame-chunk seam falls, video-border tables, the case lists, and ``chunk_plan`` -- a restatement of the
host's chunk formulas that only guards the CASES (does this shape still produce the seams it was picked for?)."""
import functools

import numpy as np

F32 = np.float32


# ------------------------------------------------------------------------------------------------
# references
# ------------------------------------------------------------------------------------------------
def _window(vol, W, pad, frame_off):
    """[vol[f + k - W//2] for k in range(W)], a frame outside frame f's own video replaced by ``pad``"""
    vol = np.asarray(vol, dtype=F32)
    F = vol.shape[0]
    H = W // 2
    if frame_off is None:
        first, last = np.zeros(F, dtype=np.int64), np.full(F, F, dtype=np.int64)
    else:
        off = np.asarray(frame_off, dtype=np.int64)
        first, last = np.repeat(off[:-1], np.diff(off)), np.repeat(off[1:], np.diff(off))
        assert first.shape[0] == F
    f = np.arange(F)
    wide = (F,) + (1,) * (vol.ndim - 1)
    out = []
    for k in range(W):
        g = f + k - H
        inside = ((g >= first) & (g < last)).reshape(wide)
        out.append(np.where(inside, vol[np.clip(g, 0, F - 1)], F32(pad)))
    return out


def ref_maxpool(vol, W, pad, frame_off=None):
    """centred sliding max along axis 0; NaN propagates (np.max)"""
    return np.max(np.stack(_window(vol, W, pad, frame_off)), axis=0)


def ref_conv(vol, taps, bias, pad, frame_off=None):
    """out[f] = bias + sum_k taps[k] * vol[f + k - K//2], left to right, every step rounded to float32 (no fused
    multiply-add: numpy multiplies and adds in two ufunc calls)"""
    t = np.asarray(taps, dtype=F32)
    v = _window(vol, t.shape[0], pad, frame_off)
    acc = np.full(v[0].shape, F32(bias), dtype=F32)
    with np.errstate(invalid='ignore', over='ignore'):
        for k in range(t.shape[0]):
            acc = acc + F32(t[k]) * v[k]
    return acc


def score_key(s):
    """sortable key of a float32 score (csrc/nms_kernels.hpp score_key): larger = earlier; -0.0 == +0.0; NaN first"""
    s = np.asarray(s, dtype=np.float32).copy()
    s[s == 0] = 0.0
    b = s.view(np.uint32)
    k = np.where(b & 0x80000000, ~b, b | 0x80000000).astype(np.uint32)
    k[np.isnan(s)] = 0xFFFFFFFF
    return k


def expected(scores_fbc, thr=None):
    """[F,B,C] -> order [F,C,B], ncand [F,C]: descending key, ties by descending index; non-candidates last"""
    F, B, C = scores_fbc.shape
    order = np.empty((F, C, B), dtype=np.int64)
    ncand = np.empty((F, C), dtype=np.int32)
    idx = np.arange(B)
    for f in range(F):
        for c in range(C):
            col = scores_fbc[f, :, c]
            k = score_key(col).astype(np.int64)
            if thr is not None:
                k[~(col > np.float32(thr))] = 0
            order[f, c] = np.lexsort((-idx, -k))
            ncand[f, c] = int((k != 0).sum())
    return order, ncand


def ref_keys_order(scores, thr=None):
    """(order [F,C,B], ncand [F,C]) of the lists the volume's sort keys stand for; the non-candidates behind ncand by
    descending index (see ``canonical_tail``)"""
    return expected(np.asarray(scores, dtype=F32), thr)


def canonical_tail(order, ncand):
    """``argsort_volume`` promises the candidates' order and only the SET of the entries behind them (``the others form the
    tail``): bring the tail into ``ref_keys_order``'s arrangement, descending index.  Without a threshold ncand == B and
    nothing moves."""
    order = np.array(order, dtype=np.int64)
    B = order.shape[-1]
    tail = np.arange(B)[None, None, :] >= np.asarray(ncand)[:, :, None]
    key = np.where(tail, -order, np.iinfo(np.int64).min)           # candidates first, in place (stable sort)
    return np.take_along_axis(order, np.argsort(key, axis=-1, kind='stable'), axis=-1)


# ------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def seam_volume(F, B, C, seed):
    """randn scores [F,B,C] (read-only, shared) with specials placed by FRAME NUMBER only: with S = B*C series per frame,
    frame f has NaN in series 3f mod S, +inf in 3f+1, -inf in 3f+2, -0.0 in 5f+7 -- so wherever a chunk seam or a video
    border falls, each special sits directly on it in some series.  1 % of the entries are exact copies of another entry of
    the same frame and class (tied keys); they are drawn first, so that no copy lands on a special (where two specials
    meet, as they must at S = 8, the non-finite one stays)."""
    rng = np.random.default_rng(seed)
    vol = rng.standard_normal((F, B, C)).astype(F32)
    n = max(1, (F * B * C) // 100)
    f, c = rng.integers(0, F, n), rng.integers(0, C, n)
    src, dst = rng.integers(0, B, n), rng.integers(0, B, n)
    vol[f, dst, c] = vol[f, src, c]
    S = B * C
    flat = vol.reshape(F, S)
    fr = np.arange(F)
    flat[fr, (5 * fr + 7) % S] = -0.0
    flat[fr, (3 * fr) % S] = np.nan
    flat[fr, (3 * fr + 1) % S] = np.inf
    flat[fr, (3 * fr + 2) % S] = -np.inf
    vol.setflags(write=False)
    return vol


BORDER_SETS = ("each", "cycle", "long", "one")
_CYCLE = (1, 2, 1, 3, 5, 1, 9)


def border_table(name, F):
    """frame offsets [V+1] of the videos that make up F concatenated frames
    each:  every frame is its own video
    cycle: lengths 1, 2, 1, 3, 5, 1, 9 and round again (the last one cut at F)
    long:  one long video (40 frames; F - 2 where F < 42) between 1-frame videos
    one:   a single video of F frames (== no table at all)"""
    if name == "each":
        off = list(range(F + 1))
    elif name == "cycle":
        off, i = [0], 0
        while off[-1] < F:
            off.append(min(F, off[-1] + _CYCLE[i % len(_CYCLE)]))
            i += 1
    elif name == "long":
        L = 40 if F >= 42 else F - 2
        lead = (F - L) // 2
        off = list(range(lead + 1)) + list(range(lead + L, F + 1))
    elif name == "one":
        off = [0, F]
    else:
        raise ValueError(name)
    return np.asarray(off, dtype=np.int64)


def taps_for(K):
    """random taps, one of them exactly 0.0 (inf * 0 = NaN must come out as NaN); the outermost taps, which reach across
    a seam first, stay non-zero"""
    t = np.random.default_rng(1000 + 17 * K).standard_normal(K).astype(F32)
    t[1] = 0.0
    return t


BIAS = 0.375
PAD_PAIRS = ((-1e5, 0.0), (0.5, -1.0))       # (pad_max, pad_conv); 0.5 lies above many inputs: a border that forgets the
FUSED_PADS = (0.5, -1.0)                     # pad and a seam that applies it both show


def seed_of(F, B, C):
    return 7000 + 1009 * F + 31 * B + C


# ------------------------------------------------------------------------------------------------
# the cases (F, B, C); standalone kernels see S = B*C series
# ------------------------------------------------------------------------------------------------
# vec4 kernels, >= 3 chunks: S = 8 and S = 1028 (one live thread in a second block of 256 float4 columns)
STANDALONE = [(F, S // 4, 4) for F in (51, 64) for S in (8, 1028)]
POOL_WINDOWS = (3, 5, 7, 9)
CONV_WINDOWS = (3, 5, 7, 9)
BOTH_WINDOWS = (3, 5, 7)
# scalar kernel: windows the vec4 kernels do not have, S % 4 != 0
WIDE = [(51, 257, 4), (64, 2, 4)]
WIDE_POOL_WINDOWS = (11, 33)
WIDE_CONV_WINDOWS = (13,)
ODD_S = [(51, 6, 5)]                          # S = 30
# the window is wider than the video
SHORT = [(F, S // 4, 4) for F in (1, 2, 3) for S in (8, 1028)]
SHORT_WINDOWS = (5, 9)
# fused pass: F = 36 is 4 chunks of 9 (chunks start on the odd frames 9 and 27), F = 27 is 3 chunks of 9; B = 70 and
# B = 45 are no multiples of 4 and leave a ragged last tile; C picks the tiling
FUSED = [(36, 70, 8), (36, 70, 100), (36, 70, 200), (36, 70, 400), (27, 45, 200)]
FUSED_WINDOWS = (3, 5)
FUSED_THR = (None, 0.25)
FUSED_TILINGS = {8: (256, 64), 100: (256, 32), 200: (512, 32), 400: (512, 16)}
# batched fallbacks of volume_pass(frame_off=...): (F, B, C, window, taps given, kernel)
BATCH_FALLBACK = [(51, 64, 6, 3, True, "both"), (51, 64, 6, 7, True, "both"), (51, 64, 8, 9, True, "vec4"),
                  (51, 64, 8, 7, False, "vec4"), (51, 37, 5, 7, True, "scalar")]
# alignment fallback (the slice starts 4 bytes into the allocation: scalar kernels, no keys)
ALIGN = [(36, 70, 8)]
ALIGN_WINDOW = 3

REPICK = ("%s: the host's chunk formula no longer splits this shape into the seams it was chosen for -- re-pick the shapes "
          "in tests/temporal_cases.py")


def chunk_plan(kind, F, B, C, n_cu, max_lds=160 * 1024):
    """(chunks, fchunk, tiling) of a launch over a volume [F,B,C] on a device with n_cu compute units.
    kind 'standalone': temporal_vec4_kernel / temporal_both_vec4_kernel over S = B*C series -- mirrors ``temporal_launch``
    and ``temporal_maxpool_conv_impl`` of csrc/vdet_capi.hip ("few series (tubelet tracks): split the frame axis", the lines
    that set gx, chunks and fchunk); tiling is None, and S % 4 != 0 (scalar kernel: no chunks) gives (1, F, None).
    kind 'fused': volume_pass_kernel -- mirrors ``volume_pass_impl`` (the loop over nt in {256, 512} that picks TB, and the
    lines that set ntiles, chunks and fchunk); tiling = (NT, TB).  A class count the fused kernel does not take gives the
    standalone plan with tiling None (the host falls back to those kernels).
    chunks is the grid's y extent, ceil(F / fchunk)."""
    def split(want):
        want = max(1, min(want, 65535))
        fchunk = (F + want - 1) // want
        return (F + fchunk - 1) // fchunk, fchunk, None

    def standalone():
        S = B * C
        if S % 4:
            return 1, F, None
        gx = (S // 4 + 255) // 256
        return split(min(max(F // 16, 1), (4 * n_cu + gx - 1) // gx) if gx < 4 * n_cu else 1)

    if kind == "standalone":
        return standalone()
    if kind != "fused":
        raise ValueError(kind)
    tiling = None
    if C % 4 == 0:
        C4 = C // 4
        for nt in (256, 512):
            tb = 64
            while tb >= 16 and tb * C4 > nt * 4:
                tb >>= 1
            if tb >= 16 and (nt == 512 or tb >= 32):
                tiling = (nt, tb)
                break
        if tiling and 2 * C4 * tiling[1] * 16 > max_lds // 2:
            tiling = None
    if tiling is None:
        return standalone()
    ntiles = (B + tiling[1] - 1) // tiling[1]
    chunks, fchunk, _ = split(min(max(F // 8, 1), (8 * n_cu + ntiles - 1) // ntiles))
    return chunks, fchunk, tiling


def seams(chunks, fchunk):
    """first frames of the chunks after the first"""
    return [k * fchunk for k in range(1, chunks)]


def reference_cases():
    """every (label, (F, B, C), W, taps or None, pad_max, pad_conv, border name or None) the GPU tests compare against
    ``ref_maxpool`` (always) and ``ref_conv`` (taps given)"""
    out = []
    for shape in STANDALONE + ODD_S:
        for W in sorted(set(POOL_WINDOWS + CONV_WINDOWS)):
            for pm, pc in PAD_PAIRS:
                out.append(("standalone", shape, W, taps_for(W), pm, pc, None))
    for shape in WIDE:
        for W in WIDE_POOL_WINDOWS:
            out.append(("wide", shape, W, None, PAD_PAIRS[1][0], 0.0, None))
        for W in WIDE_CONV_WINDOWS:
            out.append(("wide", shape, W, taps_for(W), PAD_PAIRS[1][0], PAD_PAIRS[1][1], None))
    for shape in SHORT:
        for W in SHORT_WINDOWS:
            for pm, pc in PAD_PAIRS:
                out.append(("short", shape, W, taps_for(W), pm, pc, None))
    for shape in FUSED:
        for W in FUSED_WINDOWS:
            out.append(("fused", shape, W, taps_for(W), FUSED_PADS[0], FUSED_PADS[1], None))
            for name in BORDER_SETS:
                out.append(("batched", shape, W, taps_for(W), FUSED_PADS[0], FUSED_PADS[1], name))
    for F, B, C, W, _, _ in BATCH_FALLBACK:
        for name in BORDER_SETS:
            out.append(("batched-fallback", (F, B, C), W, taps_for(W), FUSED_PADS[0], FUSED_PADS[1], name))
    for shape in ALIGN:
        out.append(("align", shape, ALIGN_WINDOW, taps_for(ALIGN_WINDOW), FUSED_PADS[0], FUSED_PADS[1], None))
    return out


@functools.lru_cache(maxsize=None)
def cached_maxpool(shape, W, pad, border):
    r = ref_maxpool(seam_volume(*shape, seed_of(*shape)), W, pad, None if border is None else border_table(border, shape[0]))
    r.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def cached_conv(shape, W, pad, border):
    r = ref_conv(seam_volume(*shape, seed_of(*shape)), taps_for(W), BIAS, pad,
                 None if border is None else border_table(border, shape[0]))
    r.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def cached_keys_order(shape, thr):
    o, n = ref_keys_order(seam_volume(*shape, seed_of(*shape)), thr)
    o.setflags(write=False)
    n.setflags(write=False)
    return o, n
