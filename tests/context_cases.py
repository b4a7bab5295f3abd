"""The cases of the multi-context suppression tests, shared by test_context_cpu.py (spec sanity) and test_context_gpu.py (device
against spec, on bits).  numpy only (``records_off_context`` alone imports the package, when it is called).

A case is a dict: ``name``, ``scores`` f32 [F,B,C], ``kw`` (the keyword arguments of context_classes: ratio / top / min_hits /
score_thresh / frame_off), and optionally ``expect`` (facts the case was built to show: thresh, k, ...), which the CPU test
checks against the spec so that the GPU test compares against a spec that is known to stand where the case aims.

CHUNK restates the host's decomposition ONCE (csrc/context_kernels.hpp: kCtxChunk): a video's scores are read as one run of
floats in chunks of CHUNK elements, a workgroup per chunk.  ``seams_ok`` asserts that the seam cases still put their planted
values on chunk and video borders; it guards the cases, not the kernels.
"""
import functools

import numpy as np

CHUNK = 32768                    # csrc/context_kernels.hpp: kCtxChunk
REC_MIN, REC_MAX = 4096, 1 << 21   # ... kCtxRecMin, kCtxRecMax: records per video = clamp(elements / 64, REC_MIN, REC_MAX)
DIGIT_BITS = (21, 10)            # the radix's digit boundaries (digits of 11 | 11 | 10 bits)

REPICK = "%s: the chunk size no longer puts this case's planted values on the seams it was chosen for -- re-pick it in tests/context_cases.py"

F32 = np.float32
DEN = np.frombuffer(np.uint32(1).tobytes(), F32)[0]          # smallest denormal
FMAX = np.finfo(F32).max


def chunks(ne):
    return (ne + CHUNK - 1) // CHUNK


def record_cap(ne):
    return min(REC_MAX, max(REC_MIN, ne // 64))


def bits(u):
    return np.frombuffer(np.uint32(u).tobytes(), F32)[0]


def down(x):
    return np.nextafter(F32(x), F32(-np.inf))


def up(x):
    with np.errstate(over='ignore'):         # (the float above the largest finite one is +inf)
        return np.nextafter(F32(x), F32(np.inf))


def _rand(seed, shape, nan_frac=0.02):
    r = np.random.RandomState(seed)
    s = r.randn(*shape).astype(F32)
    if nan_frac:
        s[r.rand(*shape) < nan_frac] = np.nan
    return s


def _knife(name, t, shape=(2, 3, 4), seed=0, extra=()):
    """The k-th value is t and the (k+1)-th is nextafter(t, -inf) (where one exists); the cells left over are NaN."""
    t = F32(t)
    above = [] if t == np.inf else [up(t), up(up(t))] + ([F32(np.inf)] if up(up(t)) < np.inf else [])
    below = [] if t == -np.inf else [down(t), down(down(t))]
    vals = above + [t] + list(extra) + below
    k = len(above) + 1
    n = int(np.prod(shape))
    flat = np.full(n, np.nan, F32)
    pos = np.random.RandomState(seed).permutation(n)[:len(vals)]
    flat[pos] = np.array(vals, F32)
    tt = F32(0.0) if t == 0 else t
    return dict(name=name, scores=flat.reshape(shape), kw=dict(top=k), expect=dict(thresh=tt, k=k, n=len(vals)))


def _plant(scores, frame_off, video, k, t, p_k, p_next):
    """Into video `video`: k - 1 values above t anywhere else, t at element p_k, nextafter(t, -inf) at p_next (element
    indices inside the video; p_next may lie in the NEXT video, where it must not count)."""
    F, B, C = scores.shape
    a, b = frame_off[video] * B * C, frame_off[video + 1] * B * C
    flat = scores.reshape(-1)
    flat[a + p_k] = t
    flat[a + p_next] = down(t)
    r = np.random.RandomState(k)
    free = np.setdiff1d(np.arange(b - a), [p_k, p_next])
    flat[a + r.choice(free, k - 1, replace=False)] = t + F32(1.0) + r.rand(k - 1).astype(F32)


def _seam_cases():
    out = []
    # one video of four chunks; background in [0, 1), planted values around 3
    shape = (2, 257, 200)
    ne = int(np.prod(shape))
    for name, p_k, p_next in (("seam_last_first", CHUNK - 1, CHUNK), ("seam_first_last", CHUNK, 2 * CHUNK - 1),
                              ("seam_video_ends", ne - 1, 0), ("seam_tail_chunk", 3 * CHUNK, 3 * CHUNK - 1)):
        s = np.random.RandomState(7).rand(*shape).astype(F32)
        _plant(s, [0, shape[0]], 0, 5, F32(3.0), p_k, p_next)
        out.append(dict(name=name, scores=s, kw=dict(top=5), expect=dict(thresh=F32(3.0), k=5),
                        seams=dict(ne=[ne], planted=[(0, p_k), (0, p_next)])))
    # two videos of three and four chunks: the k-th value on a video's last element, the next lower one across the border
    shape, off = (7, 129, 200), [0, 3, 7]
    nes = [(off[i + 1] - off[i]) * shape[1] * shape[2] for i in range(2)]
    s = np.random.RandomState(8).rand(*shape).astype(F32)
    _plant(s, off, 0, 4, F32(3.0), nes[0] - 1, nes[0])            # down(3.0) is video 1's first element
    _plant(s, off, 1, 4, F32(2.0), 1, nes[1] - 1)                # (video 1's element 0 holds down(3.0): its fourth value, above 2)
    assert s.reshape(-1)[nes[0]] == down(F32(3.0))
    out.append(dict(name="seam_video_border", scores=s, kw=dict(top=4, frame_off=off),
                    expect=dict(thresh=[F32(3.0), down(F32(3.0))]),
                    seams=dict(ne=nes, planted=[(0, nes[0] - 1), (1, 0), (1, nes[1] - 1)])))
    return out


def seams_ok(case):
    """The facts a seam case was picked for, from the restated chunk formula."""
    se = case["seams"]
    assert all(chunks(ne) >= 3 for ne in se["ne"]), REPICK % case["name"]
    for v, p in se["planted"]:
        ne = se["ne"][v]
        assert p % CHUNK in (0, CHUNK - 1) or p == ne - 1, REPICK % case["name"]
    return True


def _videos_differ():
    """V = 3, frame_off [0,1,6,8]: each video has its own pair of strong classes; video 2 also holds a class of NaN."""
    F, B, C = 8, 33, 30
    off = [0, 1, 6, 8]
    s = _rand(21, (F, B, C))
    for v, cls in enumerate(((2, 5), (7, 11), (29, 0))):
        for c in cls:
            s[off[v]:off[v + 1], ::4, c] += F32(6.0)
    s[off[2]:, :, 13] = np.nan
    return dict(name="batch_v3_high_sets_differ", scores=s, kw=dict(ratio=0.02, frame_off=off))


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    # ---- shapes (odd sizes, C below / at / beyond a 16-byte multiple), by ratio and by top
    for i, shape in enumerate(((1, 1, 1), (2, 3, 4), (3, 7, 3), (5, 33, 30), (4, 129, 200), (2, 65, 201))):
        out.append(dict(name="shape_%dx%dx%d_ratio" % shape, scores=_rand(i, shape), kw=dict(ratio=0.01)))
        out.append(dict(name="shape_%dx%dx%d_top" % shape, scores=_rand(10 + i, shape), kw=dict(top=7)))
    out[0]["scores"] = np.array([[[0.25]]], F32)         # (the 1x1x1 volumes hold a number, not a NaN)
    out[1]["scores"] = np.array([[[-1.5]]], F32)
    out += _seam_cases()
    # ---- knife edges of the select
    out.append(_knife("knife_pos_denormal", DEN))
    out.append(_knife("knife_neg_denormal", -DEN))
    out.append(_knife("knife_zero_with_neg_zero", 0.0, extra=[F32(-0.0), F32(0.0), F32(-0.0)]))
    out[-1]["expect"]["hits_total"] = out[-1]["expect"]["k"] + 3
    out.append(_knife("knife_one", 1.0))
    out.append(_knife("knife_minus_one", -1.0))
    out.append(_knife("knife_largest_finite", FMAX))
    out.append(_knife("knife_pos_inf", np.inf, extra=[F32(np.inf)]))
    out.append(_knife("knife_neg_inf", -np.inf, extra=[F32(-np.inf)]))
    out[-1]["kw"] = dict(top=out[-1]["expect"]["n"])     # k = n: the rank reaches down to -inf
    out[-1]["expect"]["k"] = out[-1]["expect"]["n"]
    for b in DIGIT_BITS:
        # positive floats: key = bits | sign, so bits with the low b bits zero / the float below with them all ones
        out.append(_knife("knife_digit%d_pos" % b, bits(0x3FA00000 if b == 21 else 0x3F800400)))
        # negative floats: key = ~bits
        out.append(_knife("knife_digit%d_neg" % b, bits(0xBF9FFFFF if b == 21 else 0xBF8003FF)))
    out.append(_knife("knife_negative_range", -3.75, shape=(3, 7, 3)))
    # ---- ranks
    s = _rand(30, (3, 7, 3), nan_frac=0.1)
    n = int((~np.isnan(s)).sum())
    out.append(dict(name="rank_k1", scores=s, kw=dict(top=1), expect=dict(k=1)))
    out.append(dict(name="rank_kn", scores=s, kw=dict(top=n), expect=dict(k=n)))
    out.append(dict(name="rank_top_beyond_n", scores=s, kw=dict(top=10 * n), expect=dict(k=n)))
    out.append(dict(name="rank_ratio_one", scores=s, kw=dict(ratio=1.0), expect=dict(k=n)))
    out.append(dict(name="ratio_n10000", scores=_rand(31, (1, 50, 200), 0), kw=dict(ratio=0.0003), expect=dict(k=2, n=10000)))
    out.append(dict(name="ratio_n30000", scores=_rand(32, (3, 50, 200), 0), kw=dict(ratio=0.0003), expect=dict(k=9, n=30000)))
    out.append(dict(name="min_hits_2", scores=_rand(33, (5, 33, 30)), kw=dict(top=40, min_hits=2)))
    # ---- ties and specials
    out.append(dict(name="all_equal_small", scores=np.full((2, 3, 4), 0.5, F32), kw=dict(top=3), expect=dict(thresh=F32(0.5))))
    # more equal scores than the video has record slots: the natural fallback to the full-read passes
    shape = (3, 50, 30)
    assert int(np.prod(shape)) > record_cap(int(np.prod(shape)))
    out.append(dict(name="all_equal_beyond_records", scores=np.full(shape, -2.25, F32), kw=dict(ratio=0.0003),
                    expect=dict(thresh=F32(-2.25))))
    shape = (2, 400, 200)        # five chunks, the tie only in the top bin's share
    s = _rand(34, shape, 0)
    s[s > 0.5] = F32(0.75)
    assert int((s == 0.75).sum()) > record_cap(s.size)
    out.append(dict(name="tied_top_beyond_records", scores=s, kw=dict(ratio=0.0003), expect=dict(thresh=F32(0.75))))
    # every score in the top bin of the first digit, [0.875, 1): too many for the records there, few below the second digit
    s = (F32(0.9) + F32(0.09) * np.random.RandomState(40).rand(*shape)).astype(F32)
    assert s.min() >= 0.875 and s.max() < 1 and s.size > record_cap(s.size)
    out.append(dict(name="late_records_uniform", scores=s, kw=dict(ratio=0.0003)))
    # records that fit the video's slice but not a workgroup's LDS share of it (csrc/context_kernels.hpp: kCtxLdsRec = 1024 a chunk)
    s = (F32(0.4) * np.random.RandomState(41).rand(*shape)).astype(F32)
    pos = CHUNK + np.random.RandomState(42).choice(CHUNK, 3000, replace=False)            # all of them in the second chunk
    s.reshape(-1)[pos] = (F32(1.0) + F32(0.24) * np.random.RandomState(43).rand(3000)).astype(F32)
    assert 2 * 1024 < 3000 <= record_cap(s.size)
    out.append(dict(name="dense_records", scores=s, kw=dict(ratio=0.0003)))
    s = _rand(35, (5, 33, 30))
    s[:, :, 4] = np.nan
    out.append(dict(name="class_all_nan", scores=s, kw=dict(ratio=0.01)))
    s = _rand(36, (8, 33, 30))
    s[1:6] = np.nan
    out.append(dict(name="video_all_nan", scores=s, kw=dict(ratio=0.01, frame_off=[0, 1, 6, 8])))
    out.append(dict(name="all_nan", scores=np.full((2, 3, 4), np.nan, F32), kw=dict(top=2), expect=dict(n=0)))
    s = _rand(37, (5, 33, 30))
    out.append(dict(name="score_thresh", scores=s, kw=dict(ratio=0.01, score_thresh=0.5)))
    out.append(dict(name="score_thresh_above_all", scores=s, kw=dict(ratio=0.01, score_thresh=1e6), expect=dict(n=0)))
    s = _rand(38, (5, 33, 30))
    s[:, 20:, :] = -np.inf       # io.py's padding
    out.append(dict(name="score_thresh_neg_inf", scores=s, kw=dict(ratio=0.01, score_thresh=-np.inf)))
    out.append(dict(name="neg_inf_is_candidate", scores=s, kw=dict(ratio=1.0), expect=dict(thresh=F32(-np.inf))))
    # ---- batches
    out.append(_videos_differ())
    out.append(dict(name="batch_v3_top", scores=_rand(39, (8, 33, 30)), kw=dict(top=25, frame_off=[0, 1, 6, 8])))
    names = [c["name"] for c in out]
    assert len(set(names)) == len(names)
    return tuple(out)


def case(name):
    return next(c for c in cases() if c["name"] == name)


def records_off_context(device=-1):
    """A fresh context created under VDET_CTX_RECORDS=0 (the switch is read at vdet_create): the four-read form on every video.
    The one copy of this set-and-restore, for the GPU tests and devtools/bench_context.py; the caller closes the context."""
    import os
    from vdetlib_amd import _lib
    old = os.environ.get("VDET_CTX_RECORDS")
    os.environ["VDET_CTX_RECORDS"] = "0"
    try:
        return _lib.Context(device)
    finally:
        if old is None:
            del os.environ["VDET_CTX_RECORDS"]
        else:
            os.environ["VDET_CTX_RECORDS"] = old
