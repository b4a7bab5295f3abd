"""The cases of the Seq-NMS tests (tests/test_seqnms_cpu.py, tests/test_seqnms_gpu.py): builders and THE list, no GPU and no
product code.  A case is a dict: name, tracks [C,R,F,5] f32, ntracks [C] int32, score (None: column 4, or [C,R,F] f32 / f64)
kw, the keyword arguments of seqnms_spec.seq_nms / ops.seq_nms, and seam: None, ('lds', path) or ('launches', n).

The seams of the device code, restated here from csrc/seqnms_kernels.hpp so that a case which is meant to sit on one still
does (test_seqnms_gpu.py asserts both against the device):
  lds_frames(R)      the longest video whose predecessor table ((F*Rp + F) int16, Rp = R rounded up to 64) fits the 128 KiB LDS
                     budget; one frame more and the table lies in global scratch (vdet_query 14: 1 / 2)
  launch_plan(F, S)  (rounds per launch, launches): max(1, 16384 // F) rounds, and S + 1 iterations to spend
"""
import functools

import numpy as np

import seqnms_spec as spec
import synth

F32, F64 = np.float32, np.float64
LDS_BUDGET, FRAME_STEPS = 128 * 1024, 16384
R_EDGES = (1, 31, 32, 33, 63, 64, 65, 128, 255, 256)      # the word (32) and wave (64) edges of a link row


def lds_frames(R):
    rp = (R + 63) // 64 * 64
    return (LDS_BUDGET // 2) // (rp + 1)


def launch_plan(F, S):
    rounds = max(1, FRAME_STEPS // F)
    return rounds, (S + 1 + rounds - 1) // rounds


def video(seed, C, R, F, jitter=6, shuffle=True):
    """tracks [C,R,F,5] of proposals that persist over the frames (synth.coherent_video), every class with its own scores and
    -- shuffle -- its own order of the rows in every frame, so that a sequence changes slot from frame to frame."""
    boxes, scores = synth.coherent_video(seed, F, R, C, jitter=jitter)            # [F,R,4], [F,R,C]
    rng = np.random.RandomState(seed + 77)
    t = np.empty((C, R, F, 5), F32)
    for c in range(C):
        for f in range(F):
            p = rng.permutation(R) if shuffle else np.arange(R)
            t[c, :, f, :4] = boxes[f, p]
            t[c, :, f, 4] = scores[f, p, c]
    return t


def sprinkle(tracks, seed, frac=0.15, score=None):
    """No-node rows on every frame: NaN boxes, NaN / +inf / -inf scores (in the score tensor when there is one)."""
    rng = np.random.RandomState(seed)
    t = tracks.copy()
    s = None if score is None else score.copy()
    C, R, F = t.shape[:3]
    kind = rng.randint(0, 4, (C, R, F))
    pick = rng.rand(C, R, F) < frac
    pick[:, 0, :] = True                       # every frame has one ...
    kind[:, 0, :] = np.arange(F)[None, :] % 4   # ... and every kind is on some frame
    t[pick & (kind == 0), 0] = np.nan
    tgt = t[..., 4] if s is None else s
    for k, val in ((1, np.nan), (2, np.inf), (3, -np.inf)):
        tgt[pick & (kind == k)] = val
    return t, s


def _case(name, tracks, ntracks=None, score=None, seam=None, **kw):
    C, R = tracks.shape[:2]
    nt = np.full(C, R, np.int32) if ntracks is None else np.asarray(ntracks, np.int32)
    assert nt.shape == (C,)
    return dict(name=name, tracks=np.ascontiguousarray(tracks, F32), ntracks=nt, score=score, seam=seam, kw=kw)


def expect(case, **over):
    """The spec's result of a case (keyword arguments overridden by ``over``)."""
    return spec.seq_nms_classes(case['tracks'], case['ntracks'], case['score'], **dict(case['kw'], **over))


def count_to_exhaustion(tracks, **kw):
    out = spec.seq_nms_classes(tracks, np.full(len(tracks), tracks.shape[1], np.int32), None, **dict(kw, max_seqs=4096))
    assert out['exhausted'].all()
    return int(out['nseq'].max()), out


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    # ---- R: the word and wave edges, ntracks 0 / 1 / R-1 / R / above R
    for R in R_EDGES:
        t = video(100 + R, 3, R, 6)
        out.append(_case('R%d_few' % R, t, (0, 1, max(R - 1, 0)), max_seqs=8))
        out.append(_case('R%d_all' % R, t, (R, R + 9, R), max_seqs=8, rescore='max' if R % 2 else 'avg'))
    # ---- F: no links, one pair, two; the LDS seam of R = 64 and the launches of a long video in global scratch
    for F in (1, 2, 3):
        out.append(_case('F%d' % F, video(200 + F, 2, 33, F), max_seqs=40))
    Fl = lds_frames(64)
    out.append(_case('F%d_lds_last' % Fl, video(210, 1, 64, Fl, shuffle=False), max_seqs=3, seam=('lds', 1)))
    out.append(_case('F%d_global_first' % (Fl + 1), video(211, 1, 64, Fl + 1, shuffle=False), max_seqs=3, seam=('lds', 2)))
    out.append(_case('F%d_global_two_launches' % (Fl + 1), video(212, 1, 40, Fl + 1, shuffle=False), max_seqs=launch_plan(Fl + 1, 1)[0],
                     rescore='max', seam=('launches', 2)))
    # ---- launches: 512 nodes that link to nothing and suppress nothing are 512 sequences; 256 rounds per launch at F = 64
    t = video(220, 1, 8, 64)
    assert launch_plan(64, 511) == (256, 2) and launch_plan(64, 512) == (256, 3)
    out.append(_case('launches_2_one_short', t, link_thres=2.0, nms_thres=2.0, max_seqs=511, seam=('launches', 2)))
    out.append(_case('launches_3_exact', t, link_thres=2.0, nms_thres=2.0, max_seqs=512, seam=('launches', 3)))
    # ---- scores
    t = video(300, 3, 40, 7)
    out.append(_case('tie_free', t, max_seqs=64))
    e = t.copy()
    e[..., 4] = 0.5
    out.append(_case('all_equal', e, max_seqs=64))
    out.append(_case('all_equal_max', e, max_seqs=64, rescore='max'))
    n = t.copy()
    n[..., 4] = -0.01 - n[..., 4]
    out.append(_case('all_negative', n, max_seqs=4096))
    m = t.copy()
    m[..., 4] = np.round(m[..., 4] * 8 - 4) / 4                         # -1 .. 1 in quarters, exact zeros among them
    assert (m[..., 4] == 0).any() and (m[..., 4] < 0).any()
    out.append(_case('mixed_sign_zeros', m, max_seqs=4096))
    out.append(_case('mixed_sign_zeros_max', m, max_seqs=64, rescore='max'))
    rng = np.random.RandomState(301)
    s64 = rng.rand(3, 40, 7) - 0.3
    out.append(_case('score_f64', t, score=s64, max_seqs=64))
    out.append(_case('score_f32', t, score=s64.astype(F32), max_seqs=64, rescore='max'))
    out.append(_case('no_nodes_col4', *sprinkle(t, 302), max_seqs=64))
    sp = sprinkle(t, 303, score=s64)
    out.append(_case('no_nodes_f64', sp[0], score=sp[1], max_seqs=64))
    sp = sprinkle(t, 304, score=s64.astype(F32))
    out.append(_case('no_nodes_f32', sp[0], score=sp[1], max_seqs=4096))
    h = t.copy()
    h[:, :, 3, 0] = np.nan
    out.append(_case('empty_middle_frame', h, max_seqs=64))
    out.append(_case('empty_class', t, (40, 0, 40), max_seqs=64))
    z = t.copy()
    z[1] = np.nan
    out.append(_case('nan_class', z, max_seqs=64))
    # ---- cut-offs, on a video small enough to run to exhaustion
    t = video(400, 2, 12, 5, jitter=10)
    nx, full = count_to_exhaustion(t)
    for S in sorted({1, nx - 1, nx, nx + 1}):
        out.append(_case('max_seqs_%d_of_%d' % (S, nx), t, max_seqs=S))
    sums = full['seq_sum'][0]
    assert sums[1] > sums[2]
    out.append(_case('min_score_before_first', t, max_seqs=64, min_score=np.inf))
    out.append(_case('min_score_between', t, max_seqs=64, min_score=float((sums[1] + sums[2]) / 2)))
    out.append(_case('min_score_exact', t, max_seqs=64, min_score=float(sums[2])))
    out.append(_case('min_score_never', t, max_seqs=64, min_score=-np.inf))
    for name, kw in (('nms0', dict(nms_thres=0.0)), ('nms2', dict(nms_thres=2.0)), ('link0', dict(link_thres=0.0)),
                     ('link2', dict(link_thres=2.0))):
        for rescore in spec.RESCORE:
            out.append(_case('%s_%s' % (name, rescore), video(410, 2, 20, 6), max_seqs=4096, rescore=rescore, **kw))
    names = [c['name'] for c in out]
    assert len(set(names)) == len(names)
    return out


def case(name):
    return next(c for c in cases() if c['name'] == name)


def border_batch():
    """5 videos of 1, 2, 7, 3, 12 frames whose border frames hold IDENTICAL boxes: the last frame of a video is the first of
    the next, so a link across a border would be taken if anything allowed it.  Returns (list of tracks [C,R,F_v,5], ntracks
    [V,C], frame_off)."""
    lens = (1, 2, 7, 3, 12)
    C, R = 2, 9
    vids = []
    for v, n in enumerate(lens):
        t = video(500 + v, C, R, n, shuffle=False)
        if vids:
            t[:, :, 0] = vids[-1][:, :, -1]
        vids.append(t)
    nt = np.full((len(lens), C), R, np.int32)
    nt[2, 1] = R - 2
    return vids, nt, np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
