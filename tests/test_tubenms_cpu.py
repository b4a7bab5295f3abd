"""No GPU: the rule of ops.nms_tubelets (tests/tubenms_spec.py) against an independent brute-force restatement and hand-worked
cases, the planted set, the argument checks that run before any launch, and the header's limits rows."""
import inspect
import math
import os
import re

import numpy as np
import pytest

import tubenms_cases as cases
import tubenms_spec as spec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def brute(tracks, ntracks, score, tboxes=None, thresh=0.5, norm='union', reduce='mean', min_shared=1):
    """The rule once more, scalar by scalar: a Python loop over pairs and frames, numpy only for the f32 scalars.
    Returns (kept slots per class, by [C,T], overlaps [C,T,T], ts [C,T])."""
    C, T, F = tracks.shape[:3]
    one, zero = F32(1), F32(0)
    mx = lambda a, b: a if a >= b else b
    mn = lambda a, b: a if a <= b else b
    keeps, bys, ovs, tss = [], np.full((C, T), -1, np.int32), np.full((C, T, T), np.nan), np.full((C, T), np.nan)
    for c in range(C):
        nt = min(max(int(ntracks[c]), 0), T)
        ex = [[t < nt and not math.isnan(float(tracks[c, t, f, 0])) for f in range(F)] for t in range(T)]
        box = [[(tracks[c, t, f, :4] if tboxes is None else tboxes[c, t, f]) for f in range(F)] for t in range(T)]
        ts = [float('nan')] * T
        for t in range(T):
            if not any(ex[t]):
                continue
            if np.ndim(score) == 2:
                ts[t] = float(score[c, t])
                continue
            vals = [float(score[c, t, f]) for f in range(F) if ex[t][f] and not math.isnan(float(score[c, t, f]))]
            if vals and reduce == 'mean':
                s = 0.0
                for x in vals:
                    s += x
                ts[t] = s / len(vals)
            elif vals:
                m = max(vals)
                ts[t] = (0.0 if any(math.copysign(1.0, x) > 0 for x in vals if x == 0.0) else -0.0) if m == 0.0 else m
        tss[c] = ts
        present = [not math.isnan(x) for x in ts]
        ovr = np.zeros((T, T))
        for a in range(T):
            for b in range(a, T):
                S, I = 0, 0
                for f in range(F):
                    if not (ex[a][f] and ex[b][f]):
                        continue
                    I += 1
                    p, q = box[a][f], box[b][f]
                    with np.errstate(all='ignore'):
                        pa = ((p[2] - p[0]) + one) * ((p[3] - p[1]) + one)
                        qa = ((q[2] - q[0]) + one) * ((q[3] - q[1]) + one)
                        w = mx(zero, (mn(p[2], q[2]) - mx(p[0], q[0])) + one)
                        h = mx(zero, (mn(p[3], q[3]) - mx(p[1], q[1])) + one)
                        inter = F32(w * h)
                        quo = F32(inter / F32(F32(pa + qa) - inter))
                        if quo > 0 and quo <= np.finfo(F32).max:
                            k = float(np.rint(F32(quo * F32(2.0 ** 24))))
                            S += 2 ** 32 - 1 if k >= 2.0 ** 32 else int(k)
                na, nb = sum(ex[a]), sum(ex[b])
                den = {'union': na + nb - I, 'shared': I, 'min': min(na, nb)}[norm]
                o = 0.0 if den == 0 or I < min_shared else float(S) / (float(den) * 16777216.0)
                ovr[a, b] = ovr[b, a] = o
        for a in range(T):
            for b in range(T):
                if present[a] and present[b]:
                    ovs[c, a, b] = ovr[a, b]
        order = sorted((t for t in range(T) if present[t]), key=lambda t: (-(ts[t] + 0.0), -t))
        kept = []
        for t in order:
            if bys[c, t] >= 0:
                continue
            bys[c, t] = t
            kept.append(t)
            for u in order:
                if bys[c, u] < 0 and ovr[t, u] >= thresh:
                    bys[c, u] = t
        keeps.append(kept)
    return keeps, bys, ovs, tss


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view({4: np.uint32, 8: np.uint64}[x.dtype.itemsize]) if x.dtype.kind == 'f' else x


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


@pytest.mark.parametrize("norm", spec.NORMS)
@pytest.mark.parametrize("kind", ["mean", "max", "slot"])
@pytest.mark.parametrize("T,F", [(9, 5), (33, 3)])
def test_spec_equals_brute_force(T, F, kind, norm):
    s = cases.random_set(100 + T, 4, T, F, nser=1, tboxes=(kind != 'max'))
    score = s['score2'] if kind == 'slot' else s['score3']
    reduce = 'max' if kind == 'max' else 'mean'
    for thresh, ms in ((0.4, 1), (0.1, 2)):
        want = spec.expected(s['tracks'], s['ntracks'], score, s['tboxes'], s['anchors'], s['series'], thresh, norm, reduce, ms)
        keeps, by, ov, ts = brute(s['tracks'], s['ntracks'], score, s['tboxes'], thresh, norm, reduce, ms)
        assert same(want['overlaps'], ov) and np.array_equal(want['by'], by)
        for c, kept in enumerate(keeps):
            assert want['ntracks'][c] == len(kept) and want['src'][c, :len(kept)].tolist() == kept
            assert (want['src'][c, len(kept):] == spec.SRC_PAD).all()
            assert same(want['tscore'][c, :len(kept)], ts[c, kept]) and np.isnan(want['tscore'][c, len(kept):]).all()
            assert same(want['tracks'][c, :len(kept)], s['tracks'][c, kept]) and np.isnan(want['tracks'][c, len(kept):]).all()
            assert same(want['series'][0][c, :len(kept)], s['series'][0][c, kept])
            assert same(want['anchors'][c, :len(kept)], s['anchors'][c, kept]) and not want['anchors'][c, len(kept):].any()
        assert (want['ntracks'] < np.clip(s['ntracks'], 0, T)).any()        # something was suppressed ...
        assert (want['ntracks'][np.clip(s['ntracks'], 0, T) > 0] > 0).all()  # ... and not everything


def test_exotic_boxes_and_score_edges_equal_brute_force():
    for tracks, ntracks, score in (cases.exotic_set(), cases.score_edge_set()):
        for thresh in (0.3, 2.0):
            want = spec.expected(tracks, ntracks, score, thresh=thresh)
            keeps, by, ov, _ = brute(tracks, ntracks, score, thresh=thresh)
            assert same(want['overlaps'], ov) and np.array_equal(want['by'], by) and want['src'][0, :len(keeps[0])].tolist() == keeps[0]
    tracks, ntracks, score = cases.exotic_set()
    ov = spec.expected(tracks, ntracks, score)['overlaps'][0]
    assert ov[0, 1] == 1.0 and ov[0, 0] == 1.0
    for t in (2, 3, 4, 6, 7, 11):                                          # no contribution, the diagonal included; no error
        assert (ov[t] == 0.0).all(), t
    assert 0.9 < ov[0, 10] < 1.0 and 0.9 < ov[8, 9] < 1.0 and ov[0, 8] == 0.0


def test_two_identical_tubelets():
    tracks, ntracks = cases.blank(1, 2, 5)
    cases.put(tracks, 0, 0, range(5), [3, 4, 30, 40])
    cases.put(tracks, 0, 1, range(5), [3, 4, 30, 40])
    for norm in spec.NORMS:
        out = spec.expected(tracks, ntracks, np.array([[1.0, 2.0]]), thresh=1.0, norm=norm)
        assert (out['overlaps'][0] == 1.0).all()
        assert out['ntracks'][0] == 1 and out['src'][0].tolist() == [1, spec.SRC_PAD] and out['by'][0].tolist() == [1, 1]
        assert out['tscore'][0, 0] == 2.0 and np.isnan(out['tscore'][0, 1])
    out = spec.expected(tracks, ntracks, np.array([[1.0, 2.0]]), thresh=np.nextafter(1.0, 2.0))
    assert out['ntracks'][0] == 2 and out['src'][0].tolist() == [1, 0]


def test_knife_edge_half():
    tracks, ntracks, score = cases.knife_pair()
    S, I, n = spec.pair_sums(tracks[0, :, :, :4], spec.exists(tracks, ntracks)[0])
    assert S[0, 1] == 2 ** 24 and I[0, 1] == 1 and n.tolist() == [2, 1]
    out = spec.expected(tracks, ntracks, score, thresh=0.5)
    assert out['overlaps'][0, 0, 1] == 0.5 and out['ntracks'][0] == 1 and out['by'][0].tolist() == [0, 0]
    out = spec.expected(tracks, ntracks, score, thresh=np.nextafter(0.5, 1.0))
    assert out['ntracks'][0] == 2 and out['by'][0].tolist() == [0, 1]
    assert spec.expected(tracks, ntracks, score, norm='shared')['overlaps'][0, 0, 1] == 1.0


def test_min_swallows_a_contained_short_tubelet():
    tracks, ntracks, score = cases.contained_pair(F=8, short=2)
    u = spec.expected(tracks, ntracks, score, thresh=0.5, norm='union')
    m = spec.expected(tracks, ntracks, score, thresh=0.5, norm='min')
    assert u['overlaps'][0, 0, 1] == 0.25 and u['ntracks'][0] == 2
    assert m['overlaps'][0, 0, 1] == 1.0 and m['ntracks'][0] == 1 and m['by'][0].tolist() == [0, 0]


def test_min_shared():
    tracks, ntracks, score = cases.contained_pair(F=8, short=2)
    for ms, n in ((1, 1), (2, 1), (3, 2)):
        out = spec.expected(tracks, ntracks, score, thresh=0.5, norm='shared', min_shared=ms)
        assert out['ntracks'][0] == n and out['overlaps'][0, 0, 1] == (1.0 if ms <= 2 else 0.0)
    assert spec.expected(tracks, ntracks, score, norm='shared', min_shared=9)['overlaps'][0, 0, 0] == 0.0   # the diagonal: no special case


def test_thresh_above_one_is_the_sort():
    tracks, ntracks, score = cases.score_edge_set()
    out = spec.expected(tracks, ntracks, score, thresh=1.5)
    # inf, the three 1.5 by descending slot, the four zeros (-0.0 == +0.0) by descending slot, -inf; the NaN score is absent
    assert out['src'][0].tolist() == [6, 9, 4, 3, 8, 7, 1, 0, 5, spec.SRC_PAD] and out['ntracks'][0] == 9
    assert out['by'][0].tolist() == [0, 1, -1, 3, 4, 5, 6, 7, 8, 9]
    assert same(out['tscore'][0, :9], score[0, [6, 9, 4, 3, 8, 7, 1, 0, 5]])            # bit for bit: the zeros keep their signs
    s = cases.random_set(5, 3, 12, 6)
    out = spec.expected(s['tracks'], s['ntracks'], s['score3'], thresh=1.0000001)
    ts = spec.tubelet_scores(s['tracks'], s['ntracks'], s['score3'])
    for c in range(3):
        assert out['src'][c, :out['ntracks'][c]].tolist() == spec.order_of(ts[c]) and out['ntracks'][c] == (~np.isnan(ts[c])).sum()


def test_planted_objects_are_kept_once():
    """jitter +/-2 px on boxes of 60..120 px: copies of one object share at least their middle half and overlap by more than
    (56/64)^2 * 1/2 there under 'union' at the worst -- measured here, on the CPU, well above the threshold of 0.3."""
    tracks, ntracks, score, owner = cases.planted_set()
    K, clutter = owner.max() + 1, int((owner < 0).sum())
    out = spec.expected(tracks, ntracks, score, thresh=0.3)
    ov = out['overlaps'][0]
    same_obj = (owner[:, None] == owner[None, :]) & (owner[:, None] >= 0)
    assert ov[same_obj].min() > 0.3 and ov[~same_obj & ~np.eye(len(owner), dtype=bool)].max() == 0.0
    assert out['ntracks'][0] == K + clutter
    kept = out['src'][0, :K + clutter]
    assert sorted(owner[kept[:K]].tolist()) == list(range(K)) and (owner[kept[K:]] < 0).all()
    for t in range(len(owner)):                                            # every copy points at its object's best-scored copy
        if owner[t] >= 0:
            best = max((u for u in range(len(owner)) if owner[u] == owner[t]), key=lambda u: score[0, u])
            assert out['by'][0, t] == best


def test_argument_checks_before_any_launch():
    """every one of these fails on the host: none needs a GPU"""
    import torch
    from vdetlib_amd import ops
    C, T, F = 2, 3, 4
    tr = torch.zeros((C, T, F, 5))
    nt = torch.full((C,), T, dtype=torch.int32)
    sc = torch.zeros((C, T))
    ok = dict(tracks=tr, ntracks=nt, score=sc)
    bad = [
        dict(thresh=float('nan')), dict(min_shared=0), dict(min_shared=1.5), dict(norm='iou'), dict(reduce='sum'),
        dict(score=torch.zeros((C, T, F + 1))), dict(score=torch.zeros((C,))), dict(score=torch.zeros((C, T), dtype=torch.float16)),
        dict(score=None), dict(tracks=torch.zeros((C, T, F, 4))), dict(ntracks=torch.zeros((C,), dtype=torch.int64)),
        dict(tboxes=torch.zeros((C, T, F, 5))), dict(anchors=torch.zeros((C, T, 2))), dict(series=torch.zeros((C, T, F))),
        dict(series=tuple(torch.zeros((C, T, F), dtype=torch.float64) for _ in range(5))),
        dict(tracks=torch.zeros((C, 257, F, 5)), score=torch.zeros((C, 257))),
        dict(tracks=torch.zeros((C, 0, F, 5)), score=torch.zeros((C, 0))),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            ops.nms_tubelets(**dict(ok, **kw))
    with pytest.raises(ValueError, match="no CPU path|same GPU"):          # everything checked: only the device is wrong
        ops.nms_tubelets(**ok)
    with pytest.raises(ValueError, match="256"):
        ops.nms_tubelets(**dict(ok, tracks=torch.zeros((C, 257, F, 5)), score=torch.zeros((C, 257))))
    with pytest.raises(ValueError, match="series"):
        ops.nms_tubelets(dict(tracks=tr, ntracks=nt, series=()), score=1)
    with pytest.raises(ValueError, match="takes the place"):
        ops.nms_tubelets(dict(tracks=tr, ntracks=nt, series=(sc,)), ntracks=nt)
    big = torch.zeros((1,), dtype=torch.float32).as_strided((1 << 16, 256, 128, 5), (0, 0, 0, 0))      # C*T*F = 2^31: no memory behind it
    with pytest.raises(ValueError, match="2\\^31 - 16"):
        ops.nms_tubelets(big, torch.zeros((1 << 16,), dtype=torch.int32), torch.zeros((1 << 16, 256)))
    # the batch form: the reader's errors, then the same settings
    off = np.array([0, 2, 4], np.int64)
    flat = torch.zeros((C * T * F * 5,))
    bo = dict(tracks=ops._batch_views(flat, off, C, T, 5), ntracks=torch.zeros((2, C), dtype=torch.int32), frame_off=off,
              det=ops._batch_views(torch.zeros((C * T * F,), dtype=torch.float64), off, C, T, 1))
    for kw in (dict(score='pooled'), dict(score=torch.zeros((3, C, T))), dict(norm='x'), dict(thresh=float('nan')), dict(min_shared=0),
               dict(reduce='median')):
        with pytest.raises(ValueError):
            ops.nms_tubelets_batch(bo, **kw)
    with pytest.raises(ValueError, match="video_batch"):
        ops.nms_tubelets_batch(dict(bo, tracks=[]))
    with pytest.raises(ValueError, match="no CPU path|same GPU"):
        ops.nms_tubelets_batch(bo)


def test_signatures_and_binding():
    from vdetlib_amd import _lib, ops
    p = inspect.signature(ops.nms_tubelets).parameters
    assert list(p) == ['tracks', 'ntracks', 'score', 'tboxes', 'anchors', 'series', 'thresh', 'norm', 'reduce', 'min_shared',
                       'return_overlaps', 'sync', 'ctx']
    assert (p['thresh'].default, p['norm'].default, p['reduce'].default, p['min_shared'].default) == (0.5, 'union', 'mean', 1)
    q = inspect.signature(ops.nms_tubelets_batch).parameters
    assert list(q)[:2] == ['batch_out', 'score'] and q['score'].default == 'det'
    assert len(_lib.SYMBOLS['vdet_nms_tubelets_batch'][1]) == len(_lib.SYMBOLS['vdet_nms_tubelets'][1]) + 1
    assert ops._TUBE_NORMS == {n: i for i, n in enumerate(spec.NORMS)}


def test_header_limits_rows():
    hdr = open(os.path.join(ROOT, 'include', 'vdet_hip.h')).read()
    flat = re.sub(r'\s+', ' ', re.sub(r'\n \*', ' ', hdr))        # (the comment's line starts taken out)
    for row in ("NMS over whole tubelets: slots (vdet_nms_tubelets, vdet_nms_tubelets_batch) 1 <= T <= 256 tubelet slots per class",
                "C*T*F < 2^31 - 16, at most 65535 videos, 0 .. 4 series VDET_EINVAL",
                "NMS over whole tubelets: settings thresh not NaN, min_shared >= 1, norm 0 .. 2 (union, shared, min), score_mode 0 .. 2",
                "no float atomics on any result path",
                "rint(q * 2^24)", "(double)S / ((double)den * 16777216.0)", "equal scores by DESCENDING slot"):
        assert row in flat, row
    for name, value in (('VDET_TUBE_NORM_UNION', 0), ('VDET_TUBE_NORM_SHARED', 1), ('VDET_TUBE_NORM_MIN', 2),
                        ('VDET_TUBE_SCORE_SLOT', 0), ('VDET_TUBE_SCORE_MEAN', 1), ('VDET_TUBE_SCORE_MAX', 2)):
        assert re.search(r'#define %s %d\b' % (name, value), hdr), name
    src = open(os.path.join(ROOT, 'vdetlib_amd', 'csrc', 'tubenms_kernels.hpp')).read()
    assert 'kTubeFC = %d' % cases.CHUNK in src and 'kTubeTile = %d' % cases.TILE in src and 'kTubeMaxT = 256' in src
