"""-m gpu: ops.merge_tracks / ops.merge_tracks_batch (csrc/merge_kernels.hpp) against the reference's recorded merges
(proto_golden: protocol_misc.merge_max / merge_combine) and against `utils.protocol.merge_score_protos` run on the protos of
the test's own arrays (the converter of test_merge_tracks_cpu.py).  Every comparison is by bit pattern, a NaN equal to a NaN:
the feature only copies and selects.

Shapes: C = 3, Ta = 4, Tb = 6 (and swapped), F in {1, 64, 65, 129} -- the 64-lane chunk edge, both parities of F*5 and, with
slots landing at every offset inside a 16-byte line, the vector and the word-by-word copy paths.  The golden pair keeps its
own shape (one class, 5 tubelets, 6 frames)."""
import functools

import numpy as np
import pytest

from test_merge_tracks_cpu import blank_set, copy_set, golden_set, mirror, same_bits, sets_equal

pytestmark = pytest.mark.gpu

C, TA, TB = 3, 4, 6
FS = (1, 64, 65, 129)
CONFIGS = ((1, False), (2, True), (4, True))        # (series, tboxes)


def to_dev(s):
    import torch
    return {k: (tuple(torch.from_numpy(x).cuda() for x in v) if k == 'series' else torch.from_numpy(v).cuda()) for k, v in s.items()}


def to_host(d):
    keys = ('tracks', 'ntracks', 'anchors', 'tboxes', 'series', 'from_b')
    return {k: (tuple(x.cpu().numpy() for x in d[k]) if k == 'series' else d[k].cpu().numpy()) for k in keys if k in d}


def build_set(rng, present, anchor_frames, ntracks, nser, tboxes):
    """A set whose live slots have boxes where `present` says (clean NaN rows elsewhere, as the device stages leave them) and
    whose DEAD slots hold finite garbage in every field."""
    Cn, T, F = present.shape
    s = blank_set(Cn, T, F, nser, tboxes)
    s['ntracks'][:] = ntracks
    live = np.arange(T)[None, :] < np.asarray(ntracks)[:, None]
    hole = live[..., None] & ~present
    xy = rng.randint(0, 600, (Cn, T, F, 2)).astype(np.float32)
    s['tracks'][..., :2] = xy
    s['tracks'][..., 2:4] = xy + rng.randint(5, 200, (Cn, T, F, 2)).astype(np.float32)
    s['tracks'][..., 4] = rng.rand(Cn, T, F).astype(np.float32)
    s['tracks'][hole] = np.nan
    s['series'] = tuple(np.where(hole, np.nan, rng.randn(Cn, T, F)) for _ in range(nser))
    if tboxes:
        s['tboxes'] = (rng.rand(Cn, T, F, 4) * 500).astype(np.float32)
        s['tboxes'][hole] = np.nan
    s['anchors'][..., 0] = anchor_frames
    s['anchors'][..., 1] = -1
    s['anchors'][..., 2] = rng.rand(Cn, T).astype(np.float32)
    return s


@functools.lru_cache(maxsize=None)
def pair(F, nser, tboxes, swap, same_layout, seed=0):
    """(a, b): class 0 has tubelets on both sides (nta != ntb) and an EMPTY slot below ntracks, class 1 on one side only,
    class 2 on neither.  same_layout: paired slots have their boxes on the same frames and the same anchor frame."""
    rng = np.random.RandomState(1000 * F + 10 * nser + seed)
    Tm = max(TA, TB)
    present = rng.rand(C, Tm, F) > 0.3
    present[0, 1] = False
    af = rng.randint(1, F + 1, (C, Tm))
    other = present if same_layout else rng.rand(C, Tm, F) > 0.3
    oaf = af if same_layout else rng.randint(1, F + 1, (C, Tm))
    a = build_set(rng, present[:, :TA], af[:, :TA], [3, 0, 0], nser, tboxes)
    b = build_set(rng, other[:, :TB], oaf[:, :TB], [5, 2, 0], nser, tboxes)
    return (b, a) if swap else (a, b)


def run(a, b, scheme, **kw):
    """ops.merge_tracks on device copies -> the result as numpy; the inputs must come back bit-identical"""
    from vdetlib_amd import ops
    da, db = to_dev(a), (None if b is a else to_dev(b))
    out = to_host(ops.merge_tracks(da, da if db is None else db, scheme, **kw))
    assert sets_equal(to_host(da), a) and (db is None or sets_equal(to_host(db), b))
    return out


def check(out, want, from_b=None):
    assert sets_equal(out, want)
    if from_b is not None:
        assert out['from_b'].dtype == np.uint8 and np.array_equal(out['from_b'], from_b)
    else:
        assert 'from_b' not in out


@pytest.mark.parametrize("scheme", ["max", "combine"])
def test_golden_pair(proto_golden, scheme):
    a = golden_set(proto_golden['spatial_maxpool']['dets_c1_0.7'])[0]
    b = golden_set(proto_golden['temporal_maxpool']['w3'])[0]
    want = golden_set(proto_golden['protocol_misc']['merge_' + scheme])[0]
    out = run(a, b, scheme)
    assert sets_equal(out, want)
    if scheme == 'max':
        assert np.array_equal(out['from_b'], (b['series'][0] > a['series'][0]).astype(np.uint8)) and out['from_b'].sum() > 0


@pytest.mark.parametrize("swap", [False, True])
@pytest.mark.parametrize("nser,tboxes", CONFIGS)
@pytest.mark.parametrize("scheme", ["max", "combine"])
@pytest.mark.parametrize("F", FS)
def test_random_sets_against_the_dict_mirror(F, scheme, nser, tboxes, swap):
    """'max' on sets with the SAME holes on both sides; 'combine' on unrelated sets.  Ta < Tb and (swap) Ta > Tb."""
    a, b = pair(F, nser, tboxes, swap, scheme == 'max')
    want, from_b = mirror(a, b, scheme)
    out = run(a, b, scheme)
    check(out, want, from_b if scheme == 'max' else None)
    nta, ntb = a['ntracks'], b['ntracks']
    if scheme == 'combine':
        assert np.array_equal(out['ntracks'], nta + ntb) and out['tracks'].shape[1] == a['tracks'].shape[1] + b['tracks'].shape[1]
        dead = np.arange(out['tracks'].shape[1])[None, :] >= out['ntracks'][:, None]
        # the inputs' dead slots hold finite garbage: none of it may show
        assert dead.any() and np.isnan(out['tracks'][dead]).all() and all(np.isnan(x[dead]).all() for x in out['series'])
        assert not tboxes or np.isnan(out['tboxes'][dead]).all()
        assert (out['anchors'][dead].view(np.uint32) == 0).all()
    else:
        assert np.array_equal(out['ntracks'], nta) and same_bits(out['anchors'], a['anchors'])
        unpaired = np.arange(a['tracks'].shape[1])[None, :] >= np.minimum(nta, ntb)[:, None]
        assert same_bits(out['tracks'][unpaired], a['tracks'][unpaired]) and not out['from_b'][unpaired].any()
        if F > 1:
            assert from_b.any() and not from_b.all()


def _regular(F, nser=2, tboxes=True, seed=5):
    """a, b with a box on every frame of every slot, nta = ntb = T"""
    rng = np.random.RandomState(seed)
    present = np.ones((C, TA, F), bool)
    af = rng.randint(1, F + 1, (C, TA))
    return (build_set(rng, present, af, [TA] * C, nser, tboxes), build_set(rng, present, af, [TA] * C, nser, tboxes))


def test_max_score_edge_cases():
    F = 65
    a, b = _regular(F)
    inf, nan = np.inf, np.nan
    edge = [(0.5, 0.5), (0.0, -0.0), (-0.0, 0.0), (inf, inf), (-inf, -inf), (inf, 1e308), (1e308, inf), (-inf, -1e308), (-1e308, -inf),
            (nan, 1.0), (1.0, nan), (nan, nan), (nan, inf), (-inf, nan), (1.0, np.nextafter(1.0, 2.0)), (np.nextafter(1.0, 2.0), 1.0),
            (5e-324, 0.0), (0.0, 5e-324), (-5e-324, -0.0)]
    da, db = a['series'][0], b['series'][0]
    for i, (x, y) in enumerate(edge):
        da[:, :, (3 * i) % F], db[:, :, (3 * i) % F] = x, y
        da[0, 1, (3 * i + 1) % F], db[0, 1, (3 * i + 1) % F] = x, y
    want, from_b = mirror(a, b, 'max')
    out = run(a, b, 'max')
    check(out, want, from_b)
    with np.errstate(invalid='ignore'):
        take = db > da
    assert np.array_equal(out['from_b'], take.astype(np.uint8)) and take.any() and not take.all()
    for k in ('tracks', 'tboxes'):                  # every field of a taken box is b's, of a kept box a's
        assert same_bits(out[k][take], b[k][take]) and same_bits(out[k][~take], a[k][~take])
    for q in range(2):
        assert same_bits(out['series'][q][take], b['series'][q][take]) and same_bits(out['series'][q][~take], a['series'][q][~take])
    assert same_bits(out['anchors'], a['anchors']) and not same_bits(a['anchors'], b['anchors'])


@pytest.mark.parametrize("F", [64, 129])
@pytest.mark.parametrize("short", ["b", "a"])
def test_max_unequal_lengths(F, short):
    """one side's tubelet is a strict prefix of the other's: boxes beyond m, and slots beyond min(nt), are a's"""
    a, b = _regular(F)
    s = b if short == 'b' else a
    cut = {(0, 0): F // 2, (0, 1): 1, (1, 2): F - 1, (2, 3): 0}
    for (c, t), n in cut.items():
        s['tracks'][c, t, n:] = np.nan
        s['tboxes'][c, t, n:] = np.nan
        for x in s['series']:
            x[c, t, n:] = np.nan
    a['ntracks'][:] = [TA, 2, TA]
    b['ntracks'][:] = [TA, TA, 1]
    want, from_b = mirror(a, b, 'max')
    out = run(a, b, 'max')
    check(out, want, from_b)
    for (c, t), n in cut.items():
        assert not out['from_b'][c, t, n:].any() and same_bits(out['tracks'][c, t, n:], a['tracks'][c, t, n:])
    assert same_bits(out['tracks'][1, 2:], a['tracks'][1, 2:]) and same_bits(out['tracks'][2, 1:], a['tracks'][2, 1:])
    assert not out['from_b'][1, 2:].any() and not out['from_b'][2, 1:].any() and out['from_b'][0, 0, :F // 2].any()


def _holes(s, frames):
    for k in ('tracks', 'tboxes'):
        s[k][:, :, frames] = np.nan
    for x in s['series']:
        x[:, :, frames] = np.nan


def test_max_same_holes_on_both_sides():
    F = 129
    a, b = _regular(F)
    frames = [0, 5, 62, 63, 64, 65, 127, 128]       # around both chunk edges, first and last frame
    _holes(a, frames)
    _holes(b, frames)
    want, from_b = mirror(a, b, 'max')
    out = run(a, b, 'max')
    check(out, want, from_b)
    assert from_b.any() and not out['from_b'][:, :, frames].any()


@pytest.mark.parametrize("kind", ["holes_differ", "anchor_frame_differs", "ith_boxes_on_different_frames"])
@pytest.mark.parametrize("F", [65, 129])
def test_max_violations(F, kind):
    import torch
    from vdetlib_amd import _lib, ops
    a, b = _regular(F)
    _holes(a, [3, 64])
    _holes(b, [3, 64])
    c, t = 1, 2
    if kind == "holes_differ":                       # b lacks a box in the middle: every later ordinal shifts by one frame
        for k in ('tracks', 'tboxes'):
            b[k][c, t, 40] = np.nan
        for x in b['series']:
            x[c, t, 40] = np.nan
    elif kind == "anchor_frame_differs":
        b['anchors'][c, t, 0] = a['anchors'][c, t, 0] % F + 1
    else:                                            # the same number of boxes, one of b's moved into the hole at frame 64
        for k in ('tracks', 'tboxes'):
            b[k][c, t, 64] = b[k][c, t, 63]
            b[k][c, t, 63] = np.nan
        for x in b['series']:
            x[c, t, 64] = x[c, t, 63]
            x[c, t, 63] = np.nan
    with pytest.raises(AssertionError):
        mirror(a, b, 'max')
    fixed = copy_set(b)                              # the offending slot made harmless: equal to a's, so a is kept
    for k in ('tracks', 'tboxes', 'anchors'):
        fixed[k][c, t] = a[k][c, t]
    for x, y in zip(fixed['series'], a['series']):
        x[c, t] = y[c, t]
    want, from_b = mirror(a, fixed, 'max')
    assert not from_b[c, t].any() and same_bits(want['tracks'][c, t], a['tracks'][c, t])
    ctx = _lib.get_context(torch.cuda.current_device())
    da, db = to_dev(a), to_dev(b)
    res = ops.merge_tracks(da, db, 'max', sync=False)
    with pytest.raises(ValueError, match="merge"):
        ctx.sync()
    torch.cuda.synchronize()
    check(to_host(res), want, from_b)                # the offending slot is a's, every other slot is merged
    with pytest.raises(ValueError, match="merge"):
        ops.merge_tracks(da, db, 'max')
    ctx.sync()                                       # the status word was cleared with the report
    check(to_host(ops.merge_tracks(da, to_dev(fixed), 'max')), want, from_b)


@pytest.mark.parametrize("scheme", ["max", "combine"])
def test_a_is_b_and_async(scheme):
    import torch
    from vdetlib_amd import _lib, ops
    a, b = pair(65, 2, True, False, True)
    want, from_b = mirror(a, a, scheme)
    out = run(a, a, scheme)
    check(out, want, from_b if scheme == 'max' else None)
    if scheme == 'max':
        assert sets_equal(out, a) and not out['from_b'].any()
    da, db = to_dev(a), to_dev(b)
    res = ops.merge_tracks(da, db, scheme, sync=False)
    _lib.get_context(torch.cuda.current_device()).sync()
    sync = to_host(ops.merge_tracks(da, db, scheme))
    got = to_host(res)
    assert sets_equal(got, sync) and (scheme == 'combine' or np.array_equal(got['from_b'], sync['from_b']))
    one = to_host(ops.merge_tracks(dict(da, series=da['series'][0]), dict(db, series=db['series'][0]), scheme))   # one tensor as series
    assert len(one['series']) == 1 and same_bits(one['series'][0], sync['series'][0]) and same_bits(one['tracks'], sync['tracks'])


def _pack(sets, off, T):
    """per-video sets -> a dict in video_batch's layout on the device"""
    import torch
    V = len(sets)

    def flat(get, per, dtype):
        buf = torch.from_numpy(np.concatenate([np.ascontiguousarray(get(s)).reshape(-1) for s in sets]).astype(dtype)).cuda()
        return [buf[C * T * per * int(off[v]): C * T * per * int(off[v + 1])].view(*((C, T, int(off[v + 1] - off[v])) + ((per,) if per > 1 else ())))
                for v in range(V)]
    return dict(tracks=flat(lambda s: s['tracks'], 5, np.float32), det=flat(lambda s: s['series'][0], 1, np.float64),
                pooled=flat(lambda s: s['series'][1], 1, np.float64), tboxes=flat(lambda s: s['tboxes'], 4, np.float32),
                anchors=torch.from_numpy(np.stack([s['anchors'] for s in sets])).cuda(),
                ntracks=torch.from_numpy(np.stack([s['ntracks'] for s in sets])).cuda(), frame_off=np.asarray(off, np.int64))


@pytest.mark.parametrize("scheme", ["max", "combine"])
def test_batch_equals_single_video_calls(scheme):
    from vdetlib_amd import ops
    frames = (1, 64, 70)
    off = np.concatenate([[0], np.cumsum(frames)]).astype(np.int64)
    pairs = [pair(F, 2, True, False, scheme == 'max', seed=v + 1) for v, F in enumerate(frames)]
    ba, bb = _pack([p[0] for p in pairs], off, TA), _pack([p[1] for p in pairs], off, TB)
    out = ops.merge_tracks_batch(ba, bb, scheme)
    To = TA + TB if scheme == 'combine' else TA
    assert np.array_equal(out['frame_off'], off) and tuple(out['anchors'].shape) == (3, C, To, 3)
    keys = ('tracks', 'det', 'pooled', 'tboxes') + (('from_b',) if scheme == 'max' else ())
    for k in keys:                                  # views of ONE allocation per field, video after video
        ops._batch_flat(out[k], 1)
        assert len({x.untyped_storage().data_ptr() for x in out[k]}) == 1
    assert scheme == 'max' or 'from_b' not in out
    for v, (a, b) in enumerate(pairs):
        one = run(a, b, scheme)
        got = dict(tracks=out['tracks'][v].cpu().numpy(), ntracks=out['ntracks'][v].cpu().numpy(), anchors=out['anchors'][v].cpu().numpy(),
                   tboxes=out['tboxes'][v].cpu().numpy(), series=(out['det'][v].cpu().numpy(), out['pooled'][v].cpu().numpy()))
        assert sets_equal(got, one), v
        if scheme == 'max':
            assert np.array_equal(out['from_b'][v].cpu().numpy(), one['from_b']), v
    # pooled / tboxes are taken only when BOTH sides have them
    few = ops.merge_tracks_batch(dict(ba, pooled=[]), dict(bb, tboxes=[]), scheme)
    assert few['pooled'] == [] and few['tboxes'] == []
    assert all(same_bits(x.cpu().numpy(), y.cpu().numpy()) for x, y in zip(few['det'] + few['tracks'], out['det'] + out['tracks']))


def test_consumers_take_a_combined_set():
    import torch
    from vdetlib_amd import eval as vev, ops
    from vdetlib_amd.vdet.tcn import TCNNet
    F = 65
    a, b = pair(F, 2, True, False, False)
    da, db = to_dev(a), to_dev(b)
    out = ops.merge_tracks(da, db, 'combine')
    # the device TCN: per tubelet the conv scores of the two separate calls, in the combined slots
    net = TCNNet.random([(n, 1) for n in ('det_scores', 'track_scores', 'anchors')], hidden=(4,), kernel=3, seed=3)
    conv = lambda d: ops.tcn_tracks(net, d['tracks'], d['ntracks'], d['anchors'], d['series'][0]).cpu().numpy()
    ca, cb, cc = conv(da), conv(db), conv(out)
    boxes = 0
    for c in range(C):
        nta, ntb = int(a['ntracks'][c]), int(b['ntracks'][c])
        assert same_bits(cc[c, :nta], ca[c, :nta]) and same_bits(cc[c, nta:nta + ntb], cb[c, :ntb])
        assert np.isnan(cc[c, nta + ntb:]).all()
        boxes += int((~np.isnan(ca[c, :nta])).sum() + (~np.isnan(cb[c, :ntb])).sum())
    assert boxes > 0
    # the evaluator: the combined set adds the detections of both
    annots = [{'video': 'v', 'annotations': [
        {'id': str(c), 'track': [{'frame': 1, 'bbox': [10, 10, 59, 59], 'class_index': c + 1}]} for c in range(C)]}]
    counts = []
    for d in (da, db, out):
        ev = ops.DetEvaluator(vev.gt_table_from_annots(annots))
        counts.append(ev.add_tracks('v', d['tracks'], d['ntracks'], d['series'][0], boxes=d['tboxes']))
    assert counts[2] == counts[0] + counts[1] > 0
    # interpolate_tracks' result goes in as it is
    ia = ops.interpolate_tracks(da['tracks'], da['ntracks'], da['anchors'], da['series'], boxes=da['tboxes'])
    ib = ops.interpolate_tracks(db['tracks'], db['ntracks'], db['anchors'], db['series'], boxes=db['tboxes'])
    got = to_host(ops.merge_tracks(ia, ib, 'combine'))
    want, _ = mirror(to_host(ia), to_host(ib), 'combine')
    assert sets_equal(got, want) and np.array_equal(got['ntracks'], a['ntracks'] + b['ntracks'])
    same = to_host(ops.merge_tracks(ia, ia, 'max'))
    assert sets_equal(same, to_host(ia)) and not same['from_b'].any()
