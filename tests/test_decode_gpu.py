"""GPU: the Fast R-CNN box decode on the device (ops.decode_boxes, ops.det_nms_volume_deltas, ops.tubelet_dets) against
tests/decode_spec.py on every case of tests/decode_cases.py, and ops.dets_as_tracks against its loop -- bit for bit, no
tolerances.  A NaN equals a NaN whatever its payload."""
import functools

import numpy as np
import pytest
import torch

import decode_cases as dc
import decode_spec as ds

pytestmark = pytest.mark.gpu

DEV = 'cuda'
F32, F64 = np.float32, np.float64
IM = (375, 500)


def g(a):
    return torch.from_numpy(np.array(a, order='C')).to(DEV)       # (a copy: the shared cases are read-only)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    bits = {4: np.int32, 8: np.int64}[a.dtype.itemsize]
    return bool(np.array_equal(na, nb) and np.array_equal(a[~na].view(bits), b[~nb].view(bits)))


CASES = {c[0]: c for c in dc.cases()}


# ---- (a) decode_boxes ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(CASES))
def test_decode_boxes_on_every_case(name):
    from vdetlib_amd import ops
    _, rois, deltas, im = CASES[name]
    n, K = deltas.shape[:2]
    want = ds.decode(rois, deltas, im)
    for r in (rois, rois.astype(F64)) if rois.dtype == F32 else (rois,):
        got = ops.decode_boxes(g(r[None]), g(deltas[None]), im)
        assert got.dtype == torch.float32 and tuple(got.shape) == (1, n, K, 4)
        assert same_bits(got[0].cpu().numpy(), want), name
        flat = ops.decode_boxes(g(r[None]), g(deltas.reshape(1, n, 4 * K)), im)            # the head's [B, 4K] rows
        assert torch.equal(flat.view(torch.int32), got.view(torch.int32))
    if rois.dtype == F64 and name == 'f64_rois':
        assert not same_bits(ops.decode_boxes(g(rois.astype(F32)[None]), g(deltas[None]), im)[0].cpu().numpy(), want)


@functools.lru_cache(maxsize=None)
def volume(seed, F, B, K, f64=False):
    rois, deltas = dc.random_case(seed, F * B, K, IM, f64=f64)
    return rois.reshape(F, B, 4), deltas.reshape(F, B, K, 4)


@pytest.mark.parametrize('K', [5, 1, 67])              # 67: a wave straddles two boxes; 1: every lane its own box
@pytest.mark.parametrize('f64', [False, True])
def test_decode_boxes_volume_shapes(K, f64):
    from vdetlib_amd import ops
    F, B = 3, 150
    rois, deltas = volume(40 + K, F, B, K, f64)
    want = ds.decode(rois, deltas, IM)
    got = ops.decode_boxes(g(rois), g(deltas), IM)
    assert same_bits(got.cpu().numpy(), want)
    assert same_bits(ops.decode_boxes(g(rois), g(deltas.reshape(F, B, 4 * K)), IM).cpu().numpy(), want)
    # another image size moves the clip only
    assert same_bits(ops.decode_boxes(g(rois), g(deltas), (100, 120)).cpu().numpy(), ds.decode(rois, deltas, (100, 120)))


def test_decode_boxes_offset_views_and_empty_shapes():
    from vdetlib_amd import ops
    F, B, K = 3, 150, 5
    rois, deltas = volume(45, F, B, K)
    want = ds.decode(rois, deltas, IM)
    big_r = torch.zeros(F * B * 4 + 8, dtype=torch.float32, device=DEV)
    big_d = torch.zeros(F * B * K * 4 + 8, dtype=torch.float32, device=DEV)
    big_r[4:4 + F * B * 4] = g(rois).reshape(-1); big_d[8:] = g(deltas).reshape(-1)
    vr, vd = big_r[4:4 + F * B * 4].view(F, B, 4), big_d[8:].view(F, B, K, 4)          # 16 and 32 bytes into their storage
    assert same_bits(ops.decode_boxes(vr, vd, IM).cpu().numpy(), want)
    # a strided view is made contiguous first
    wide = torch.zeros((F, B, 8), dtype=torch.float32, device=DEV)
    wide[..., :4] = g(rois)
    assert same_bits(ops.decode_boxes(wide[..., :4], vd, IM).cpu().numpy(), want)
    big_r[1:1 + F * B * 4] = g(rois).reshape(-1)
    with pytest.raises(ValueError):
        ops.decode_boxes(big_r[1:1 + F * B * 4].view(F, B, 4), vd, IM)                 # 4 bytes in: not 16-byte aligned
    assert tuple(ops.decode_boxes(g(rois[:, :0]), g(deltas[:, :0]), IM).shape) == (F, 0, K, 4)
    assert tuple(ops.decode_boxes(g(rois), g(deltas[:, :, :0]), IM).shape) == (F, B, 0, 4)


# ---- (b) det_nms_volume_deltas ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def head_output(seed, F, B, K, levels=0):
    """rois, scores, deltas of a head: overlapping boxes, scores uniform (or quantised to ``levels``: runs of equal scores)"""
    rois, deltas = volume(seed, F, B, K)
    rng = np.random.RandomState(seed + 1000)
    S = rng.rand(F, B, K)
    S = (np.floor(S * levels) / levels if levels else S).astype(F32)
    S.setflags(write=False)
    return rois, S, deltas


def both(rois, S, deltas, im=IM, **kw):
    """(fused outputs, decode-then-NMS outputs) as device tensors"""
    from vdetlib_amd import ops
    r, s, d = g(rois), g(S), g(deltas)
    return ops.det_nms_volume_deltas(r, s, d, im, **kw), ops.det_nms_volume(ops.decode_boxes(r, d, im), s, **kw)


def all_equal(got, want):
    for a, b in zip(got, want):
        if a is None or b is None:
            assert a is None and b is None
            continue
        assert a.dtype == b.dtype and a.shape == b.shape
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))                      # dets: NaN payloads included
    return True


@pytest.mark.parametrize('topk', [7, 64, 65, 128])            # 64 | 65: the two-rows-per-lane seam of the wave
@pytest.mark.parametrize('thr', [0.05, 0.9])                  # ~380 candidates: the cut applies; ~40: box order up to topk 64
def test_fused_equals_decode_then_nms(topk, thr):
    rois, S, deltas = head_output(50, 3, 400, 5)              # F*K = 15 problems: the last block of four waves is short
    got, want = both(rois, S, deltas, score_thresh=thr, topk=topk, nms_thresh=0.3)
    assert all_equal(got, want)
    dcnt, kcnt = got[2].cpu().numpy(), got[4].cpu().numpy()
    n = (S[:, :, 1:] > thr).sum(1)
    assert np.array_equal(dcnt[:, 1:], np.minimum(n, topk)) and (kcnt[:, 1:] > 0).all() and (kcnt[:, 1:] < dcnt[:, 1:]).any()
    assert (n > topk).any() if thr == 0.05 or topk == 7 else (n <= topk).all()


@pytest.mark.parametrize('kw', [dict(score_thresh=None, topk=100), dict(first_class=0, topk=33), dict(first_class=2, topk=100),
                                dict(want_dets=False), dict(nms_thresh=0.7, score_thresh=0.5, topk=128)],
                         ids=['no_threshold', 'first_class_0', 'first_class_2', 'no_dets', 'nms_0.7'])
def test_fused_options(kw):
    rois, S, deltas = head_output(51, 2, 300, 3)
    got, want = both(rois, S, deltas, **kw)
    assert all_equal(got, want)
    if kw.get('first_class') == 2:
        assert not got[2][:, :2].any() and got[2][:, 2].all()
    if 'want_dets' in kw:
        assert got[0] is None


def test_fused_tied_scores_and_f64_rois():
    rois, S, deltas = head_output(52, 3, 400, 5, levels=12)
    for topk in (100, 37):
        assert all_equal(*both(rois, S, deltas, score_thresh=0.05, topk=topk))
        assert all_equal(*both(rois.astype(F64) + 1e-9 / 3, S, deltas, score_thresh=0.05, topk=topk))


def test_fused_nan_deltas_and_padded_frames():
    """NaN deltas among the candidates decode to NaN boxes on both routes; a frame padded with NaN rois and NaN scores selects
    nothing from its padding"""
    rois, S, deltas = (np.array(a) for a in head_output(53, 2, 200, 4))
    top = np.argsort(-S[0, :, 1])[:9]
    deltas[0, top[::2], 1, 2] = np.nan
    deltas[0, top[1], 1] = np.nan
    deltas[1, :5, 2, 0] = np.inf
    rois[1, 150:] = np.nan; S[1, 150:] = np.nan
    got, want = both(rois, S, deltas, score_thresh=0.3, topk=100)
    assert all_equal(got, want)
    assert torch.isnan(got[0][0, 1, :int(got[2][0, 1])]).any()
    sel = got[1][1].cpu().numpy()
    assert sel.max() < 150
    # against the same frame without its padding
    short = both(rois[1:, :150], S[1:, :150], deltas[1:, :150], score_thresh=0.3, topk=100)[0]
    assert all(torch.equal(a[1:].view(torch.int32), b.view(torch.int32)) for a, b in zip(got, short))


def test_fused_async_and_contexts():
    from vdetlib_amd import _lib, ops
    rois, S, deltas = head_output(54, 3, 300, 5)
    r, s, d = g(rois), g(S), g(deltas)
    want = ops.det_nms_volume(ops.decode_boxes(r, d, IM), s, topk=64)
    ctx = _lib.get_context(r.device.index)
    got = ops.det_nms_volume_deltas(r, s, d, IM, topk=64, sync=False)
    ctx.sync()
    assert all_equal(got, want)
    # a context that has run other work against a fresh one
    ops.nms_volume(g(rois), s, 0.3)
    used = ops.det_nms_volume_deltas(r, s, d, IM, topk=64)
    fresh_ctx = _lib.Context(r.device.index)
    fresh = ops.det_nms_volume_deltas(r, s, d, IM, topk=64, ctx=fresh_ctx)
    assert all_equal(used, want) and all_equal(fresh, want)
    fresh_ctx.close()


def test_fused_zero_union_raises_on_both_routes():
    """two identical inverted rois that decode to boxes of width 0 under the +1 convention, at the top of a class"""
    from vdetlib_amd import _lib, ops
    rois, S, deltas = (np.array(a) for a in head_output(55, 1, 40, 3))
    rois[0, 3] = rois[0, 9] = [10, 10, 9, 30]
    deltas[0, 3, 2] = deltas[0, 9, 2] = 0
    S[0, 3, 2], S[0, 9, 2] = 2.0, 1.5
    box = ds.decode(rois, deltas, IM)[0, 3, 2]
    assert box[2] - box[0] + F32(1) == 0
    r, s, d = g(rois), g(S), g(deltas)
    with pytest.raises(ZeroDivisionError):
        ops.det_nms_volume(ops.decode_boxes(r, d, IM), s, score_thresh=None, topk=100)
    with pytest.raises(ZeroDivisionError):
        ops.det_nms_volume_deltas(r, s, d, IM, score_thresh=None, topk=100)
    ctx = _lib.get_context(r.device.index)
    ops.det_nms_volume_deltas(r, s, d, IM, score_thresh=None, topk=100, sync=False)
    with pytest.raises(ZeroDivisionError):
        ctx.sync()
    ctx.sync()


def test_fused_against_the_oracle_on_spec_decoded_rows(oracle):
    """an expectation that does not pass through the library: the rows of fast_rcnn_det_vid's per-class loop from the numpy
    decode, and the oracle's nms of those rows"""
    from vdetlib_amd import ops
    rois, S, deltas = head_output(56, 2, 300, 4)
    F, B, K = S.shape
    BX = ds.decode(rois, deltas, IM)
    for thr, k in ((0.05, 100), (0.8, 100)):
        dets, sel, dcnt, keep, kcnt = (t.cpu().numpy() for t in ops.det_nms_volume_deltas(g(rois), g(S), g(deltas), IM,
                                                                                          score_thresh=thr, topk=k))
        for f in range(F):
            rows = oracle.threshold_topk(S[f], BX[f].reshape(B, 4 * K), thr, k)
            assert dcnt[f, 0] == 0 and kcnt[f, 0] == 0
            for j in range(1, K):
                want = np.asarray(rows[j], F32).reshape(-1, 5)
                n = int(dcnt[f, j])
                assert n == len(want) > 0 and np.array_equal(dets[f, j, :n], want), (f, j)
                assert np.array_equal(BX[f, sel[f, j, :n], j], want[:, :4])
                assert keep[f, j, :int(kcnt[f, j])].tolist() == oracle.nms(want, 0.3), (f, j)
                assert np.all(keep[f, j, int(kcnt[f, j]):] == -1) and np.isnan(dets[f, j, n:]).all()


# ---- (c) tubelet_dets ---------------------------------------------------------------------------------------------------
C, T, F, K = 3, 4, 6, 5
HOLES = ((0, 1, 2), (0, 3, 4), (2, 0, 0), (2, 1, 5))


@functools.lru_cache(maxsize=None)
def tubelets():
    rng = np.random.RandomState(60)
    rois, _ = dc.random_case(60, C * T * F, 1, IM)
    tr = np.concatenate([rois.reshape(C, T, F, 4), rng.rand(C, T, F, 1).astype(F32)], -1)
    for c, t, f in HOLES:
        tr[c, t, f] = np.nan
    nt = np.asarray([4, 0, 2], np.int32)
    return tr, nt


def present(tr, nt, f0, f1):
    return np.asarray([(c, t, f) for f in range(f0, f1) for c in range(C) for t in range(int(nt[c])) if tr[c, t, f, 0] == tr[c, t, f, 0]],
                      np.int32).reshape(-1, 3)


def head_rows(seed, n):
    rng = np.random.RandomState(seed)
    return rng.rand(n, K).astype(F32), (rng.standard_normal((n, 4 * K)) * 0.4).astype(F32)


def expected_dets(tr, slots, scores, deltas, cols, det=None, tboxes=None):
    det = np.full((C, T, F), np.nan, F64) if det is None else det.copy()
    tboxes = np.full((C, T, F, 4), np.nan, F32) if tboxes is None else tboxes.copy()
    for n, (c, t, f) in enumerate(slots):
        det[c, t, f] = F64(scores[n, cols[c]])
        tboxes[c, t, f] = ds.decode(tr[c, t, f, :4], deltas[n].reshape(K, 4)[cols[c]][None], IM)[0]
    return det, tboxes


def test_tubelet_dets_against_the_loop():
    from vdetlib_amd import ops
    tr, nt = tubelets()
    slots = present(tr, nt, 0, F)
    n = len(slots)
    scores, deltas = head_rows(61, n + 3)
    pad = np.concatenate([slots, np.full((3, 3), -1, np.int32)])
    count = torch.tensor([n], dtype=torch.int32, device=DEV)
    out = ops.tubelet_dets(g(scores), g(deltas), g(tr), g(pad), count, IM)
    wdet, wtb = expected_dets(tr, slots, scores, deltas, [1, 2, 3])
    assert out['det'].dtype == torch.float64 and out['tboxes'].dtype == torch.float32
    assert same_bits(out['det'].cpu().numpy(), wdet) and same_bits(out['tboxes'].cpu().numpy(), wtb)
    assert np.isnan(wdet).sum() == C * T * F - n
    # [N,K,4] deltas, f64 track rows of four, a class -> column map, a count below the rows given
    cols = np.asarray([4, 0, 2], np.int32)
    few = torch.tensor([n - 5], dtype=torch.int32, device=DEV)
    out = ops.tubelet_dets(g(scores), g(deltas.reshape(-1, K, 4)), g(tr[..., :4].astype(F64)), g(pad), few, IM, cols=g(cols),
                           shape=(C, T, F))
    wdet, wtb = expected_dets(tr, slots[:n - 5], scores, deltas, cols)
    assert same_bits(out['det'].cpu().numpy(), wdet) and same_bits(out['tboxes'].cpu().numpy(), wtb)
    # count None: all rows
    out = ops.tubelet_dets(g(scores[:n]), g(deltas[:n]), g(tr), g(slots), None, IM)
    wdet, wtb = expected_dets(tr, slots, scores, deltas, [1, 2, 3])
    assert same_bits(out['det'].cpu().numpy(), wdet) and same_bits(out['tboxes'].cpu().numpy(), wtb)


def test_tubelet_dets_out_over_two_frame_ranges():
    from vdetlib_amd import ops
    tr, nt = tubelets()
    out, wdet, wtb = None, None, None
    for k, (f0, f1) in enumerate(((0, 2), (2, F))):
        slots = present(tr, nt, f0, f1)
        scores, deltas = head_rows(62 + k, len(slots))
        out = ops.tubelet_dets(g(scores), g(deltas), g(tr), g(slots), None, IM, out=out)
        wdet, wtb = expected_dets(tr, slots, scores, deltas, [1, 2, 3], wdet, wtb)
        assert same_bits(out['det'].cpu().numpy(), wdet) and same_bits(out['tboxes'].cpu().numpy(), wtb)
    assert not np.isnan(wdet[0, 0]).any() and np.isnan(wdet[1]).all()


def test_tubelet_dets_bad_slot_and_bad_column_at_the_wait():
    from vdetlib_amd import _lib, ops
    tr, nt = tubelets()
    slots = present(tr, nt, 0, 3)
    scores, deltas = head_rows(64, len(slots))
    ctx = _lib.get_context(torch.cuda.current_device())
    for bad_slot, cols in (((C, 0, 0), None), ((0, T, 0), None), ((0, 0, -1), None), (None, [1, 2, K]), (None, [-1, 2, 3])):
        s = slots.copy()
        if bad_slot is not None:
            s[2] = bad_slot
        gc = None if cols is None else g(np.asarray(cols, np.int32))
        out = ops.tubelet_dets(g(scores), g(deltas), g(tr), g(s), None, IM, cols=gc, sync=False)
        with pytest.raises(ValueError):
            ctx.sync()
        ctx.sync()                                  # reported once
        skip = np.arange(len(s)) == 2 if bad_slot is not None else (s[:, 0] == (2 if cols[2] == K else 0))
        wdet, wtb = expected_dets(tr, s[~skip], scores[~skip], deltas[~skip], [1, 2, 3] if cols is None else cols)
        assert same_bits(out['det'].cpu().numpy(), wdet) and same_bits(out['tboxes'].cpu().numpy(), wtb)
        with pytest.raises(ValueError):
            ops.tubelet_dets(g(scores), g(deltas), g(tr), g(s), None, IM, cols=gc)


def test_round_trip_rois_head_dets_rescore():
    """tubelet_rois -> a toy head -> tubelet_dets -> rescore_tubelets(floor=det): equals tests/rescore_spec.py given the floor
    the loop builds from the same head output, and the decoded boxes go into nms_tracks as tboxes"""
    import rescore_spec
    import synth
    from vdetlib_amd import ops
    Fv, B, Cv, Tv, Kf = 5, 40, 2, 3, 4
    boxes, scores = synth.coherent_video(77, Fv, B, Cv)
    feat = (np.random.RandomState(81).normal(size=(Fv, Kf, (synth.H + 7) // 8, (synth.W + 7) // 8)) - 1).astype(F32)
    tb, ts = g(boxes), g(scores)
    fr, ab, sc, _ = ops.top_anchors(tb, ts, Tv)
    tr, an, nt = ops.track_from_anchors(tb, fr, ab, sc)
    cap = Cv * Tv * Fv
    pooled = ops.tubelet_rois(g(feat), tr, nt, (0, Fv), cap, spatial_scale=0.125, pooled=(2, 2))
    n = int(pooled['count'])
    assert n > Fv
    gen = torch.Generator().manual_seed(82)
    ws = (torch.randn(Kf * 4, Cv + 1, generator=gen) * 0.3).to(DEV)
    wd = (torch.randn(Kf * 4, 4 * (Cv + 1), generator=gen) * 0.05).to(DEV)
    flat = pooled['pooled'].reshape(cap, -1)
    hs, hd = torch.softmax(flat @ ws, 1), (flat @ wd).contiguous()
    out = ops.tubelet_dets(hs, hd, tr, pooled['slot'], pooled['count'], (synth.H, synth.W))
    trn, ntn, slots = tr.cpu().numpy(), nt.cpu().numpy(), pooled['slot'][:n].cpu().numpy()
    hsn, hdn = hs.cpu().numpy(), hd.cpu().numpy()
    wdet = np.full((Cv, Tv, Fv), np.nan, F64)
    wtb = np.full((Cv, Tv, Fv, 4), np.nan, F32)
    for i, (c, t, f) in enumerate(slots):
        wdet[c, t, f] = F64(hsn[i, c + 1])
        wtb[c, t, f] = ds.decode(trn[c, t, f, :4], hdn[i].reshape(Cv + 1, 4)[c + 1][None], (synth.H, synth.W))[0]
    assert same_bits(out['det'].cpu().numpy(), wdet) and same_bits(out['tboxes'].cpu().numpy(), wtb)
    det, pl, tboxes, src = ops.rescore_tubelets(tr, nt, tb, ts, floor=out['det'])
    sdet, spl, stb, ssrc, eindex = rescore_spec.spec(trn, ntn, boxes, scores, floor=wdet)
    assert not eindex
    assert np.array_equal(det.cpu().numpy(), sdet, equal_nan=True) and np.array_equal(pl.cpu().numpy(), spl, equal_nan=True)
    assert np.array_equal(tboxes.cpu().numpy(), stb, equal_nan=True) and np.array_equal(src.cpu().numpy(), ssrc)
    lists = ops.nms_tracks(tr, nt, out['det'], tboxes=out['tboxes'])
    assert int(lists['cnt'].sum()) > 0


# ---- dets_as_tracks -----------------------------------------------------------------------------------------------------
def test_dets_as_tracks_against_the_loop():
    from vdetlib_amd import ops
    rois, S, deltas = head_output(70, 4, 200, 5)
    for first, topk in ((1, 30), (0, 7), (2, 128)):
        outs = ops.det_nms_volume_deltas(g(rois), g(S), g(deltas), IM, score_thresh=0.3, topk=topk, first_class=first)
        dets, sel, dcnt, keep, kcnt = outs
        got = ops.dets_as_tracks(dets, sel, keep, kcnt, first_class=first)
        want = ds.dets_as_tracks(*(t.cpu().numpy() for t in (dets, sel, keep, kcnt)), first_class=first)
        assert sorted(got) == sorted(want)
        for k in want:
            a = got[k].cpu().numpy()
            assert a.dtype == want[k].dtype and (same_bits(a, want[k]) if a.dtype.kind == 'f' else np.array_equal(a, want[k])), k
        assert int(got['ntracks'].max()) > 1 and bool((got['src'][:, 0] >= 0).all())
    # frames without a survivor in one class: cnt 0, NaN rows
    S0 = np.array(S); S0[1, :, 2] = 0
    outs = ops.det_nms_volume_deltas(g(rois), g(S0), g(deltas), IM, score_thresh=0.3, topk=30)
    got = ops.dets_as_tracks(outs[0], outs[1], outs[3], outs[4])
    assert int(got['cnt'][1, 1]) == 0 and bool(torch.isnan(got['tracks'][1, :, 1]).all()) and bool((got['src'][1, :, 1] == -2 ** 31).all())


def test_dets_as_tracks_feeds_the_evaluator_seq_nms_and_nms_tracks():
    import synth
    from test_eval_gpu import _check
    from vdetlib_amd import eval as vev, ops
    Fv, B, Cv = 12, 120, 3
    boxes, scores, annot = synth.vid_with_objects(71, Fv, B, Cv)
    rng = np.random.RandomState(72)
    S = np.concatenate([np.zeros((Fv, B, 1), F32), scores], 2)
    deltas = (rng.standard_normal((Fv, B, Cv + 1, 4)) * 0.02).astype(F32)
    outs = ops.det_nms_volume_deltas(g(boxes), g(S), g(deltas), (synth.H, synth.W), score_thresh=0.02, topk=50, nms_thresh=0.5)
    d = ops.dets_as_tracks(outs[0], outs[1], outs[3], outs[4])
    classes = list(range(1, Cv + 1))               # every class of the head, with ground truth in the video or not
    ev = ops.DetEvaluator(vev.gt_table_from_annots([annot]), classes=classes)
    want = ds.dets_as_tracks(*(t.cpu().numpy() for t in (outs[0], outs[1], outs[3], outs[4])))
    assert ev.add_detections(annot['video'], d) == int(want['cnt'].sum()) > Fv
    host = vev.detections_from_tracks(annot['video'], want['tracks'], want['ntracks'], want['score'])
    assert len(host) == int(want['cnt'].sum())
    aps, m = _check(ev, host, [annot], 'voc', classes=classes)
    assert m > 0
    sq = ops.seq_nms(d, score='score')
    assert tuple(sq['tracks'].shape) == tuple(d['tracks'].shape) and int(sq['nseq'].sum()) > 0
    again = ops.nms_tracks(d, score=d['score'], thresh=0.5)
    # the lists are already NMS survivors at 0.5: a second pass keeps every row (rows of equal score may swap places)
    assert torch.equal(again['cnt'], d['cnt']) and same_bits(again['score'].cpu().numpy(), d['score'].cpu().numpy())


# ---- argument errors ----------------------------------------------------------------------------------------------------
def test_argument_errors():
    from vdetlib_amd import ops
    rois, S, deltas = head_output(80, 2, 50, 3)
    r, s, d = g(rois), g(S), g(deltas)
    bad = [lambda: ops.decode_boxes(r.half(), d, IM), lambda: ops.decode_boxes(r, d.double(), IM), lambda: ops.decode_boxes(r[0], d, IM),
           lambda: ops.decode_boxes(r[..., :3], d, IM), lambda: ops.decode_boxes(r, d[:1], IM), lambda: ops.decode_boxes(r, d[..., :3], IM),
           lambda: ops.decode_boxes(r, d.reshape(2, 50, 12)[..., :10], IM), lambda: ops.decode_boxes(r, d, (0, 500)),
           lambda: ops.decode_boxes(r, d, (375, 0)), lambda: ops.decode_boxes(r, d, 375), lambda: ops.decode_boxes(r.cpu(), d, IM),
           lambda: ops.decode_boxes(r.cpu(), d.cpu(), IM), lambda: ops.decode_boxes(rois, deltas, IM),
           lambda: ops.det_nms_volume_deltas(r, s.double(), d, IM), lambda: ops.det_nms_volume_deltas(r, s[0], d, IM),
           lambda: ops.det_nms_volume_deltas(r.half(), s, d, IM), lambda: ops.det_nms_volume_deltas(r, s, d.half(), IM),
           lambda: ops.det_nms_volume_deltas(r[:, :49], s, d, IM), lambda: ops.det_nms_volume_deltas(r, s, d[:, :, :2], IM),
           lambda: ops.det_nms_volume_deltas(r, s[..., :2], d, IM), lambda: ops.det_nms_volume_deltas(r, s, d, (375, 0)),
           lambda: ops.det_nms_volume_deltas(r, s, d, (-1, 500)), lambda: ops.det_nms_volume_deltas(r, s.cpu(), d, IM),
           lambda: ops.det_nms_volume_deltas(r, s, d, IM, topk=0), lambda: ops.det_nms_volume_deltas(r, s, d, IM, topk=129),
           lambda: ops.det_nms_volume_deltas(r, s, d, IM, first_class=-1)]
    big = 32768                                     # one beyond det_nms_volume's boxes per frame
    zr, zs = torch.zeros((1, big, 4), device=DEV), torch.zeros((1, big, 2), device=DEV)
    bad += [lambda: ops.det_nms_volume_deltas(zr, zs, torch.zeros((1, big, 8), device=DEV), IM)]
    assert ops.det_nms_volume_deltas(r, s, d, IM, topk=128)[2].shape == (2, 3)
    tr, nt = tubelets()
    slots = present(tr, nt, 0, F)
    sc, dl = head_rows(81, len(slots))
    gs, gd, gt, gl = g(sc), g(dl), g(tr), g(slots)
    cnt = torch.tensor([3], dtype=torch.int32, device=DEV)
    ok = ops.tubelet_dets(gs, gd, gt, gl, cnt, IM)
    bad += [lambda: ops.tubelet_dets(gs.double(), gd, gt, gl, cnt, IM), lambda: ops.tubelet_dets(gs, gd[:, :16], gt, gl, cnt, IM),
            lambda: ops.tubelet_dets(gs, gd.double(), gt, gl, cnt, IM), lambda: ops.tubelet_dets(gs, gd, gt[..., :3], gl, cnt, IM),
            lambda: ops.tubelet_dets(gs, gd, gt.half(), gl, cnt, IM), lambda: ops.tubelet_dets(gs, gd, gt, gl.long(), cnt, IM),
            lambda: ops.tubelet_dets(gs, gd, gt, gl[:-1], cnt, IM), lambda: ops.tubelet_dets(gs, gd, gt, gl, cnt.long(), IM),
            lambda: ops.tubelet_dets(gs, gd, gt, gl, cnt, (375, 0)), lambda: ops.tubelet_dets(gs, gd, gt, gl, cnt, IM, shape=(C, T, F + 1)),
            lambda: ops.tubelet_dets(gs, gd, gt, gl, cnt, IM, cols=torch.zeros(C, dtype=torch.int64, device=DEV)),
            lambda: ops.tubelet_dets(gs, gd, gt, gl, cnt, IM, cols=torch.zeros(C + 1, dtype=torch.int32, device=DEV)),
            lambda: ops.tubelet_dets(gs[:, :C], gd[:, :4 * C], gt, gl, cnt, IM),                  # the default cols need K >= C + 1
            lambda: ops.tubelet_dets(gs, gd, gt, gl, cnt, IM, out=dict(det=ok['det'])),
            lambda: ops.tubelet_dets(gs, gd, gt, gl, cnt, IM, out=dict(det=ok['det'].float(), tboxes=ok['tboxes'])),
            lambda: ops.tubelet_dets(gs, gd, gt, gl, cnt, IM, out=dict(det=ok['det'][:, :2], tboxes=ok['tboxes'][:, :2])),
            lambda: ops.tubelet_dets(gs, gd, gt, gl.cpu(), cnt, IM), lambda: ops.tubelet_dets(gs, gd, gt[:, :, ::2], gl, cnt, IM)]
    dets, sel, dcnt, keep, kcnt = ops.det_nms_volume_deltas(r, s, d, IM, topk=20)
    nodets = ops.det_nms_volume_deltas(r, s, d, IM, topk=20, want_dets=False)[0]
    bad += [lambda: ops.dets_as_tracks(nodets, sel, keep, kcnt), lambda: ops.dets_as_tracks(dets.double(), sel, keep, kcnt),
            lambda: ops.dets_as_tracks(dets[..., :4], sel, keep, kcnt), lambda: ops.dets_as_tracks(dets, sel.long(), keep, kcnt),
            lambda: ops.dets_as_tracks(dets, sel, keep[:, :, :19], kcnt), lambda: ops.dets_as_tracks(dets, sel, keep, kcnt[:1]),
            lambda: ops.dets_as_tracks(dets, sel, keep, kcnt, first_class=3), lambda: ops.dets_as_tracks(dets, sel, keep, kcnt, first_class=-1),
            lambda: ops.dets_as_tracks(dets, sel, keep, kcnt.cpu()), lambda: ops.dets_as_tracks(dets[:0], sel[:0], keep[:0], kcnt[:0])]
    for i, fn in enumerate(bad):
        with pytest.raises(ValueError):
            fn()
            pytest.fail("case %d did not raise" % i)
