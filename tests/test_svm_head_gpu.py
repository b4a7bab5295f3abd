"""GPU: the SVM head of the CNN scorers on the device (ops.svm_head, ops.svm_scores and the dict level above them) against
tests/svm_spec.py, bit for bit: every finite score is compared on its bits (NaN scores as NaN), winners and boxes exactly."""
import functools
import gzip
import json
import os

import numpy as np
import pytest
import torch

import svm_spec as ss

pytestmark = pytest.mark.gpu

DEV = 'cuda'
NP_OF = {'f64': np.float64, 'f32': np.float32}


def g(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def store(x, fdt):
    """f64 values -> (the array svm_spec reads, the device tensor) in storage dtype fdt."""
    if fdt == 'bf16':
        bits = ss.to_bf16(x.astype(np.float32))
        return bits, g(bits.view(np.int16)).view(torch.bfloat16)
    a = x.astype({'f64': np.float64, 'f32': np.float32, 'f16': np.float16}[fdt])
    return a, g(a)


def model_of(seed, K, M, wdt):
    """An asymmetric W (+ column*0.01 + k*0.001: a transposed or shifted column cannot pass), B, and feat_norm_mean -- a float64
    scalar with a float64 W (the .mat models), a python float with a float32 W (numpy's result type is then float32)."""
    rng = np.random.RandomState(seed)
    W = rng.uniform(-1, 1, (K, M)) + np.arange(M)[None] * 0.01 + np.arange(K)[:, None] * 0.001
    B = rng.uniform(-0.5, 0.5, M)
    fnm = 19.25 + rng.rand()
    dt = NP_OF[wdt]
    return {'W': W.astype(dt), 'B': B.astype(dt), 'feat_norm_mean': np.float64(fnm) if wdt == 'f64' else float(fnm)}


def cdt_of(fdt, wdt):
    return np.float32 if (fdt != 'f64' and wdt == 'f32') else np.float64


def scale_of(model, cdt):
    s = 20. / model['feat_norm_mean']
    return float(np.float32(s)) if cdt == np.float32 else float(s)


def dev_model(model):
    return {'W': g(model['W']), 'B': g(model['B']), 'feat_norm_mean': model['feat_norm_mean']}


def slots_of(seed, N, shape):
    C, T, F = shape
    assert C * T * F >= N
    flat = np.random.RandomState(seed).permutation(C * T * F)[:N]
    return np.stack([flat // (T * F), (flat // F) % T, flat % F], 1).astype(np.int32)


def same(got, want, what=''):
    """A device tensor against the spec's array: dtype, shape, NaN places, and the bits everywhere else."""
    got = got.cpu().numpy()
    want = np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    if got.dtype.kind == 'f':
        assert np.array_equal(np.isnan(got), np.isnan(want)), what
        iv = {4: np.int32, 8: np.int64}[got.dtype.itemsize]
        keep = ~np.isnan(want)
        assert np.array_equal(got[keep].view(iv), want[keep].view(iv)), what
    else:
        assert np.array_equal(got, want), what


def check(out, want, what=''):
    for k in ('score', 'arg_flat', 'det', 'arg', 'tboxes'):
        if want[k] is None:
            assert out[k] is None, (what, k)
        else:
            same(out[k], want[k], '%s %s' % (what, k))
    assert out['nbad'].dtype == torch.int32 and out['nbad'].cpu().tolist() == [want['nbad']], what


def run_case(seed, N, G, K, fdt='f32', wdt='f64', M=7, shape=None, with_slot=True, with_boxes=True, what=''):
    from vdetlib_amd import ops
    rng = np.random.RandomState(seed)
    model = model_of(seed + 1, K, M, wdt)
    cdt = cdt_of(fdt, wdt)
    feat, dfeat = store(rng.randn(N * G, K), fdt)
    shape = shape or (3, 2, max(1, (N + 5) // 6 + 1))
    C = shape[0]
    cols = ((np.arange(C) * 3 + 2) % M).astype(np.int32)                     # no identity
    slot = slots_of(seed + 2, N, shape) if with_slot else None
    sboxes = rng.uniform(1, 300, (N, G, 4)) if with_boxes else None
    kw = dict(group=G, cols=cols if with_slot else cols[:1], sboxes=sboxes)
    want = ss.head(feat, model['W'], model['B'], scale_of(model, cdt), cdt, slot=slot, shape=shape if with_slot else None, **kw)
    assert not want['bad']
    out = ops.svm_head(dfeat, dev_model(model), group=G, slot=None if slot is None else g(slot), shape=shape if with_slot else None,
                       cols=g(kw['cols']), sboxes=None if sboxes is None else g(sboxes))
    assert out['score'].dtype == (torch.float32 if cdt == np.float32 else torch.float64)
    check(out, want, what or 'N=%d G=%d K=%d %s/%s' % (N, G, K, fdt, wdt))
    return out, want


# 511 / 512 / 520: the one-round / two-round register paths; 1024 / 1032: the register cap against the chunked path; sizes that
# are no multiple of 8 take the element-load form of the chunked path
@pytest.mark.parametrize('K', [1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 511, 512, 520, 1024, 1025, 1027, 1032, 2056])
def test_every_k_path(K):
    for wdt in ('f64', 'f32'):
        run_case(100 + K, 5, 3, K, 'f32', wdt)


@pytest.mark.parametrize('G', [1, 2, 33, 256])
def test_group_sizes_and_counts(G):
    for N in (0, 1, 3, 4, 5, 257):
        run_case(200 + G + N, N, G, 24, 'f32', 'f64')
    run_case(300 + G, 5, G, 1024, 'f32', 'f64')
    run_case(301 + G, 4, G, 13, 'f32', 'f32', with_slot=False)


def test_many_groups_past_the_grid_axis_limit():
    run_case(400, 70000, 1, 8, 'f32', 'f64', shape=(2, 5, 7000))


@pytest.mark.parametrize('wdt', ['f64', 'f32'])
@pytest.mark.parametrize('fdt', ['f64', 'f32', 'f16', 'bf16'])
def test_storage_dtypes(fdt, wdt):
    for K in (40, 1024, 1027):
        out, want = run_case(500 + K, 5, 3, K, fdt, wdt)
    assert want['score'].dtype == (np.float32 if (fdt != 'f64' and wdt == 'f32') else np.float64)


def test_order_does_not_depend_on_storage_or_grouping():
    """The same values stored as f16 and as f32, and the same windows grouped by 1, 4 and 8: the same window scores."""
    from vdetlib_amd import ops
    rng = np.random.RandomState(600)
    K, M = 1024, 5
    model = model_of(601, K, M, 'f64')
    x = rng.randn(16, K).astype(np.float16)
    dm = dev_model(model)
    cols = g(np.array([3], np.int32))
    base = ops.svm_head(g(x), dm, cols=cols)['score']
    for t in (g(x.astype(np.float32)), g(x.astype(np.float64))):
        assert torch.equal(ops.svm_head(t, dm, cols=cols)['score'], base)
    for G in (4, 8):
        o = ops.svm_head(g(x), dm, group=G, cols=cols)
        assert torch.equal(o['score'], base.view(-1, G).max(1).values)
        assert torch.equal(o['arg_flat'].long(), base.view(-1, G).argmax(1))


def test_identity_probe():
    """Unit feature rows: one product, sums with zeros only -- W[k,col]*scale + B[col] exactly, without the spec."""
    from vdetlib_amd import ops
    for wdt, K in (('f64', 1024), ('f32', 1024), ('f64', 77), ('f64', 1032)):
        model = model_of(700 + K, K, 9, wdt)
        cdt = NP_OF[wdt]
        scale = cdt(scale_of(model, cdt))
        for col in (0, 4, 8):
            out = ops.svm_head(g(np.eye(K, dtype=cdt)), dev_model(model), cols=g(np.array([col], np.int32)))
            want = (cdt(1) * scale) * model['W'][:, col] + model['B'][col]
            same(out['score'], want, 'K=%d col=%d' % (K, col))
            assert not out['arg_flat'].any() and out['det'] is None and out['arg'] is None and out['tboxes'] is None


def test_duplicates_and_nans():
    from vdetlib_amd import ops
    rng = np.random.RandomState(800)
    N, G, K = 4, 7, 64
    model = model_of(801, K, 6, 'f64')
    x = rng.randn(N, G, K).astype(np.float32)
    x[0, :] = x[0, 0]                                    # all windows equal: window 0
    x[1, 5] = x[1, 2]                                    # window 2 twice, and made the winner below
    x[2, 3, 10] = np.nan                                 # the first NaN wins
    x[2, 6, 0] = np.nan
    x[3, 0, 5] = np.nan                                  # a NaN in window 0
    cols = np.array([1], np.int32)
    sb = rng.uniform(1, 300, (N, G, 4))
    scale = scale_of(model, np.float64)
    s = ss.window_scores(x.reshape(-1, K), model['W'], model['B'], scale, np.full(N * G, 1), np.float64).reshape(N, G)
    # make window 2 and its copy 5 of box 1 the largest (the former winner's row moves there)
    j = int(np.argmax(s[1]))
    row = x[1, j].copy()
    if j not in (2, 5):
        x[1, j] = x[1, 0]
    x[1, 2] = x[1, 5] = row
    want = ss.head(x.reshape(-1, K), model['W'], model['B'], scale, np.float64, group=G, cols=cols, sboxes=sb)
    assert want['arg_flat'].tolist()[0] == 0 and want['arg_flat'].tolist()[2:] == [3, 0] and np.isnan(want['score'][2:]).all()
    w1 = want['windows'].reshape(N, G)[1]
    assert w1[2] == w1[5] == w1.max() and want['arg_flat'][1] == int(np.argmax(w1)) <= 2
    out = ops.svm_head(g(x.reshape(-1, K)), dev_model(model), group=G, cols=g(cols), sboxes=g(sb))
    check(out, want)
    assert np.array_equal(out['tboxes'].cpu().numpy(), sb[np.arange(N), want['arg_flat']])


def test_ok_masks():
    from vdetlib_amd import ops
    rng = np.random.RandomState(900)
    N, G, K = 6, 5, 48
    shape = (2, 3, 4)
    model = model_of(901, K, 6, 'f64')
    x = rng.randn(N * G, K).astype(np.float32)
    ok = (rng.rand(N, G) < 0.6).astype(np.uint8)
    ok[1] = 0                                            # a whole box masked
    ok[4] = 0
    ok[2] = 1
    x[np.flatnonzero(ok.reshape(-1) == 0)] = np.nan      # what a masked window holds must not matter
    slot = slots_of(902, N, shape)
    sb = rng.uniform(1, 300, (N, G, 4))
    scale = scale_of(model, np.float64)
    want = ss.head(x, model['W'], model['B'], scale, np.float64, group=G, slot=slot, shape=shape, sboxes=sb, ok=ok)
    assert want['nbad'] == 2 and want['arg_flat'][1] == -1 and np.isnan(want['score'][1]) and not np.isnan(want['score'][[0, 2, 3, 5]]).any()
    for okt in (g(ok), g(ok.reshape(-1))):
        out = ops.svm_head(g(x), dev_model(model), group=G, slot=g(slot), shape=shape, sboxes=g(sb), ok=okt)
        check(out, want)


def test_device_count_and_unread_rows():
    from vdetlib_amd import ops
    rng = np.random.RandomState(1000)
    N, G, K, n = 9, 3, 32, 6
    shape = (2, 3, 4)
    model = model_of(1001, K, 6, 'f64')
    x = rng.randn(N * G, K).astype(np.float32)
    slot = slots_of(1002, N, shape)
    slot[n:] = -1                                        # what tubelet_patches leaves behind the count
    scale = scale_of(model, np.float64)
    want = ss.head(x, model['W'], model['B'], scale, np.float64, group=G, slot=slot, shape=shape, count=n)
    assert not want['bad'] and np.isnan(want['score'][n:]).all() and (want['arg_flat'][n:] == -1).all()
    out = ops.svm_head(g(x), dev_model(model), group=G, slot=g(slot), shape=shape, count=g(np.array([n], np.int32)))
    check(out, want)
    assert int(torch.isnan(out['det']).sum()) == 24 - n
    # a count beyond N means N
    want = ss.head(x[:n * G], model['W'], model['B'], scale, np.float64, group=G, slot=slot[:n], shape=shape)
    out = ops.svm_head(g(x[:n * G]), dev_model(model), group=G, slot=g(slot[:n]), shape=shape, count=g(np.array([n + 5], np.int32)))
    check(out, want)


def test_frame_ranges_through_out():
    from vdetlib_amd import ops
    rng = np.random.RandomState(1100)
    N, G, K = 10, 4, 40
    shape = (2, 2, 6)
    model = model_of(1101, K, 6, 'f64')
    dm = dev_model(model)
    x = rng.randn(N * G, K).astype(np.float32)
    slot = slots_of(1102, N, shape)
    slot = slot[np.argsort(slot[:, 2], kind='stable')]                       # frames in order, as the patch calls give them
    sb = rng.uniform(1, 300, (N, G, 4))
    whole = ops.svm_head(g(x), dm, group=G, slot=g(slot), shape=shape, sboxes=g(sb))
    a = 6
    first = ops.svm_head(g(x[:a * G]), dm, group=G, slot=g(slot[:a]), shape=shape, sboxes=g(sb[:a]))
    assert int(torch.isnan(first['det']).sum()) == 24 - a
    second = ops.svm_head(g(x[a * G:]), dm, group=G, slot=g(slot[a:]), sboxes=g(sb[a:]), out=first)
    for k in ('det', 'arg', 'tboxes'):
        assert second[k] is first[k]
        same(second[k], whole[k].cpu().numpy(), k)
    assert int(torch.isnan(whole['det']).sum()) == 24 - N and int((whole['arg'] == -1).sum()) == 24 - N
    assert torch.equal(torch.cat([first['score'], second['score']]), whole['score'])


def test_bad_slot_and_bad_column_raise_at_the_sync_and_write_nothing():
    from vdetlib_amd import _lib, ops
    rng = np.random.RandomState(1200)
    N, G, K = 5, 2, 16
    shape = (2, 2, 3)
    model = model_of(1201, K, 4, 'f64')
    dm = dev_model(model)
    x = g(rng.randn(N * G, K).astype(np.float32))
    good = slots_of(1202, N, shape)
    sb = g(rng.uniform(1, 300, (N, G, 4)))
    ref = ops.svm_head(x, dm, group=G, slot=g(good), shape=shape, sboxes=sb)
    ctx = _lib.get_context(x.device.index)
    for bad_slot, cols in (((0, 0, 3), None), ((2, 0, 0), None), ((0, -1, 0), None), ((0, 2, 1), None), (None, [1, 4]), (None, [-1, 0])):
        slot = good.copy()
        if bad_slot is not None:
            slot[2] = bad_slot
        ct = None if cols is None else g(np.asarray(cols, np.int32))
        hit = [2] if bad_slot is not None else [i for i in range(N) if not 0 <= cols[good[i, 0]] < 4]
        assert hit
        out = ops.svm_head(x, dm, group=G, slot=g(slot), shape=shape, sboxes=sb, cols=ct, sync=False)
        with pytest.raises(ValueError):
            ctx.sync()
        ctx.sync()                                       # reported once
        for i in range(N):
            c, t, f = good[i]
            if i in hit:
                assert np.isnan(float(out['score'][i])) and int(out['arg_flat'][i]) == -1
                if bad_slot is None:                     # its slot is in range: nothing was written there
                    assert np.isnan(float(out['det'][c, t, f])) and int(out['arg'][c, t, f]) == -1
                    assert bool(torch.isnan(out['tboxes'][c, t, f]).all())
            elif cols is None:
                assert torch.equal(out['det'][c, t, f], ref['det'][c, t, f]) and torch.equal(out['tboxes'][c, t, f], ref['tboxes'][c, t, f])
        assert int(torch.isnan(out['det']).sum()) == 12 - (N - len(hit))
        with pytest.raises(ValueError):
            ops.svm_head(x, dm, group=G, slot=g(slot), shape=shape, sboxes=sb, cols=ct)


def test_asynchronous_mode_gives_the_same_bytes():
    from vdetlib_amd import _lib, ops
    rng = np.random.RandomState(1300)
    N, G, K = 12, 5, 1024
    shape = (3, 2, 4)
    model = model_of(1301, K, 8, 'f64')
    dm = dev_model(model)
    x, slot, sb = g(rng.randn(N * G, K).astype(np.float32)), g(slots_of(1302, N, shape)), g(rng.uniform(1, 300, (N, G, 4)))
    a = ops.svm_head(x, dm, group=G, slot=slot, shape=shape, sboxes=sb)
    sa = ops.svm_scores(x[:7], dm)
    ctx = _lib.get_context(x.device.index)
    ctx.set_async(True)
    try:
        syncs = ctx.query(8)
        b = ops.svm_head(x, dm, group=G, slot=slot, shape=shape, sboxes=sb, sync=False)
        sbb = ops.svm_scores(x[:7], dm, sync=False)
        assert ctx.query(8) == syncs                     # no host wait inside the calls
        ctx.sync()
    finally:
        ctx.set_async(False)
    for k in ('det', 'arg', 'tboxes', 'score', 'arg_flat', 'nbad'):
        assert torch.equal(a[k].view(torch.uint8), b[k].view(torch.uint8)), k
    assert torch.equal(sa, sbb)


def test_host_checks():
    from vdetlib_amd import ops
    rng = np.random.RandomState(1400)
    N, G, K = 4, 2, 16
    shape = (2, 2, 2)
    model = model_of(1401, K, 4, 'f64')
    dm = dev_model(model)
    x = g(rng.randn(N * G, K).astype(np.float32))
    slot = g(slots_of(1402, N, shape))
    sb = g(rng.uniform(1, 300, (N, G, 4)))
    ok = ops.svm_head(x, dm, group=G, slot=slot, shape=shape, sboxes=sb)
    wide = dict(dm, W=g(np.zeros((K, 1))))
    bad = [lambda: ops.svm_head(x.cpu(), dm), lambda: ops.svm_head(x.int(), dm), lambda: ops.svm_head(x[:, :8], dm),
           lambda: ops.svm_head(x.t(), dm), lambda: ops.svm_head(x, dm, group=3), lambda: ops.svm_head(x, dm, group=0),
           lambda: ops.svm_head(x, dm, group=G, slot=slot), lambda: ops.svm_head(x, dm, group=G, slot=slot.long(), shape=shape),
           lambda: ops.svm_head(x, dm, group=G, slot=slot[:3], shape=shape), lambda: ops.svm_head(x, dm, group=G, shape=shape),
           lambda: ops.svm_head(x, dm, group=G, slot=slot, shape=shape, cols=g(np.zeros(3, np.int32))),
           lambda: ops.svm_head(x, dm, group=G, slot=slot, shape=shape, cols=g(np.zeros(2, np.int64))),
           lambda: ops.svm_head(x, dm, group=G, slot=slot, shape=shape, sboxes=sb.float()),
           lambda: ops.svm_head(x, dm, group=G, slot=slot, shape=shape, sboxes=sb[:, :1]),
           lambda: ops.svm_head(x, dm, group=G, slot=slot, shape=shape, ok=g(np.ones(N, np.uint8))),
           lambda: ops.svm_head(x, dm, group=G, slot=slot, shape=shape, count=g(np.array([2], np.int64))),
           lambda: ops.svm_head(x, dm, group=G, slot=slot, shape=(2, 2, 3), out=ok),
           lambda: ops.svm_head(x, dm, group=G, out=ok), lambda: ops.svm_head(x, wide, group=G, slot=slot, shape=shape),
           lambda: ops.svm_head(x, dict(dm, W=dm['W'].cpu()), group=G), lambda: ops.svm_head(x, dict(dm, W=dm['W'].half()), group=G),
           lambda: ops.svm_head(x, dict(dm, feat_norm_mean=np.ones(2)), group=G),
           lambda: ops.svm_scores(x.cpu(), dm), lambda: ops.svm_scores(x.half(), dm), lambda: ops.svm_scores(x[:, :8], dm)]
    for i, fn in enumerate(bad):
        with pytest.raises(ValueError):
            fn()
            pytest.fail("case %d did not raise" % i)


def test_svm_scores_on_device_tensors():
    from vdetlib_amd import ops
    from vdetlib_amd.vdet.image_det import svm_scores
    rng = np.random.RandomState(1500)
    for n, K, M, fdt, wdt in ((37, 1024, 200, 'f32', 'f64'), (5, 70, 13, 'f64', 'f64'), (66, 129, 65, 'f32', 'f32')):
        model = model_of(1501 + n, K, M, wdt)
        x = rng.randn(n, K).astype(NP_OF[fdt])
        want = svm_scores(x, model)
        got = ops.svm_scores(g(x), dev_model(model))
        same(got, want, '%d x %d x %d' % (n, K, M))
        got4 = ops.svm_scores(g(x)[:, :, None, None], model)                  # numpy model, [n,K,1,1] features
        assert torch.equal(got4, got)


# ---- the dict level against the reference's recorded outputs -----------------------------------------------------------

@functools.lru_cache(maxsize=None)
def golden():
    with gzip.open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'svmhead_golden.json.gz'), 'rt') as f:
        return json.load(f)


@pytest.mark.parametrize('which', [0, 1])
def test_dict_level_against_the_reference(which, monkeypatch):
    from vdetlib_amd.vdet import tubelet_cls as T
    case = golden()['cases'][which]
    K = case['K']
    vid, trp = ss.golden_protos(case)
    monkeypatch.setattr(T, 'imread', lambda path: int(os.path.splitext(os.path.basename(path))[0]) + 1)
    monkeypatch.setattr(T, 'svm_from_rcnn_model', lambda m: ss.golden_model(case['seed'], K))
    monkeypatch.setattr(T, 'googlenet_features', lambda img, boxes, net, layer: ss.golden_features(img, boxes, K))
    for class_idx in case['classes']:
        rec = case['plain'][str(class_idx)]
        tubs = T.rcnn_scoring(vid, trp, None, class_idx, None, save_feat=True, save_all_sc=True)
        assert len(tubs) == len(rec)
        for tub, r in zip(tubs, rec):
            assert [b['frame'] for b in tub['boxes']] == r['frame']
            assert [b['bbox'] for b in tub['boxes']] == r['bbox']
            np.testing.assert_allclose([b['det_score'] for b in tub['boxes']], r['det_score'], rtol=1e-9, atol=1e-9)
            for b in tub['boxes']:
                assert len(b['feat']) == K and len(b['all_score']) == 200
                assert abs(b['all_score'][T.index_vdet_to_det[class_idx] - 1] - b['det_score']) <= 1e-9 * (1 + abs(b['det_score']))
        rec = case['sampling'][str(class_idx)]
        np.random.seed(case['seed'])
        tubs = T.rcnn_sampling_scoring(vid, trp, None, class_idx, None, samples_per_box=case['samples_per_box'], save_all_sc=True)
        for tub, r in zip(tubs, rec):
            assert [b['frame'] for b in tub['boxes']] == r['frame']
            assert [b['bbox'] for b in tub['boxes']] == r['bbox']                # the winners: the reference's boxes, exactly
            np.testing.assert_allclose([b['det_score'] for b in tub['boxes']], r['det_score'], rtol=1e-9, atol=1e-9)
            assert all('feat' not in b and len(b['all_score']) == 200 for b in tub['boxes'])


def test_end_to_end_patches_to_head_to_rescore():
    """Anchor-route tubelets -> tubelet_patches (two frame ranges) -> a one-line torch 'net' -> svm_head through out= ->
    rescore_tubelets(floor=det), against svm_spec + rescore_spec on the same features."""
    import rescore_spec
    import synth
    from vdetlib_amd import ops
    F, B, C, T, S, p, K = 5, 40, 2, 3, 8, 2, 24
    boxes, scores = synth.coherent_video(77, F, B, C)
    imgs = np.random.RandomState(16).randint(0, 256, size=(F, synth.H, synth.W, 3)).astype(np.uint8)
    tb, ts, gi = g(boxes), g(scores), g(imgs)
    fr, ab, sc, _ = ops.top_anchors(tb, ts, T)
    tr, an, nt = ops.track_from_anchors(tb, fr, ab, sc)
    model = model_of(1700, K, 6, 'f64')
    dm = dev_model(model)
    cols = np.array([4, 1], np.int32)
    net = lambda patches: patches.reshape(patches.shape[0], -1)[:, :K * 8:8] * 0.01          # "pool5": K values per window
    out, feats, slots = None, [], []
    for f0, f1 in ((0, 2), (2, F)):
        po = ops.tubelet_patches(gi[f0:f1], tr, nt, (f0, f1), C * T * (f1 - f0), crop_size=S, padding=p, sync=False)
        feat = net(po['patches']).contiguous()
        out = ops.svm_head(feat, dm, slot=po['slot'], count=po['count'], shape=None if out else (C, T, F), cols=g(cols), ok=po['ok'],
                           out=out)
        n = int(po['count'])
        feats.append(feat[:n].cpu().numpy())
        slots.append(po['slot'][:n].cpu().numpy())
        assert not po['ok'][:n].eq(0).any()
    det = out['det']
    assert det.dtype == torch.float64 and int(out['nbad']) == 0
    want = ss.head(np.concatenate(feats), model['W'], model['B'], scale_of(model, np.float64), np.float64, slot=np.concatenate(slots),
                   shape=(C, T, F), cols=cols)
    assert len(want['score']) > F
    same(det, want['det'])
    same(out['arg'], want['arg'])
    got = ops.rescore_tubelets(tr, nt, tb, ts, floor=det)
    w = rescore_spec.spec(tr.cpu().numpy(), nt.cpu().numpy(), boxes, scores, floor=want['det'])
    assert not w[4]
    for a, b in zip(got, w[:4]):
        assert np.array_equal(a.cpu().numpy(), b, equal_nan=True)
