"""CPU-only: the numpy statement of the SVM head (tests/svm_spec.py) against the reference's recorded outputs and against
np.dot + argmax, its argmax rules, and the C-ABI / dict-level surface of the device form (vdet_svm_head, vdet_svm_scores_dev)."""
import ctypes
import gzip
import json
import os
import re

import numpy as np
import pytest

import svm_spec as ss

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = dict(rtol=1e-9, atol=1e-9)          # the project's f64 bar for this product (test_svm_scores_matches_numpy)


@pytest.fixture(scope='module')
def golden():
    with gzip.open(os.path.join(ROOT, 'tests', 'golden', 'svmhead_golden.json.gz'), 'rt') as f:
        return json.load(f)['cases']


def _frame_boxes(trp, frame_id):
    """(tubelet index, bbox) of the tubelets that have a box in the frame, in tubelet order -- the reference's frame loop."""
    return [(t, b['bbox']) for t, tr in enumerate(trp['tracks']) for b in tr if b['frame'] == frame_id]


def test_fixture_shape(golden):
    assert [c['samples_per_box'] for c in golden] == [4, 32] and all(c['classes'] == [1, 7] and c['K'] == 40 for c in golden)
    for case in golden:
        _, trp = ss.golden_protos(case)
        assert any(len(tr) < case['F'] for tr in trp['tracks'])                  # holes
        for mode in ('plain', 'sampling'):
            for cls in ('1', '7'):
                assert [r['frame'] for r in case[mode][cls]] == [[b['frame'] for b in tr] for tr in trp['tracks']]
        args = [a for cls in ('1', '7') for r in case['sampling'][cls] for a in r['arg']]
        assert len(set(args)) > 2 and max(args) <= case['samples_per_box']       # the winners are not all the box itself


@pytest.mark.parametrize('which', [0, 1])
def test_spec_against_the_reference(golden, which):
    """Features rebuilt from the seeds, offsets redrawn from numpy's legacy stream in the reference's order: svm_spec picks the
    reference's winners and boxes exactly and its scores within the bar."""
    from vdetlib_amd.vdet.dataset import index_vdet_to_det
    from vdetlib_amd.vdet.tubelet_cls import sampling_boxes
    case = golden[which]
    K, G = case['K'], case['samples_per_box'] + 1
    vid, trp = ss.golden_protos(case)
    model = ss.golden_model(case['seed'], K)
    scale = float(20. / model['feat_norm_mean'])
    for class_idx in case['classes']:
        cols = np.array([index_vdet_to_det[class_idx] - 1], np.int32)
        plain = {(t, f): (s, b) for t, r in enumerate(case['plain'][str(class_idx)])
                 for f, s, b in zip(r['frame'], r['det_score'], r['bbox'])}
        samp = {(t, f): (s, b, a) for t, r in enumerate(case['sampling'][str(class_idx)])
                for f, s, b, a in zip(r['frame'], r['det_score'], r['bbox'], r['arg'])}
        np.random.seed(case['seed'])
        for frame in vid['frames']:
            fid = frame['frame']
            here = _frame_boxes(trp, fid)
            if not here:
                continue
            boxes = np.asarray([b for _, b in here])
            out = ss.head(ss.golden_features(fid, boxes, K), model['W'], model['B'], scale, np.float64, cols=cols)
            np.testing.assert_allclose(out['score'], [plain[(t, fid)][0] for t, _ in here], **BAR)
            assert [plain[(t, fid)][1] for t, _ in here] == boxes.tolist()
            sampled = np.vstack([sampling_boxes(b, G - 1, 0.05) for b in boxes])                # the reference's draws, redrawn
            out = ss.head(ss.golden_features(fid, sampled, K), model['W'], model['B'], scale, np.float64, group=G, cols=cols,
                          sboxes=sampled.reshape(len(here), G, 4))
            assert out['arg_flat'].tolist() == [samp[(t, fid)][2] for t, _ in here]
            assert out['tboxes'].tolist() == [samp[(t, fid)][1] for t, _ in here]
            np.testing.assert_allclose(out['score'], [samp[(t, fid)][0] for t, _ in here], **BAR)


def test_sampling_boxes_is_the_reference_line_for_line():
    from vdetlib_amd.vdet.tubelet_cls import sampling_boxes
    box = np.array([10., 20., 30., 60.])
    np.random.seed(5)
    got = sampling_boxes(box, 3, 0.1)
    np.random.seed(5)
    off = np.random.uniform(-0.1, 0.1, [3, 4]) * [20., 40., 20., 40.]
    assert got.shape == (4, 4) and np.array_equal(got[0], box) and np.array_equal(got[1:], box + off)
    np.random.seed(5)
    assert np.array_equal(sampling_boxes(box, 3, 0.1, return_orig=False), box + off)
    assert np.abs(got[1:] - box).max() <= 0.1 * 40


@pytest.mark.parametrize('cdt', [np.float64, np.float32])
def test_spec_against_numpy_dot(cdt):
    rng = np.random.RandomState(1)
    # f32: a term passes at most 8*3 + 6 + 1 additions and two products, each within 2^-24 relative, and the terms' absolute
    # sum stays below 1100 * E|x| * 1.03 * E|w| ~ 1100 * 0.8 * 1.03 * 0.5 < 600: 33 * 2^-24 * 600 = 1.2e-3
    bar = BAR if cdt == np.float64 else dict(rtol=0, atol=1.2e-3)
    for K, M, N, G in ((1, 3, 4, 2), (7, 5, 6, 3), (64, 9, 5, 4), (513, 4, 3, 5), (1024, 200, 4, 33), (1100, 6, 2, 2)):
        W, B = rng.uniform(-1, 1, (K, M)).astype(cdt), rng.uniform(-1, 1, M).astype(cdt)
        x = rng.randn(N * G, K).astype(np.float32)
        shape = (M, 2, N)
        slot = np.stack([rng.randint(0, M, N), rng.randint(0, 2, N), np.arange(N)], 1).astype(np.int32)
        sb = rng.uniform(0, 100, (N, G, 4))
        out = ss.head(x, W, B, 1.03, cdt, group=G, slot=slot, shape=shape, sboxes=sb)
        full = np.dot(x.astype(np.float64) * 1.03, W.astype(np.float64)) + B
        s = full[np.arange(N * G), np.repeat(slot[:, 0], G)].reshape(N, G)
        assert out['score'].dtype == cdt and out['det'].dtype == cdt
        np.testing.assert_allclose(out['windows'].reshape(N, G), s, **bar)
        np.testing.assert_allclose(out['score'], s.max(1), **bar)
        if cdt == np.float64:
            assert np.array_equal(out['arg_flat'], np.argmax(s, 1))
        assert np.array_equal(out['arg_flat'], np.argmax(out['windows'].reshape(N, G), 1))
        for g in range(N):
            c, t, f = slot[g]
            assert out['det'][c, t, f] == out['score'][g] and out['arg'][c, t, f] == out['arg_flat'][g]
            assert np.array_equal(out['tboxes'][c, t, f], sb[g, out['arg_flat'][g]])
        assert np.isnan(out['det']).sum() == M * 2 * N - N and (out['arg'] == -1).sum() == M * 2 * N - N


def test_spec_order_is_the_written_one():
    """K = 1024 by hand for one window: lanes, ascending k inside a lane, the butterfly."""
    rng = np.random.RandomState(2)
    K = 1024
    x, w = rng.randn(K).astype(np.float32), rng.uniform(-1, 1, K)
    scale = 1.0371
    acc = [0.0] * 64
    for lane in range(64):
        for r in range(2):
            for i in range(8):
                k = (r * 64 + lane) * 8 + i
                acc[lane] = acc[lane] + (float(x[k]) * scale) * w[k]
    for d in (32, 16, 8, 4, 2, 1):
        acc = [acc[lane] + acc[lane ^ d] for lane in range(64)]
    got = ss.window_scores(x[None], w[:, None], np.array([0.25]), scale, [0], np.float64)
    assert got[0] == acc[0] + 0.25 and len(set(acc)) == 1
    # storage does not change the order: f16 values as f16, f32 and f64
    h = x.astype(np.float16)
    a = [ss.window_scores(h.astype(dt)[None], w[:, None], None, scale, [0], np.float64)[0] for dt in (np.float16, np.float32, np.float64)]
    assert a[0] == a[1] == a[2]
    b = ss.window_scores(ss.to_bf16(x)[None], w[:, None], None, scale, [0], np.float64)[0]
    assert b == ss.window_scores(ss.widen(ss.to_bf16(x), np.float32)[None], w[:, None], None, scale, [0], np.float64)[0]


def test_argmax_rules():
    nan = float('nan')
    for s in ([1.0, 3.0, 3.0, 2.0], [5.0], [2.0, 2.0], [1.0, nan, 7.0, nan], [nan, 1.0], [-np.inf, -np.inf], [1.0, np.inf, nan],
              [-0.0, 0.0], [0.0, -0.0]):
        best, arg = ss.argmax_first(s)
        assert arg == int(np.argmax(s)) and (best == s[arg] or (np.isnan(best) and np.isnan(s[arg]))), s
    # planted in a head call: ties (equal windows), a NaN, a masked winner, a box with no window
    rng = np.random.RandomState(3)
    K, G = 16, 4
    W, B = rng.uniform(-1, 1, (K, 2)), np.zeros(2)
    x = rng.randn(5, G, K)
    x[0, 2] = x[0, 0] = x[0, 3]                                             # windows 0, 2, 3 equal
    x[1, 2, 4] = nan
    ok = np.ones((5, G), np.uint8)
    out0 = ss.head(x.reshape(-1, K), W, B, 1.0, np.float64, group=G)
    ok[2, out0['arg_flat'][2]] = 0                                          # the winner of box 2 may not compete
    ok[3] = 0
    out = ss.head(x.reshape(-1, K), W, B, 1.0, np.float64, group=G, ok=ok)
    w = out0['windows'].reshape(5, G)
    assert out['arg_flat'][0] == (0 if w[0, 0] >= w[0, 1] else 1)
    assert out['arg_flat'][1] == 2 and np.isnan(out['score'][1])
    assert out['arg_flat'][2] != out0['arg_flat'][2] and out['score'][2] == np.sort(w[2])[-2]
    assert out['arg_flat'][3] == -1 and np.isnan(out['score'][3]) and out['nbad'] == 1
    assert out['arg_flat'][4] == out0['arg_flat'][4] == np.argmax(w[4])
    # count, and the groups the device refuses
    slot = np.array([[0, 0, 0], [1, 0, 1], [0, 0, 2], [2, 0, 0], [-1, -1, -1]], np.int32)
    out = ss.head(x.reshape(-1, K), W, B, 1.0, np.float64, group=G, slot=slot, shape=(2, 1, 3), count=4)
    assert out['bad'] == [3] and np.isnan(out['score'][3:]).all() and (~np.isnan(out['score'][[0, 2]])).all()      # (box 1 holds the NaN)
    out = ss.head(x.reshape(-1, K), W, B, 1.0, np.float64, group=G, slot=slot, shape=(2, 1, 3), count=3, cols=[1, 2])
    assert out['bad'] == [1] and np.isnan(out['det'][1, 0, 1])


def test_svm_from_rcnn_model(tmp_path):
    import scipy.io as sio
    from vdetlib_amd.utils.common import svm_from_rcnn_model
    rng = np.random.RandomState(4)
    W, B = rng.randn(12, 5), rng.randn(1, 5)
    path = str(tmp_path / 'rcnn_model.mat')
    sio.savemat(path, {'rcnn_model': {'detectors': {'W': W, 'B': B}, 'training_opts': {'feat_norm_mean': 19.5, 'other': 3.0}}})
    svm = svm_from_rcnn_model(path)
    assert set(svm) == {'W', 'B', 'feat_norm_mean'}
    assert np.array_equal(svm['W'], W) and np.array_equal(svm['B'], B) and svm['W'].dtype == np.float64
    assert svm['feat_norm_mean'] == 19.5 and np.ndim(svm['feat_norm_mean']) == 0
    assert np.result_type(np.zeros(1, np.float32) * (20. / svm['feat_norm_mean'])) == np.float64        # the .mat models compute in f64


# ---- the C-ABI and the dict level ------------------------------------------------------------------------------------------

def _prototype(name):
    src = open(os.path.join(ROOT, 'include', 'vdet_hip.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    m = re.search(r'\bint\s+%s\s*\(([^;]*?)\)\s*;' % name, src, flags=re.S)
    assert m, "%s is not declared in include/vdet_hip.h" % name
    return [re.sub(r'\s+', ' ', a).strip() for a in m.group(1).split(',')]


def _ctype_of(arg):
    if '*' in arg:
        return ctypes.c_void_p
    return {'int': ctypes.c_int, 'int64_t': ctypes.c_int64, 'double': ctypes.c_double, 'float': ctypes.c_float}[arg.split()[-2]]


def test_header_prototypes_and_symbol_rows():
    from vdetlib_amd import _lib
    hp = _prototype('vdet_svm_head')
    assert [a.split()[-1].lstrip('*') for a in hp] == ['ctx', 'd_feat', 'feat_dtype', 'N', 'G', 'K', 'd_W', 'w_f64', 'd_B', 'b_f64', 'M',
                                                       'scale', 'compute_f64', 'd_slot', 'd_count', 'C', 'T', 'F', 'd_cols', 'd_sboxes',
                                                       'd_ok', 'd_det', 'd_arg', 'd_tboxes', 'd_score', 'd_arg_flat', 'd_nbad']
    protos = [('vdet_svm_head', hp)]
    for name in ('vdet_svm_scores_dev_f64', 'vdet_svm_scores_dev_f32'):
        p = _prototype(name)
        assert [a.split()[-1].lstrip('*') for a in p] == ['ctx', 'd_feat', 'n', 'k', 'd_W', 'd_B', 'm', 'd_out']
        protos.append((name, p))
    for name, proto in protos:
        res, args = _lib.SYMBOLS[name]
        assert res is ctypes.c_int
        assert args == [_ctype_of(a) for a in proto], name
    src = open(os.path.join(ROOT, 'include', 'vdet_hip.h')).read()
    assert [int(re.search(r'#define VDET_FEAT_%s (\d)' % n, src).group(1)) for n in ('F32', 'F16', 'BF16', 'F64')] == [0, 1, 2, 3]


def test_null_context_refused():
    from vdetlib_amd import _lib
    L = _lib.load_library()
    z = None
    assert L.vdet_svm_head(z, z, 0, 1, 1, 8, z, 1, z, 1, 4, 1.0, 1, z, z, 1, 1, 1, z, z, z, z, z, z, z, z, z) == _lib.VDET_EINVAL
    assert L.vdet_svm_scores_dev_f64(z, z, 1, 1, z, z, 1, z) == _lib.VDET_EINVAL
    assert L.vdet_svm_scores_dev_f32(z, z, 1, 1, z, z, 1, z) == _lib.VDET_EINVAL


def test_dict_level_needs_gpu(monkeypatch):
    """Without a GPU the dict level raises -- there is no CPU fallback."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from vdetlib_amd.vdet import tubelet_cls as T
    case = dict(seed=1, F=2, T=1)
    vid, trp = ss.golden_protos(case)
    trp['tracks'] = [[{'frame': 1, 'bbox': [3., 3., 9., 9.], 'score': 0.5, 'anchor': 0}]]
    monkeypatch.setattr(T, 'imread', lambda path: np.zeros((20, 20, 3), np.uint8))
    monkeypatch.setattr(T, 'svm_from_rcnn_model', lambda m: ss.golden_model(1, 8))
    with pytest.raises(RuntimeError):
        T.rcnn_scoring(vid, trp, object(), 1, None)
    monkeypatch.setattr(T, 'googlenet_features', lambda img, boxes, net, layer: ss.golden_features(1, boxes, 8))
    with pytest.raises(RuntimeError):
        T.rcnn_sampling_scoring(vid, trp, object(), 1, None, samples_per_box=2)
