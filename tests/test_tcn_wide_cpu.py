"""CPU-only: the statement of the device TCN's wide first layer (tests/tcn_wide_spec.py), the C-ABI rows of
vdet_tcn_tracks_wide[_batch], and score_conv_cls_batched's layout of per-box rows."""
import contextlib
import ctypes
import io
import os
import re

import numpy as np
import pytest

import tcn_wide_spec as ws

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def test_spec_by_hand_two_boxes_three_channels_k3():
    """One one-channel input around a two-channel wide blob; rows of three frames, the tubelet has boxes on frames 0 and 2."""
    inputs = [('det_scores', 1), ('all_scores', 2)]
    rows = np.array([[1.5, -2.0], [99.0, 99.0], [0.25, 4.0]], np.float32)            # frame 1 is a hole: never read
    x = ws.concat_inputs(inputs, {'det_scores': [0.5, -1.0]}, {'all_scores': rows}, [0, 2])
    assert x.dtype == np.float32 and np.array_equal(x, np.array([[0.5, -1.0], [1.5, 0.25], [-2.0, 4.0]], np.float32))
    w = np.array([[[0.1, 0.2, 0.3], [-0.4, 0.5, 0.6], [0.7, -0.8, 0.9]]], np.float32)  # [1, 3, 3]
    b = np.array([0.05], np.float32)
    # position 0 sees (pad, x0, x1), position 1 sees (x0, x1, pad); the padded products are added as w * 0
    want = []
    for taps in ([(0.0, 0.5, -1.0), (0.0, 1.5, 0.25), (0.0, -2.0, 4.0)], [(0.5, -1.0, 0.0), (1.5, 0.25, 0.0), (-2.0, 4.0, 0.0)]):
        acc = f32(b[0])
        for ci in range(3):
            for k in range(3):
                acc = f32(acc + f32(w[0, ci, k] * f32(taps[ci][k])))
        want.append(acc)
    got = ws.layer0(x, w, b, relu=False)
    assert got.shape == (1, 2) and got[0, 0] == want[0] and got[0, 1] == want[1]
    assert np.array_equal(ws.layer0(x, w, b, relu=True), np.maximum(got, 0))
    # the padded product is ADDED: an infinite weight on a padded tap makes the sum NaN (inf * 0), it is not skipped
    w_inf = w.copy()
    w_inf[0, 0, 0] = np.inf
    got_inf = ws.layer0(x, w_inf, b, relu=False)
    assert np.isnan(got_inf[0, 0]) and np.isinf(got_inf[0, 1])


@pytest.mark.parametrize("cin,cout,K,L", [(3, 2, 1, 1), (9, 5, 3, 2), (200, 4, 5, 17), (65, 3, 7, 40)])
def test_spec_against_f64_within_the_recursive_summation_bound(cin, cout, K, L):
    """|f32 chain - exact| <= (K*Cin + 1) * 2^-23 * (|b| + sum |w*x|) per output: K*Cin products (2^-24 each) and K*Cin sums
    (at most K*Cin * 2^-24 relative each on the running magnitude), first order, doubled for the higher orders."""
    rng = np.random.RandomState(cin + K)
    x = rng.randn(cin, L).astype(np.float32)
    w = (rng.randn(cout, cin, K) / np.sqrt(cin * K)).astype(np.float32)
    b = (0.1 * rng.randn(cout)).astype(np.float32)
    got = ws.layer0(x, w, b, relu=False).astype(np.float64)
    val, mag = ws.layer0_f64(x, w, b)
    bound = (K * cin + 1) * 2.0 ** -23 * mag
    err = np.abs(got - val)
    print("Cin %d K %d: worst error / bound = %.3g" % (cin, K, float((err / bound).max())))
    assert (err <= bound).all()


def test_f64_rows_round_once():
    up = np.float64(1.0) + 2.0 ** -24 + 2.0 ** -40          # above the midpoint of 1 and 1 + 2^-23: rounds UP
    assert ws.widen_rows(np.array([up]))[0] == f32(1.0) + f32(2.0 ** -23)
    assert ws.widen_rows(np.array([1.0 + 2.0 ** -25]))[0] == f32(1.0)


# ---- the C-ABI ---------------------------------------------------------------------------------------------------------------

def _prototype(name):
    src = open(os.path.join(ROOT, 'include', 'vdet_hip.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    m = re.search(r'\bint\s+%s\s*\(([^;]*?)\)\s*;' % name, src, flags=re.S)
    assert m, "%s is not declared in include/vdet_hip.h" % name
    return [re.sub(r'\s+', ' ', a).strip() for a in m.group(1).split(',')]


def _ctype_of(arg):
    if '*' in arg:
        return ctypes.c_void_p
    return {'int': ctypes.c_int, 'int64_t': ctypes.c_int64}[arg.split()[-2]]


WIDE_ARGS = ['h_codes', 'h_widths', 'h_rows', 'h_dtypes', 'n_inputs']


def test_header_prototypes_and_symbol_rows():
    """The wide entry points take the arguments of vdet_tcn_tracks[_batch] with (h_channels, n_channels) replaced by the
    per-input code, width, row pointer and dtype tables."""
    from vdetlib_amd import _lib
    for name in ('vdet_tcn_tracks', 'vdet_tcn_tracks_batch'):
        narrow = [a.split()[-1].lstrip('*') for a in _prototype(name)]
        wide_name = name.replace('vdet_tcn_tracks', 'vdet_tcn_tracks_wide')
        proto = _prototype(wide_name)
        i = narrow.index('h_channels')
        assert [a.split()[-1].lstrip('*') for a in proto] == narrow[:i] + WIDE_ARGS + narrow[i + 2:]
        assert wide_name in _lib.SYMBOLS, wide_name
        res, args = _lib.SYMBOLS[wide_name]
        assert res is ctypes.c_int and args == [_ctype_of(a) for a in proto]


def test_null_context_refused():
    from vdetlib_amd import _lib
    L = _lib.load_library()
    z = None
    assert L.vdet_tcn_tracks_wide(z, z, z, 1, z, z, z, z, 1, 4, 1, 1, z, z, z, z, 1, z, z) == _lib.VDET_EINVAL
    assert L.vdet_tcn_tracks_wide_batch(z, z, z, 1, z, z, z, z, 1, z, 1, 1, 1, z, z, z, z, 1, z, z) == _lib.VDET_EINVAL


def test_device_inputs_of_a_net():
    from vdetlib_amd.vdet.tcn import TCNNet
    net = TCNNet.random([('all_scores', 3), ('det_scores', 1), ('feats', 5), ('labels', 1)], hidden=(4,))
    assert net.device_inputs({'all_scores': 0, 'feats': 0}) == [(-1, 3), (0, 1), (-1, 5), (5, 1)]
    with pytest.raises(ValueError):
        net.device_channels()                                   # the narrow call still refuses the net
    for bad in ({'all_scores': 0}, {'all_scores': 0, 'feats': 0, 'det_scores': 0}, {'all_scores': 0, 'feats': 0, 'other': 0}):
        with pytest.raises(ValueError):
            net.device_inputs(bad)
    with pytest.raises(ValueError):
        TCNNet.random([('det_scores', 2)], hidden=(4,)).device_inputs({})
    with pytest.raises(ValueError):
        TCNNet.random([('a%d' % i, 1) for i in range(17)], hidden=(2,)).device_inputs({'a%d' % i: 0 for i in range(17)})
    with pytest.raises(ValueError):
        TCNNet.random([('feats', 4097)], hidden=()).device_inputs({'feats': 0})
    with pytest.raises(ValueError):
        TCNNet.random([('feats', 4096), ('det_scores', 1)], hidden=()).device_inputs({'feats': 0})


# ---- the dict level ----------------------------------------------------------------------------------------------------------

def _proto(lengths, widths):
    rng = np.random.RandomState(3)
    tubs = []
    for n in lengths:
        boxes = []
        for j in range(n):
            box = {'frame': j + 1, 'det_score': float(rng.rand()), 'track_score': float(rng.rand()), 'gt_overlap': 0.0,
                   'anchor': j - 1, 'bbox': [0, 0, 4, 4]}
            for key, wd in widths.items():
                box[key] = rng.randn(wd).tolist()
            boxes.append(box)
        tubs.append({'gt': 0, 'boxes': boxes})
    return {'video': 'v', 'method': 'm', 'tubelets': tubs}


def test_score_conv_cls_batched_transposes_per_box_rows(monkeypatch):
    from vdetlib_amd.vdet import tubelet_cls as TC
    from vdetlib_amd.vdet.tcn import TCNNet
    proto = _proto([4, 1, 3], {'all_score': 3, 'feat': 2})
    net = TCNNet.random([('all_scores', 3), ('det_scores', 1), ('feats', 2)], hidden=(4,))
    seen = []

    def stub(self, series, ctx=None):
        seen.extend(series)
        return [np.full(s.shape[1], 0.25, np.float32) for s in series]
    monkeypatch.setattr(TCNNet, 'forward_series', stub)
    with contextlib.redirect_stdout(io.StringIO()):
        out = TC.score_conv_cls_batched(proto, net)
    assert len(seen) == 3
    for tub, x in zip(proto['tubelets'], seen):
        n = len(tub['boxes'])
        assert x.shape == (6, n) and x.dtype == np.float32 and x.flags['C_CONTIGUOUS']
        for j, box in enumerate(tub['boxes']):
            want = np.array(box['all_score'] + [box['det_score']] + box['feat'], dtype=np.float32)
            assert np.array_equal(x[:, j], want)               # channel q at position j = entry q of box j
        assert all(b['conv_score'] == 0.25 for b in tub['boxes'])
    assert out['tubelets'] is proto['tubelets']
    # a blob whose channel count is not the rows' width is refused, not reshaped
    bad = TCNNet.random([('all_scores', 2), ('det_scores', 1)], hidden=(4,))
    with pytest.raises(ValueError), contextlib.redirect_stdout(io.StringIO()):
        TC.score_conv_cls_batched(_proto([6], {'all_score': 3}), bad)
    # score_conv_cls keeps the reference's behaviour for wide blobs: numpy cannot broadcast [L, ch] into (1, ch, 1, L)
    monkeypatch.undo()
    with pytest.raises(ValueError), contextlib.redirect_stdout(io.StringIO()):
        TC.score_conv_cls(_proto([4], {'all_score': 3, 'feat': 2}), net)


def test_one_channel_nets_are_laid_out_as_before(monkeypatch):
    from vdetlib_amd.vdet import tubelet_cls as TC
    from vdetlib_amd.vdet.tcn import TCNNet
    proto = _proto([5, 2], {})
    net = TCNNet.random([('det_scores', 1), ('anchors', 1), ('track_scores', 1)], hidden=(4,))
    seen = []
    monkeypatch.setattr(TCNNet, 'forward_series', lambda self, series, ctx=None: seen.extend(series) or
                        [np.zeros(s.shape[1], np.float32) for s in series])
    with contextlib.redirect_stdout(io.StringIO()):
        TC.score_conv_cls_batched(proto, net)
    for tub, x in zip(proto['tubelets'], seen):
        n = len(tub['boxes'])
        want = np.stack([np.asarray([b['det_score'] for b in tub['boxes']], dtype='float32'),
                         (np.asarray([b['anchor'] for b in tub['boxes']], dtype=np.float64) / n).astype(np.float32),
                         np.asarray([b['track_score'] for b in tub['boxes']], dtype='float32')], 0)
        assert np.array_equal(x, want)
