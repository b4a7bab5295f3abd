"""CPU: the device merge of tubelet sets above and below the C-ABI, as far as it goes without a device -- the two symbols and
their prototypes, the argument checks that start no device work, the ops signatures and every ValueError of
ops.merge_tracks / ops.merge_tracks_batch -- and the converter between tubelet-set arrays and score-proto dicts that
test_merge_tracks_gpu.py uses to run `utils.protocol.merge_score_protos` (pinned to the reference's recorded outputs by
test_protocol_cpu.py) as the executable specification."""
import copy
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

# ---- arrays <-> score protos ---------------------------------------------------------------------------------------------
# A set is a dict of numpy arrays: tracks [C,T,F,5] f32, ntracks [C] i32, anchors [C,T,3] f32, series (tuple of [C,T,F] f64),
# optionally tboxes [C,T,F,4] f32.  Class c becomes one score proto; slot t < ntracks[c] one tubelet; a row whose column 0 is
# not NaN one box with frame, bbox, det_score (series 0), track_score (row column 4), anchor (frame - anchor frame), tbox, and
# series q >= 1 under the key extra[q - 1] (the golden protos keep their f64 track_score that way).  f32 values travel as
# python floats (exact both ways).  'src' tags the side a box's values come from: `merge_score_protos` copies every key of
# a's box from b's, the tag included, which is how the expected from_b is read off the mirror.


def blank_set(C, T, F, nser, tboxes):
    s = dict(tracks=np.full((C, T, F, 5), np.nan, np.float32), ntracks=np.zeros((C,), np.int32),
             anchors=np.zeros((C, T, 3), np.float32), series=tuple(np.full((C, T, F), np.nan, np.float64) for _ in range(nser)))
    if tboxes:
        s['tboxes'] = np.full((C, T, F, 4), np.nan, np.float32)
    return s


def copy_set(s):
    out = {k: (tuple(x.copy() for x in v) if k == 'series' else v.copy()) for k, v in s.items() if k != 'from_b'}
    return out


def set_to_protos(s, video='v', method='m', extra=(), src='a', hashes=None):
    C, T, F = s['tracks'].shape[:3]
    protos = []
    for c in range(C):
        tubs = []
        for t in range(int(s['ntracks'][c])):
            af = int(s['anchors'][c, t, 0])
            boxes = []
            for f in range(F):
                row = s['tracks'][c, t, f]
                if np.isnan(row[0]):
                    continue
                box = {'frame': f + 1, 'bbox': [float(v) for v in row[:4]], 'det_score': float(s['series'][0][c, t, f]),
                       'track_score': float(row[4]), 'anchor': f + 1 - af, 'src': src}
                if 'tboxes' in s:
                    box['tbox'] = [float(v) for v in s['tboxes'][c, t, f]]
                for q, key in enumerate(extra):
                    box[key] = float(s['series'][q + 1][c, t, f])
                if hashes is not None:
                    box['hash'] = hashes[(f + 1, tuple(int(v) for v in row[:4]))]
                boxes.append(box)
            tubs.append({'class_index': c + 1, 'class': 'class%d' % (c + 1), 'gt': 0, 'boxes': boxes,
                         'anchor_row': [float(v) for v in s['anchors'][c, t]]})
        protos.append({'video': video, 'method': method, 'tubelets': tubs})
    return protos


def protos_into_set(protos, base, extra=()):
    """Write the tubelets of one proto per class over `base` (a set of the output's shape): the boxes, the anchors and the
    counts; what a proto does not carry (dead slots, frames without a box) stays as `base` has it.  Returns (set, from_b)."""
    out = copy_set(base)
    C, T, F = out['tracks'].shape[:3]
    from_b = np.zeros((C, T, F), np.uint8)
    for c, proto in enumerate(protos):
        out['ntracks'][c] = len(proto['tubelets'])
        for t, tub in enumerate(proto['tubelets']):
            if 'anchor_row' in tub:
                out['anchors'][c, t] = tub['anchor_row']
            elif tub['boxes']:
                out['anchors'][c, t] = (tub['boxes'][0]['frame'] - tub['boxes'][0]['anchor'], -1, 0)
            for box in tub['boxes']:
                f = box['frame'] - 1
                out['tracks'][c, t, f, :4] = box['bbox']
                out['tracks'][c, t, f, 4] = box['track_score']
                out['series'][0][c, t, f] = box['det_score']
                if 'tboxes' in out:
                    out['tboxes'][c, t, f] = box['tbox']
                for q, key in enumerate(extra):
                    out['series'][q + 1][c, t, f] = box[key]
                from_b[c, t, f] = box.get('src') == 'b'
    return out, from_b


def golden_set(proto, T=None, F=6):
    """One golden score proto (one class) as a set: series = (det_score, the f64 track_score); its hashes by (frame, bbox)."""
    n = len(proto['tubelets'])
    base = blank_set(1, n if T is None else T, F, 2, False)
    s, _ = protos_into_set([proto], base, extra=('track_score',))
    hashes = {(b['frame'], tuple(b['bbox'])): b['hash'] for t in proto['tubelets'] for b in t['boxes']}
    return s, hashes


def same_bits(x, y):
    """bit for bit, a NaN equal to any NaN"""
    x, y = np.asarray(x), np.asarray(y)
    if x.shape != y.shape or x.dtype != y.dtype:
        return False
    if x.dtype.kind != 'f':
        return bool(np.array_equal(x, y))
    iv = {4: np.uint32, 8: np.uint64}[x.dtype.itemsize]
    return bool(np.all((x.view(iv) == y.view(iv)) | (np.isnan(x) & np.isnan(y))))


def sets_equal(x, y):
    keys = sorted(k for k in x if k != 'from_b')
    if keys != sorted(k for k in y if k != 'from_b') or len(x['series']) != len(y['series']):
        return False
    return all(same_bits(x[k], y[k]) for k in keys if k != 'series') and all(same_bits(p, q) for p, q in zip(x['series'], y['series']))


def mirror(a, b, scheme, extra=None):
    """`merge_score_protos` on the protos of two sets -> (expected set, expected from_b).  'max' starts from a's arrays (what
    the protos do not carry is a's), 'combine' from NaN rows and zero anchors."""
    from vdetlib_amd.utils import protocol as P
    extra = tuple('s%d' % q for q in range(1, len(a['series']))) if extra is None else extra
    pa, pb = set_to_protos(a, extra=extra, src='a'), set_to_protos(b, extra=extra, src='b')
    merged = [P.merge_score_protos(x, y, scheme) for x, y in zip(pa, pb)]
    C, Ta, F = a['tracks'].shape[:3]
    base = copy_set(a) if scheme == 'max' else blank_set(C, Ta + b['tracks'].shape[1], F, len(a['series']), 'tboxes' in a)
    return protos_into_set(merged, base, extra=extra)


# ---- tests ---------------------------------------------------------------------------------------------------------------

def _strip(proto, keys=('anchor_row',), box_keys=('src',)):
    p = copy.deepcopy(proto)
    for t in p['tubelets']:
        for k in keys:
            t.pop(k, None)
        for b in t['boxes']:
            for k in box_keys:
                b.pop(k, None)
    return p


def test_converter_round_trips_the_golden_protos(proto_golden):
    from vdetlib_amd.utils import protocol as P
    g = proto_golden['protocol_misc']
    a, b = proto_golden['spatial_maxpool']['dets_c1_0.7'], proto_golden['temporal_maxpool']['w3']
    for proto in (a, b, g['merge_max'], g['merge_combine']):
        s, hashes = golden_set(proto)
        assert s['tracks'].shape == (1, len(proto['tubelets']), 6, 5) and int(s['ntracks'][0]) == len(proto['tubelets'])
        back = set_to_protos(s, video=proto['video'], method=proto['method'], extra=('track_score',), hashes=hashes)[0]
        for t, tub in zip(back['tubelets'], proto['tubelets']):
            t['class'] = tub['class']
        assert _strip(back) == proto
        again, _ = protos_into_set([back], blank_set(1, len(proto['tubelets']), 6, 2, False), extra=('track_score',))
        assert sets_equal(again, s)
    # ... and the mirror on the converted golden pair is the reference's recorded merge, both schemes
    sa, sb = golden_set(a)[0], golden_set(b)[0]
    for scheme in ('max', 'combine'):
        want, from_b = mirror(sa, sb, scheme, extra=('track_score',))
        assert sets_equal(want, golden_set(g['merge_' + scheme])[0])
        if scheme == 'max':
            assert from_b.sum() == np.sum(sb['series'][0] > sa['series'][0]) > 0
    assert P.merge_score_protos(copy.deepcopy(a), copy.deepcopy(b), 'max') == g['merge_max']


def test_symbols_and_prototypes():
    from vdetlib_amd import _lib
    L = _lib.load_library()
    vp, ci, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    sets_and_out = [vp] * 8 + [vp, vp, ci] + [vp] * 6       # a (4), b (4), h_series_a, h_series_b, n_series, outputs (5), from_b
    want = {"vdet_merge_tracks": [vp, ci, i64, i64, ci, ci] + sets_and_out,
            "vdet_merge_tracks_batch": [vp, ci, vp, i64, i64, ci, ci] + sets_and_out}
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'vdet_hip.h')).read()
    header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    for name, args in want.items():
        assert _lib.SYMBOLS[name] == (ci, args)
        fn = getattr(L, name)
        assert fn.restype is ci and list(fn.argtypes) == args
        proto = re.search(r'\bint\s+%s\s*\((.*?)\)\s*;' % name, header, flags=re.S).group(1)
        assert len(proto.split(',')) == len(args)
    assert re.search(r'#define\s+VDET_MERGE_COMBINE\s+0\b', header) and re.search(r'#define\s+VDET_MERGE_MAX\s+1\b', header)


def test_null_context_and_bad_scheme_are_einval_without_a_device():
    from vdetlib_amd import _lib
    L = _lib.load_library()
    off = (ctypes.c_int64 * 2)(0, 4)
    nul = [None] * 8 + [None, None, 1] + [None] * 6
    for scheme in (0, 1, 2, -1):
        assert L.vdet_merge_tracks(None, scheme, 4, 3, 2, 2, *nul) == _lib.VDET_EINVAL
        assert L.vdet_merge_tracks_batch(None, scheme, off, 1, 3, 2, 2, *nul) == _lib.VDET_EINVAL


def test_ops_signatures():
    from vdetlib_amd import ops
    sig = inspect.signature(ops.merge_tracks)
    assert list(sig.parameters) == ['a', 'b', 'scheme', 'sync', 'ctx']
    assert (sig.parameters['scheme'].default, sig.parameters['sync'].default, sig.parameters['ctx'].default) == ('combine', True, None)
    sig = inspect.signature(ops.merge_tracks_batch)
    assert list(sig.parameters) == ['batch_a', 'batch_b', 'scheme', 'sync', 'ctx']
    assert (sig.parameters['scheme'].default, sig.parameters['sync'].default, sig.parameters['ctx'].default) == ('combine', True, None)


def _host_set(C=3, T=4, F=5, nser=2, tboxes=True):
    import torch
    s = dict(tracks=torch.zeros((C, T, F, 5)), ntracks=torch.zeros((C,), dtype=torch.int32), anchors=torch.zeros((C, T, 3)),
             series=tuple(torch.zeros((C, T, F), dtype=torch.float64) for _ in range(nser)))
    if tboxes:
        s['tboxes'] = torch.zeros((C, T, F, 4))
    return s


def test_merge_tracks_argument_errors_on_host_tensors():
    import torch
    from vdetlib_amd import ops
    a = _host_set()
    ch = lambda **kw: dict(_host_set(), **kw)
    cases = [
        (lambda: ops.merge_tracks(a, _host_set(), 'sum'), "scheme"),
        (lambda: ops.merge_tracks(a, ch(tracks=a['tracks'].double())), "b: tracks must be float32"),
        (lambda: ops.merge_tracks(ch(tracks=a['tracks'][..., :4]), a), "a: tracks must be float32"),
        (lambda: ops.merge_tracks(a, ch(ntracks=a['ntracks'].long())), "ntracks must be int32"),
        (lambda: ops.merge_tracks(a, ch(ntracks=a['ntracks'][:2])), "ntracks must be int32"),
        (lambda: ops.merge_tracks(a, ch(anchors=a['anchors'][:, :3])), "anchors must be float32"),
        (lambda: ops.merge_tracks(a, ch(anchors=a['anchors'].double())), "anchors must be float32"),
        (lambda: ops.merge_tracks(a, ch(tboxes=a['tboxes'][..., :3])), "tboxes must be float32"),
        (lambda: ops.merge_tracks(a, ch(tboxes=a['tboxes'].double())), "tboxes must be float32"),
        (lambda: ops.merge_tracks(a, ch(series=(a['series'][0].float(), a['series'][1]))), "float64"),
        (lambda: ops.merge_tracks(a, ch(series=(a['series'][0][:, :, :4], a['series'][1]))), "float64 tensor \\[C,T,F\\]"),
        (lambda: ops.merge_tracks(a, ch(series=())), "1 to 4 series"),
        (lambda: ops.merge_tracks(a, ch(series=tuple(a['series'][0] for _ in range(5)))), "1 to 4 series"),
        (lambda: ops.merge_tracks(a, {k: v for k, v in a.items() if k != 'anchors'}), "must be a dict"),
        (lambda: ops.merge_tracks(a, _host_set(C=2)), "share C and F"),
        (lambda: ops.merge_tracks(a, _host_set(F=6)), "share C and F"),
        (lambda: ops.merge_tracks(a, _host_set(nser=1)), "same number of series"),
        (lambda: ops.merge_tracks(a, _host_set(tboxes=False)), "tboxes: in both sets or in neither"),
        (lambda: ops.merge_tracks(_host_set(tboxes=False), a), "tboxes: in both sets or in neither"),
        (lambda: ops.merge_tracks(a, _host_set(T=6)), "same GPU"),                    # host tensors: there is no CPU path
        (lambda: ops.merge_tracks(a, a, 'max'), "same GPU"),
    ]
    if torch.cuda.is_available():       # mixed devices
        dev = {k: (tuple(x.cuda() for x in v) if k == 'series' else v.cuda()) for k, v in a.items()}
        cases.append((lambda: ops.merge_tracks(dev, a), "same GPU"))
        cases.append((lambda: ops.merge_tracks(dev, dict(dev, ntracks=a['ntracks'])), "same GPU"))
    for fn, msg in cases:
        with pytest.raises(ValueError, match=msg):
            fn()


def _host_batch(off=(0, 2, 5), C=3, T=4, pooled=True, tboxes=True):
    import torch
    off = np.asarray(off, dtype=np.int64)
    V, Ft = len(off) - 1, int(off[-1])

    def views(per, dtype):
        flat = torch.zeros((C * T * Ft * per,), dtype=dtype)
        return [flat[C * T * per * int(off[v]): C * T * per * int(off[v + 1])].view(*((C, T, int(off[v + 1] - off[v])) + ((per,) if per > 1 else ())))
                for v in range(V)]
    return dict(tracks=views(5, torch.float32), det=views(1, torch.float64), pooled=views(1, torch.float64) if pooled else [],
                tboxes=views(4, torch.float32) if tboxes else [], anchors=torch.zeros((V, C, T, 3)),
                ntracks=torch.zeros((V, C), dtype=torch.int32), frame_off=off)


def test_merge_tracks_batch_argument_errors_on_host_tensors():
    from vdetlib_amd import ops
    a = _host_batch()
    ch = lambda **kw: dict(_host_batch(), **kw)
    cases = [
        (lambda: ops.merge_tracks_batch(a, _host_batch(), 'sum'), "scheme"),
        (lambda: ops.merge_tracks_batch(a, _host_batch(off=(0, 3, 5))), "same frame_off"),
        (lambda: ops.merge_tracks_batch(a, _host_batch(off=(0, 5))), "same frame_off"),
        (lambda: ops.merge_tracks_batch(a, {k: v for k, v in a.items() if k != 'frame_off'}), "video_batch's layout"),
        (lambda: ops.merge_tracks_batch(a, ch(det=[])), "video_batch's layout"),
        (lambda: ops.merge_tracks_batch(a, _host_batch(C=2)), "share C"),
        (lambda: ops.merge_tracks_batch(a, ch(ntracks=a['ntracks'].long())), "ntracks must be int32"),
        (lambda: ops.merge_tracks_batch(a, ch(anchors=a['anchors'][:, :, :3])), "anchors float32"),
        (lambda: ops.merge_tracks_batch(a, ch(tracks=[x.double() for x in a['tracks']])), "not a video_batch result"),
        (lambda: ops.merge_tracks_batch(a, ch(tracks=a['tracks'][::-1])), "tracks\\[0\\] must be|consecutive"),
        (lambda: ops.merge_tracks_batch(a, ch(det=[x.float() for x in _host_batch()['det']])), "det must be float64"),
        (lambda: ops.merge_tracks_batch(a, ch(det=_host_batch(T=5)['det'])), "det must be float64"),
        (lambda: ops.merge_tracks_batch(a, _host_batch(T=6, pooled=False, tboxes=False)), "same GPU"),     # host tensors
        (lambda: ops.merge_tracks_batch(a, a, 'max'), "same GPU"),
    ]
    for fn, msg in cases:
        with pytest.raises(ValueError, match=msg):
            fn()
