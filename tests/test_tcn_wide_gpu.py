"""-m gpu: wide inputs of the device TCN (ops.tcn_tracks(wide=...) / tcn_tracks_batch(wide=...); csrc/tcn_kernels.hpp,
tcn_wide_layer_kernel) against two comparators, bit for bit, neither of which is the code under test:
  (i)  TCNNet.forward per tubelet -- the per-layer conv1d_kernel -- with its blobs filled with rows[frames].T and the
       one-channel series restated here in numpy;
  (ii) tests/tcn_wide_spec.py for layer 0 (numpy f32), followed by (i)'s later layers.
Tracks are built directly as arrays; no tracker runs."""
import os

import numpy as np
import pytest

import tcn_wide_spec as ws

pytestmark = pytest.mark.gpu

WIDE_TILE = 128          # kTcnWideTile: positions of one tile of the wide first layer
C, T, F = 3, 4, 70
NT = [4, 2, 0]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    nan_a, nan_b = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(nan_a, nan_b) and np.array_equal(a.view(np.uint32)[~nan_a], b.view(np.uint32)[~nan_b])


def make_tracks(seed, nC, nT, nF, nt, present):
    """Host arrays of one video: tracks [C,T,F,5] (NaN rows where ``present`` is False), anchors [C,T,3], det f64 [C,T,F],
    gt_overlap f64 [C,T,F].  Slots behind ntracks keep LIVE-looking rows: only ntracks says they do not exist."""
    rng = np.random.RandomState(seed)
    tr = rng.uniform(1, 200, (nC, nT, nF, 5)).astype(np.float32)
    tr[..., 4] = rng.rand(nC, nT, nF).astype(np.float32)
    tr[~present] = np.nan
    an = np.zeros((nC, nT, 3), np.float32)
    an[..., 0] = rng.randint(1, nF + 1, (nC, nT))
    det = rng.randn(nC, nT, nF)
    go = rng.rand(nC, nT, nF)
    return dict(tr=tr, an=an, nt=np.asarray(nt, np.int32), det=det, go=go)


def base_present():
    p = np.ones((C, T, F), bool)
    p[0, 1, :3] = False
    p[0, 1, 68:] = False                 # 65
    p[0, 2, 64:] = False                 # 64
    p[0, 3, 2::3] = False                # 47: every third frame a hole
    p[1, 0] = False
    p[1, 0, [10, 40]] = True             # 2
    p[1, 1] = False
    p[1, 1, 69] = True                   # 1
    return p


def to_dev(h):
    import torch
    return {k: torch.from_numpy(v).cuda() for k, v in h.items()}


@pytest.fixture(scope="module")
def base():
    h = make_tracks(1, C, T, F, NT, base_present())
    return h, to_dev(h)


def test_fixture_has_the_series_the_checks_need(base):
    h, _ = base
    has = ~np.isnan(h['tr'][..., 0])
    lens = sorted(int(has[c, t].sum()) for c in range(C) for t in range(NT[c]))
    assert lens == [1, 2, 47, 64, 65, 70]
    assert has[1, 2].all() and has[2].all()          # live-looking rows behind ntracks


def tubelets(h):
    """(c, t, frames) of every tubelet that exists."""
    has = ~np.isnan(h['tr'][..., 0])
    for c in range(h['tr'].shape[0]):
        for t in range(min(int(h['nt'][c]), h['tr'].shape[1])):
            fr = np.nonzero(has[c, t])[0]
            if len(fr):
                yield c, t, fr


def one_channel_series(h, c, t, fr):
    """The assembly of score_conv_cls restated: f64 values, one rounding to f32."""
    L = len(fr)
    rel = (fr + 1 - int(h['an'][c, t, 0])).astype(np.float64) / L
    go = h['go'][c, t, fr]
    return {'det_scores': h['det'][c, t, fr].astype(np.float32), 'track_scores': h['tr'][c, t, fr, 4],
            'anchors': rel.astype(np.float32), 'abs_anchors': np.abs(rel).astype(np.float32),
            'gt_overlaps': go.astype(np.float32), 'labels': (go >= 0.5).astype(np.float32)}


def rows_f32(rows):
    """Host f32 view of device rows as the kernel reads them (f16 / bf16 exact, f64 rounded once by numpy)."""
    import torch
    if rows.dtype == torch.float64:
        return rows.cpu().numpy().astype(np.float32)
    return rows.float().cpu().numpy()


def reference_forward(net, h, wide_np):
    """Comparator (i): TCNNet.forward per tubelet, blobs filled by hand."""
    want = np.full(h['det'].shape, np.nan, np.float32)
    for c, t, fr in tubelets(h):
        ser = one_channel_series(h, c, t, fr)
        for name, ch in net.inputs:
            blob = net.blobs[name]
            blob.reshape(1, ch, 1, len(fr))
            src = np.ascontiguousarray(wide_np[name][c, t][fr].T) if name in wide_np else ser[name]
            blob.data[...] = np.asarray(src, dtype=np.float32).reshape(1, ch, 1, len(fr))
        want[c, t, fr] = np.asarray(net.forward()['probs'])[0, 1]
    return want


def reference_spec(net, h, wide_np):
    """Comparator (ii): the spec for layer 0, then the later layers through TCNNet.forward (for a one-layer net: an
    identity K = 1 layer, whose fused softmax is the only thing left; exact for finite logits)."""
    from vdetlib_amd.vdet.tcn import TCNNet
    w0, b0 = net.layers[0]
    if len(net.layers) > 1:
        tail = TCNNet([('h0', w0.shape[0])], net.layers[1:])
    else:
        tail = TCNNet([('h0', 2)], [(np.eye(2, dtype=np.float32)[:, :, None], np.zeros(2, np.float32))])
    want = np.full(h['det'].shape, np.nan, np.float32)
    for c, t, fr in tubelets(h):
        x = ws.concat_inputs(net.inputs, one_channel_series(h, c, t, fr), {k: v[c, t] for k, v in wide_np.items()}, fr)
        h0 = ws.layer0(x, w0, b0, relu=len(net.layers) > 1)
        blob = tail.blobs['h0']
        blob.reshape(1, h0.shape[0], 1, len(fr))
        blob.data[...] = h0.reshape(1, h0.shape[0], 1, len(fr))
        want[c, t, fr] = np.asarray(tail.forward()['probs'])[0, 1]
    return want


def make_net(inputs, hidden, k0, k=3, seed=0):
    from vdetlib_amd.vdet.tcn import TCNNet
    rng = np.random.RandomState(seed)
    cin = sum(ch for _, ch in inputs)
    layers = []
    for i, cout in enumerate(list(hidden) + [2]):
        kk = k0 if i == 0 else k
        layers.append((rng.randn(cout, cin, kk).astype(np.float32) / np.sqrt(cin * kk), (0.1 * rng.randn(cout)).astype(np.float32)))
        cin = cout
    return TCNNet(inputs, layers)


def make_rows(inputs, shape, seed=5, dtype=None):
    """Device rows for every input that is not a device channel."""
    import torch
    from vdetlib_amd.vdet.tcn import TCNNet
    g = torch.Generator().manual_seed(seed)
    out = {}
    for name, ch in inputs:
        if name not in TCNNet.DEVICE_CHANNELS:
            out[name] = torch.randn(tuple(shape) + (ch,), generator=g, dtype=torch.float32).to(dtype or torch.float32).cuda()
    return out


def run(net, d, wide, ctx=None, go=None, sync=True):
    from vdetlib_amd import ops
    return ops.tcn_tracks(net, d['tr'], d['nt'], d['an'], d['det'], gt_overlap=go, sync=sync, ctx=ctx, wide=wide)


def check_both(net, h, d, wide, go=None, check_live=True):
    got = run(net, d, wide, go=go).cpu().numpy()
    wide_np = {k: rows_f32(v) for k, v in wide.items()}
    assert got.dtype == np.float32
    assert same_bits(got, reference_forward(net, h, wide_np)), "against TCNNet.forward"
    assert same_bits(got, reference_spec(net, h, wide_np)), "against the spec"
    live = ~np.isnan(h['tr'][..., 0]) & (np.arange(h['tr'].shape[1])[None, :, None] < h['nt'][:, None, None])
    assert not check_live or np.array_equal(~np.isnan(got), live)          # NaN exactly where there is no box
    return got


D, TS, AN, AB, GO, LB = (('det_scores', 1), ('track_scores', 1), ('anchors', 1), ('abs_anchors', 1), ('gt_overlaps', 1),
                         ('labels', 1))
# name: (inputs, hidden widths, K0).  The kernel stages 32 channels at a time (widths 31 / 32 / 33 and their sums), a wave
# owns 2 output channels up to cout0 = 8 and 8 above it, a pass covers 8 / 32 of them (cout0 8 | 9, 32 | 33, 64 | 70), and K0 = 3
# and 5 are unrolled instantiations, 1 and 7 the generic one.
CASES = {
    'as1_only_c1_k1': ([('all_scores', 1)], (1,), 1),
    'as3_first_c2_k3': ([('all_scores', 3), D], (2,), 3),
    'as8_last_c5_k5': ([D, ('all_scores', 8)], (5,), 5),
    'as9_c16_k7': ([('all_scores', 9), TS], (16,), 7),
    'as200_between_c17_k5': ([D, ('all_scores', 200), AN], (17,), 5),
    'f63_only_c64_k3': ([('feats', 63)], (64,), 3),
    'f64_c70_k1': ([('feats', 64), D], (70,), 1),
    'f65_c8_k7': ([AN, ('feats', 65)], (8,), 7),
    'f31_32_33_c9_k3': ([('all_scores', 31), ('feats', 32), ('more', 33)], (9,), 3),
    'two_wide_around_c32_k5': ([TS, ('all_scores', 33), D, AB, ('feats', 31), AN], (32,), 5),
    'c33_k3': ([('feats', 40), D], (33,), 3),
    'f1030_only_c5_k3': ([('feats', 1030)], (5,), 3),
    'flagship_as200_f1024_c64_k5': ([('all_scores', 200), D, ('feats', 1024)], (64,), 5),
    'gt_and_labels_beside_c5_k3': ([GO, ('all_scores', 8), LB], (5,), 3),
    'one_layer_k1': ([('all_scores', 9), D], (), 1),
    'one_layer_k3': ([D, ('all_scores', 200)], (), 3),
    'one_layer_k5': ([('feats', 65)], (), 5),
    'one_layer_k7': ([('all_scores', 3), AN, ('feats', 64)], (), 7),
    'three_layers_k5': ([('all_scores', 200), D, TS], (16, 7), 5),
    'four_layers_k3': ([D, ('feats', 65), AN], (17, 10, 5), 3),
}


@pytest.mark.parametrize("key", sorted(CASES))
def test_bit_equal_to_both_comparators(base, key):
    h, d = base
    inputs, hidden, k0 = CASES[key]
    net = make_net(inputs, hidden, k0, seed=len(key))
    wide = make_rows(inputs, (C, T, F))
    go = d['go'] if any(n in ('gt_overlaps', 'labels') for n, _ in inputs) else None
    check_both(net, h, d, wide, go=go)


def test_halo_longer_than_the_series():
    """K0 = 7 on series of 1 and 2 boxes (the fixture has them) is covered above; here K0 = 31, the largest, on 1, 2 and 20."""
    p = np.zeros((1, 3, 24), bool)
    p[0, 0, 5] = True
    p[0, 1, [0, 23]] = True
    p[0, 2, 2:22] = True
    h = make_tracks(3, 1, 3, 24, [3], p)
    inputs = [('all_scores', 9), D]
    check_both(make_net(inputs, (4,), 31, seed=2), h, to_dev(h), make_rows(inputs, (1, 3, 24)))


def test_series_over_three_position_tiles_and_a_remainder():
    nF = 3 * WIDE_TILE + 16
    p = np.ones((1, 2, nF), bool)
    p[0, 1, 1::5] = False
    h = make_tracks(4, 1, 2, nF, [2], p)
    assert int(p[0, 0].sum()) == 3 * WIDE_TILE + 16 and int(p[0, 1].sum()) > 2 * WIDE_TILE
    inputs = [('all_scores', 40), D]
    check_both(make_net(inputs, (9,), 5, seed=9), h, to_dev(h), make_rows(inputs, (1, 2, nF)))


def _ctx_with(env):
    from vdetlib_amd import _lib
    old = os.environ.get(env)
    os.environ[env] = "1"
    try:
        return _lib.Context()
    finally:
        if old is None:
            del os.environ[env]
        else:
            os.environ[env] = old


@pytest.mark.parametrize("key", ['one_layer_k3', 'as200_between_c17_k5', 'three_layers_k5', 'four_layers_k3'])
def test_forced_tiled_and_global_later_layers(base, key):
    h, d = base
    inputs, hidden, k0 = CASES[key]
    net = make_net(inputs, hidden, k0, seed=len(key))
    wide = make_rows(inputs, (C, T, F))
    want = run(net, d, wide).cpu().numpy()
    for env in ('VDET_TCN_TILED', 'VDET_TCN_GLOBAL'):
        cx = _ctx_with(env)
        try:
            assert same_bits(run(net, d, wide, ctx=cx).cpu().numpy(), want), env
        finally:
            cx.close()


@pytest.mark.parametrize("dtype", ['float32', 'float16', 'bfloat16', 'float64'])
def test_row_storage(base, dtype):
    import torch
    h, d = base
    dt = getattr(torch, dtype)
    inputs = [('all_scores', 9), D, ('feats', 65)]
    net = make_net(inputs, (9,), 3, seed=7)
    wide = make_rows(inputs, (C, T, F), dtype=dt)
    if dtype == 'float64':
        wide = {k: v + torch.randn(v.shape, dtype=dt, device=v.device) * 1e-9 for k, v in wide.items()}      # not f32 values
        up = 1.0 + 2.0 ** -24 + 2.0 ** -40                       # above the midpoint: rounds UP into f32
        wide['all_scores'][0, 0, 0, 0] = up
        assert np.float32(up) == np.float32(1.0) + np.float32(2.0 ** -23) and float(wide['all_scores'][0, 0, 0, 0]) == up
    check_both(net, h, d, wide)
    # rows whose base is only element-aligned: one element into a larger buffer (f16: 2 bytes, odd widths)
    shifted = {}
    for k, v in wide.items():
        buf = torch.empty(v.numel() + 1, dtype=dt, device=v.device)
        buf[1:] = v.reshape(-1)
        shifted[k] = buf[1:].view(v.shape)
        assert shifted[k].is_contiguous() and shifted[k].data_ptr() == buf.data_ptr() + v.element_size()
    assert same_bits(run(net, d, shifted).cpu().numpy(), run(net, d, wide).cpu().numpy())


def test_rows_of_holes_and_behind_ntracks_are_never_read(base):
    import torch
    h, d = base
    inputs = [('all_scores', 33), D]
    net = make_net(inputs, (9,), 5, seed=3)
    live = torch.from_numpy(~np.isnan(h['tr'][..., 0]) & (np.arange(T)[None, :, None] < h['nt'][:, None, None])).cuda()
    rows = make_rows(inputs, (C, T, F))['all_scores']
    zeros = torch.where(live[..., None], rows, torch.zeros_like(rows))
    poison = torch.where(live[..., None], rows, torch.full_like(rows, float('nan')))
    poison[..., 1::2] = torch.where(live[..., None], rows, torch.full_like(rows, float('inf')))[..., 1::2]
    assert not bool(torch.isfinite(poison[~live]).any())
    a = run(net, d, {'all_scores': zeros}).cpu().numpy()
    b = run(net, d, {'all_scores': poison}).cpu().numpy()
    assert same_bits(a, b) and np.array_equal(~np.isnan(b), live.cpu().numpy())


def test_nan_inside_a_read_row_reaches_its_neighbourhood_only(base):
    h, d = base
    inputs = [D, ('all_scores', 33)]
    k0 = 5
    net = make_net(inputs, (), k0, seed=4)                    # one layer: no ReLU between the NaN and the output
    rows = make_rows(inputs, (C, T, F))['all_scores']
    fr = np.nonzero(~np.isnan(h['tr'][0, 3, :, 0]))[0]        # the series with holes
    j0 = 20
    rows[0, 3, int(fr[j0]), 17] = float('nan')
    got = check_both(net, h, d, {'all_scores': rows}, check_live=False)
    nan_at = np.isnan(got[0, 3, fr])
    assert np.array_equal(np.nonzero(nan_at)[0], np.arange(j0 - k0 // 2, j0 + k0 // 2 + 1))


def _batch(nfs, nts, seed):
    """A video_batch-shaped dict built by hand (flat buffers, per-video views), and the per-video host arrays."""
    import torch
    hs = []
    for v, (nf, nt) in enumerate(zip(nfs, nts)):
        rng = np.random.RandomState(seed + v)
        p = rng.rand(C, T, nf) > 0.2
        p[:, :, 0] = True
        hs.append(make_tracks(seed + 10 * v, C, T, nf, nt, p))
    off = np.concatenate([[0], np.cumsum(nfs)]).astype(np.int64)

    def flat(key):
        return torch.from_numpy(np.concatenate([x[key].ravel() for x in hs])).cuda()
    tr, det, go = flat('tr'), flat('det'), flat('go')

    def views(buf, per):
        return [buf[C * T * int(off[v]) * per: C * T * int(off[v + 1]) * per].view((C, T, nfs[v]) + ((per,) if per > 1 else ()))
                for v in range(len(nfs))]
    bo = {'frame_off': off, 'tracks': views(tr, 5), 'det': views(det, 1),
          'ntracks': torch.from_numpy(np.stack([x['nt'] for x in hs])).cuda(),
          'anchors': torch.from_numpy(np.stack([x['an'] for x in hs])).cuda()}
    return hs, bo, go, views


def test_batch_equals_video_by_video():
    import torch
    from vdetlib_amd import ops
    nfs, nts = [9, 30, 17], [[4, 2, 0], [0, 0, 0], [1, 4, 3]]          # the second video has T slots and no tubelet
    hs, bo, go, views = _batch(nfs, nts, 40)
    inputs = [('all_scores', 33), D, GO, ('feats', 9)]
    net = make_net(inputs, (9,), 5, seed=6)
    Ft = sum(nfs)
    g = torch.Generator().manual_seed(1)
    flat = {n: torch.randn((C * T * Ft, ch), generator=g).cuda() for n, ch in (('all_scores', 33), ('feats', 9))}
    got = ops.tcn_tracks_batch(net, bo, gt_overlap=go, wide=flat)
    as_views = {n: views(r.view(-1), r.shape[1]) for n, r in flat.items()}
    got_views = ops.tcn_tracks_batch(net, bo, gt_overlap=go, wide=as_views)
    gov = views(go, 1)
    for v in range(len(nfs)):
        one = ops.tcn_tracks(net, bo['tracks'][v], bo['ntracks'][v], bo['anchors'][v], bo['det'][v], gt_overlap=gov[v],
                             wide={n: r[v] for n, r in as_views.items()})
        assert tuple(got[v].shape) == (C, T, nfs[v])
        assert same_bits(got[v].cpu().numpy(), one.cpu().numpy()) and same_bits(got_views[v].cpu().numpy(), one.cpu().numpy())
        want = reference_forward(net, hs[v], {n: rows_f32(r[v]) for n, r in as_views.items()})
        assert same_bits(one.cpu().numpy(), want), v
    assert bool(torch.isnan(got[1]).all())
    apart = dict(as_views)
    apart['feats'] = [r.clone() for r in as_views['feats']]             # per-video tensors of their own: not consecutive
    with pytest.raises(ValueError):
        ops.tcn_tracks_batch(net, bo, gt_overlap=go, wide=apart)
    with pytest.raises(ValueError):
        ops.tcn_tracks_batch(net, bo, gt_overlap=go, wide={'all_scores': flat['all_scores'][:-1], 'feats': flat['feats']})


def test_errors_leave_a_working_context(base):
    import torch
    from vdetlib_amd import _lib, ops
    h, d = base
    inputs = [('all_scores', 9), D]
    net = make_net(inputs, (5,), 3, seed=8)
    rows = make_rows(inputs, (C, T, F))['all_scores']
    want = run(net, d, {'all_scores': rows}).cpu().numpy()
    bad = [
        {'all_scores': rows[..., :8].contiguous()},                          # width unequal to the channel count
        {'all_scores': rows, 'det_scores': d['det'].float()[..., None]},     # a device-channel name in wide
        {'all_scores': rows.cpu()},                                          # CPU rows
        {'all_scores': torch.randn(C, T, F, 18, device='cuda')[..., ::2]},   # not contiguous
        {'all_scores': rows.to(torch.int32)},                                # an int dtype
        {'all_scores': rows[:, :, :-1].contiguous()},                        # shape
        {'all_scores': rows, 'feats': rows},                                 # rows for a blob the net does not have
        [rows],                                                              # not a dict
    ]
    for w in bad:
        with pytest.raises(ValueError):
            run(net, d, w)
    with pytest.raises(ValueError):                                          # a wide blob without rows: as before
        run(net, d, None)
    with pytest.raises(ValueError):
        run(make_net([('det_scores', 2)], (4,), 3), d, {'all_scores': rows})
    many = [('w%d' % i, 1) for i in range(17)]                               # 17 inputs
    with pytest.raises(ValueError):
        run(make_net(many, (4,), 3), d, {n: rows[..., :1].contiguous() for n, _ in many})
    with pytest.raises(ValueError):                                          # Cin = 4097
        run(make_net([('feats', 4096), D], (2,), 1), d, {'feats': torch.zeros(C, T, F, 4096, device='cuda')})
    # the raw C-ABI: a null row pointer, an unknown dtype, a width that does not chain, 17 inputs, Cin = 4097
    cx = _lib.get_context(torch.cuda.current_device())
    params, shapes = net.packed()
    out = torch.empty((C, T, F), dtype=torch.float32, device='cuda')

    def raw(codes, widths, ptrs, dtypes, shp=shapes, par=params):
        codes, widths = np.asarray(codes, np.int32), np.asarray(widths, np.int32)
        ptrs, dtypes = np.asarray(ptrs, np.uint64), np.asarray(dtypes, np.int32)
        return cx.lib.vdet_tcn_tracks_wide(cx.h, par.ctypes.data, shp.ctypes.data, len(shp), codes.ctypes.data, widths.ctypes.data,
                                           ptrs.ctypes.data, dtypes.ctypes.data, len(codes), F, C, T, d['tr'].data_ptr(),
                                           d['nt'].data_ptr(), d['an'].data_ptr(), d['det'].data_ptr(), 1, None, out.data_ptr())
    p = rows.data_ptr()
    assert raw([-1, 0], [9, 1], [0, 0], [0, 0]) == _lib.VDET_EINVAL
    assert raw([-1, 0], [9, 1], [p, 0], [4, 0]) == _lib.VDET_EINVAL
    assert raw([-1, 0], [8, 1], [p, 0], [0, 0]) == _lib.VDET_EINVAL
    assert raw([-1, 0], [0, 1], [p, 0], [0, 0]) == _lib.VDET_EINVAL
    assert raw([-1, 7], [9, 1], [p, 0], [0, 0]) == _lib.VDET_EINVAL
    assert raw([-1, 0], [9, 2], [p, 0], [0, 0]) == _lib.VDET_EINVAL
    assert raw([0] * 17, [1] * 17, [0] * 17, [0] * 17) == _lib.VDET_EINVAL
    big = np.array([[2, 4097, 1]], np.int32)
    assert raw([-1, 0], [4096, 1], [p, 0], [0, 0], shp=big, par=np.zeros(2 * 4097 + 2, np.float32)) == _lib.VDET_EINVAL
    with pytest.raises(ValueError):
        cx.check(_lib.VDET_EINVAL)
    assert raw([-1, 0], [9, 1], [p, 0], [0, 0]) == 0                         # the same call with good arguments
    cx.sync()
    assert same_bits(out.cpu().numpy(), want)
    assert same_bits(run(net, d, {'all_scores': rows}).cpu().numpy(), want)  # the context still works


def test_async_call_never_waits_and_repeat_uploads_nothing(base):
    from vdetlib_amd import _lib
    h, d = base
    inputs = [('all_scores', 33), D, ('feats', 65)]
    net = make_net(inputs, (9, 4), 5, seed=5)
    wide = make_rows(inputs, (C, T, F))
    cx = _lib.Context()
    try:
        want = run(net, d, wide, ctx=cx)
        n_up = cx.query(10)
        before = cx.query(8)
        a = run(net, d, wide, ctx=cx, sync=False)
        d2 = dict(d)
        d2['det'] = d['det'] * 0.5
        b = run(net, d2, wide, ctx=cx, sync=False)
        assert cx.query(8) == before, "an asynchronous tcn_tracks(wide=...) waited for the device"
        assert cx.query(10) == n_up == 1
        cx.sync()
        assert cx.query(8) == before + 1
        assert same_bits(a.cpu().numpy(), want.cpu().numpy())
        h2 = dict(h)
        h2['det'] = h['det'] * 0.5
        assert same_bits(b.cpu().numpy(), reference_forward(net, h2, {k: rows_f32(v) for k, v in wide.items()}))
    finally:
        cx.close()


def test_narrow_calls_are_untouched_by_an_empty_wide(base):
    h, d = base
    net = make_net([D, TS, AN], (5,), 3, seed=1)
    a, b = run(net, d, None).cpu().numpy(), run(net, d, {}).cpu().numpy()
    assert same_bits(a, b) and same_bits(a, reference_forward(net, h, {}))


def test_chain_from_patches_to_the_evaluator():
    """tubelet_patches -> a one-line net -> svm_head -> the winners' rows -> svm_scores -> index_put_ through slot ->
    tcn_tracks(wide={'all_scores': ...}) -> DetEvaluator.add_tracks."""
    import torch
    from vdetlib_amd import eval as vev, ops
    nC, nT, nF, K = 2, 2, 6, 16
    rng = np.random.RandomState(11)
    p = np.ones((nC, nT, nF), bool)
    p[0, 1, 2] = False
    p[1, 0, :3] = False
    h = make_tracks(12, nC, nT, nF, [2, 1], p)
    x1, y1 = rng.randint(1, 20, (nC, nT, nF)), rng.randint(1, 12, (nC, nT, nF))
    h['tr'][..., 0], h['tr'][..., 1] = x1, y1
    h['tr'][..., 2], h['tr'][..., 3] = x1 + rng.randint(8, 24, x1.shape), y1 + rng.randint(8, 16, x1.shape)
    h['tr'][~p] = np.nan
    d = to_dev(h)
    images = torch.from_numpy(rng.randint(0, 256, (nF, 32, 48, 3)).astype(np.uint8)).cuda()
    pat = ops.tubelet_patches(images, d['tr'], d['nt'], (0, nF), cap=nC * nT * nF, crop_size=8, padding=1)
    n = int(pat['count'])
    assert n == int((p & (np.arange(nT)[None, :, None] < h['nt'][:, None, None])).sum())
    proj = torch.from_numpy(rng.randn(3 * 8 * 8, K).astype(np.float32) / 100).cuda()
    feats = (pat['patches'].flatten(1) @ proj).contiguous()                                   # the "net"
    model = {'W': torch.from_numpy(rng.randn(K, 200).astype(np.float32)).cuda(),
             'B': torch.from_numpy(rng.randn(200).astype(np.float32)).cuda(), 'feat_norm_mean': 20.0}
    head = ops.svm_head(feats, model, group=1, slot=pat['slot'], count=pat['count'], shape=(nC, nT, nF),
                        cols=torch.arange(nC, dtype=torch.int32, device='cuda'))
    assert int(head['nbad']) == 0
    winners = torch.arange(n, device='cuda') + head['arg_flat'][:n].long()
    all_sc = ops.svm_scores(feats[winners].contiguous(), model)                               # [n, 200]
    c, t, f = pat['slot'][:n].long().unbind(1)
    rows = torch.full((nC, nT, nF, 200), float('nan'), dtype=all_sc.dtype, device='cuda')     # NaN where nothing is read
    rows.index_put_((c, t, f), all_sc)
    inputs = [D, ('all_scores', 200)]
    net = make_net(inputs, (8,), 3, seed=13)
    conv = ops.tcn_tracks(net, d['tr'], d['nt'], d['an'], head['det'], wide={'all_scores': rows})
    hh = dict(h)
    hh['det'] = head['det'].double().cpu().numpy()
    want = reference_forward(net, hh, {'all_scores': rows_f32(rows)})
    assert same_bits(conv.cpu().numpy(), want) and np.isfinite(want[~np.isnan(want)]).all()
    annot = {'video': 'chain', 'annotations': [{'id': '0', 'track': [
        {'frame': 1, 'bbox': [int(v) for v in h['tr'][0, 0, 0, :4]], 'class_index': 1, 'class': 'c1'}]}]}
    ev = ops.DetEvaluator(vev.gt_table_from_annots([annot]))
    assert ev.add_tracks('chain', d['tr'], d['nt'], scores=conv) > 0
    aps, _ = ev.compute()
    assert aps
