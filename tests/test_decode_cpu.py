"""CPU: the numpy rule of the Fast R-CNN box decode (tests/decode_spec.py) against itself and against the host functions it
restates -- the vectorised spec against its plain loop on every case of tests/decode_cases.py, E against np.exp, the spec against
``clip_boxes(bbox_transform_inv(...))``, the clip's NaN and -0.0 cases, the rank layout of ``dets_as_tracks`` from a loop -- and
guards that the case list still holds what it is there for.  Nothing here touches the device."""
import numpy as np
import pytest

import decode_cases as dc
import decode_spec as ds

F32, F64 = np.float32, np.float64
ULP = 2.0 ** -52


def same_bits(a, b):
    """Equal bit for bit, a NaN equal to a NaN whatever its payload."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    bits = {4: np.int32, 8: np.int64}[a.dtype.itemsize]
    return bool(np.array_equal(na, nb) and np.array_equal(a[~na].view(bits), b[~nb].view(bits)))


CASES = {c[0]: c for c in dc.cases()}


@pytest.mark.parametrize('name', list(CASES))
def test_vectorised_spec_equals_the_loop_transcription(name):
    _, rois, deltas, im_size = CASES[name]
    got = ds.decode(rois, deltas, im_size)
    assert got.dtype == F32 and got.shape == deltas.shape
    assert same_bits(got, ds.decode_loop(rois, deltas, im_size))
    if rois.dtype == F32:          # a f32 roi widened by the caller is the same roi
        assert same_bits(got, ds.decode(rois.astype(F64), deltas, im_size))


def test_E_against_numpy_exp():
    """E is a degree-13 Taylor polynomial on |r| <= ln2/2 after an exact-product range reduction.  Its error budget in units of
    2^-52 relative: the last Horner step p*r + 1 rounds twice (<= 0.5 for the sum, <= 0.5*|r| <= 0.18 for the product), the
    earlier steps and the truncation r^14/14! add less than 0.05, and the reduced argument's own error (|k| * ulp(ln2_lo) and
    two roundings at |r| <= 0.35, absolute ~4e-17) another 0.2: below 1.  np.exp is itself within 1 of the true value.  So the
    two differ by less than 2 units of 2^-52; that is the bound asserted, and the measured maximum -- 1.00 on this sample -- is
    printed before it."""
    rng = np.random.RandomState(20)
    x = np.concatenate([rng.uniform(-10, 10, 2000000).astype(F32), np.linspace(-10, 10, 200001).astype(F32),
                        np.array([0.0, -0.0, 1.0, -1.0, 10.0, -10.0], F32)]).astype(F64)
    got, want = ds.E(x), np.exp(x)
    err = float(np.max(np.abs(got - want) / want)) / ULP
    print("max relative error of E against np.exp on [-10, 10]: %.4f units of 2^-52" % err)
    assert err <= 2.0
    assert np.all(np.diff(ds.E(np.sort(x[:1000]))) >= 0)           # (a sanity check of the shape, no claim of monotonicity)
    some = rng.randint(0, len(x), 300)
    assert same_bits(got[some], np.array([ds.E_loop(v) for v in x[some]]))


def test_E_special_values():
    x = np.array([np.nan, np.inf, -np.inf, 709.0, np.nextafter(709.0, np.inf), -708.0, np.nextafter(-708.0, -np.inf), 0.0, -0.0,
                  3.4e38, -3.4e38])
    got = ds.E(x)
    assert np.isnan(got[0]) and got[1] == np.inf and got[2] == 0 and not np.signbit(got[2])
    assert np.isfinite(got[3]) and abs(got[3] / np.exp(709.0) - 1) <= 2 * ULP and got[4] == np.inf
    assert got[5] >= np.finfo(F64).tiny and abs(got[5] / np.exp(-708.0) - 1) <= 2 * ULP and got[6] == 0 and not np.signbit(got[6])
    assert got[7] == 1.0 and got[8] == 1.0 and got[9] == np.inf and got[10] == 0
    assert same_bits(got, np.array([ds.E_loop(v) for v in x]))


def test_clip_keeps_nan_and_turns_negative_zero_into_positive_zero():
    v = np.array([np.nan, -0.0, 0.0, -1.0, 5.0, 99.0, np.nextafter(99.0, 100.0), np.inf, -np.inf, 1e-320, -1e-320])
    got = ds.clip(v, 99)
    want = np.array([np.nan, 0.0, 0.0, 0.0, 5.0, 99.0, 99.0, 99.0, 0.0, 1e-320, 0.0])
    assert same_bits(got, want) and not np.signbit(got[1]) and not np.signbit(got[10])
    assert same_bits(got, np.array([ds.clip_loop(F64(x), 99) for x in v]))
    # numpy's own clip, the host's: the same values, and a NaN where the spec has one (the sign of its zero is the host's)
    host = np.maximum(np.minimum(v, 99), 0)
    assert np.array_equal(np.isnan(host), np.isnan(got)) and np.array_equal(host[1:], got[1:])
    # the device's fmin / fmax would have dropped the NaN
    assert not np.isnan(np.fmax(np.fmin(v[:1], 99), 0)[0])


def test_nonfinite_inputs_give_nan_or_clipped_coordinates_only():
    for name in ('nonfinite_roi', 'nonfinite_delta'):
        _, rois, deltas, (H, W) = CASES[name]
        out = ds.decode(rois, deltas, (H, W))
        ok = ~np.isnan(out)
        assert np.isnan(out).any()
        assert np.all(out[ok] >= 0) and np.all(out[..., 0::2][ok[..., 0::2]] <= W - 1) and np.all(out[..., 1::2][ok[..., 1::2]] <= H - 1)
        assert not np.signbit(out[ok]).any()
    # a NaN in x touches x only
    out = ds.decode(np.array([[np.nan, 1, 20, 20]], F32), np.zeros((1, 1, 4), F32), (375, 500))[0, 0]
    assert np.isnan(out[0]) and np.isnan(out[2]) and out[1] == 1 and out[3] == 20


def test_spec_against_the_host_pair():
    """clip_boxes(bbox_transform_inv(...)).astype(float32) on 4 * 10^5 seeded elements: at most 1 element in 10^4 may differ,
    and those by one f32 ulp only (E is within 2 f64 ulp of np.exp, so a difference needs a coordinate within ~1e-13 px of a
    f32 rounding boundary)."""
    from vdetlib_amd.vdet.image_det import bbox_transform_inv, clip_boxes
    n, K, im = 20000, 5, (375, 500)
    differ = total = 0
    for seed, f64 in ((31, False), (32, True)):
        rois, deltas = dc.random_case(seed, n, K, im, f64=f64)
        got = ds.decode(rois, deltas, im)
        want = clip_boxes(bbox_transform_inv(rois, deltas.reshape(n, 4 * K)), im + (3,)).astype(F32).reshape(n, K, 4)
        ne = got != want
        differ += int(ne.sum()); total += got.size
        assert np.all(np.abs(got[ne].view(np.int32) - want[ne].view(np.int32)) == 1)
    print("elements that differ from the host pair: %d of %d" % (differ, total))
    assert total >= 10 ** 5 and differ * 10 ** 4 <= total


def test_dets_as_tracks_layout_from_a_loop():
    rng = np.random.RandomState(33)
    F, K, topk = 3, 4, 6
    dets = rng.rand(F, K, topk, 5).astype(F32)
    sel = rng.randint(0, 50, (F, K, topk)).astype(np.int32)
    keep_cnt = rng.randint(0, topk + 1, (F, K)).astype(np.int32)
    keep_cnt[0, 2], keep_cnt[1, 3] = 0, topk
    keep = np.full((F, K, topk), -1, np.int32)
    for f in range(F):
        for j in range(K):
            keep[f, j, :keep_cnt[f, j]] = rng.permutation(topk)[:keep_cnt[f, j]]
    for first in (0, 1, 2):
        out = ds.dets_as_tracks(dets, sel, keep, keep_cnt, first)
        C = K - first
        assert out['tracks'].shape == (C, topk, F, 5) and out['score'].dtype == F64 and out['src'].shape == (C, topk, F)
        assert np.array_equal(out['cnt'], keep_cnt[:, first:].T) and np.array_equal(out['ntracks'], keep_cnt[:, first:].max(0))
        for c in range(C):
            for f in range(F):
                n = keep_cnt[f, c + first]
                assert np.array_equal(out['tracks'][c, :n, f], dets[f, c + first, keep[f, c + first, :n]])
                assert np.array_equal(out['score'][c, :n, f], dets[f, c + first, keep[f, c + first, :n], 4].astype(F64))
                assert np.array_equal(out['src'][c, :n, f], sel[f, c + first, keep[f, c + first, :n]])
                assert np.isnan(out['tracks'][c, n:, f]).all() and np.isnan(out['score'][c, n:, f]).all()
                assert np.all(out['src'][c, n:, f] == -2 ** 31)


def test_case_list_still_holds_its_edge_cases():
    assert set(dc.EDGE_NAMES) <= set(CASES) and sum(n.startswith('random') for n in CASES) >= 3
    out = {n: ds.decode(*CASES[n][1:]) for n in CASES}
    _, rois, deltas, (H, W) = CASES['on_border']
    assert np.array_equal(out['on_border'][0, 0], [0, 0, W - 1, H - 1])
    _, rois, deltas, (H, W) = CASES['beyond_border']
    r, d = rois.astype(F64), deltas.astype(F64)
    x2 = (d[..., 0] * ((r[:, 2] - r[:, 0]) + 1e-14)[:, None] + (r[:, 0] + 0.5 * ((r[:, 2] - r[:, 0]) + 1e-14))[:, None]) \
        + 0.5 * (ds.E(d[..., 2]) * ((r[:, 2] - r[:, 0]) + 1e-14)[:, None])
    assert x2[0, 0] == np.nextafter(F64(W - 1), np.inf)              # one f64 step beyond W-1, clipped back onto it
    assert out['beyond_border'][0, 0, 2] == W - 1 and (x2 > W - 1).sum() >= 3
    assert out['beyond_border'][1, 0, 0] == 0 and rois[1, 0] < 0 and rois[1, 0] > -1e-10
    assert any(np.signbit(c[1]).any() and (c[1] == 0).any() for c in (CASES['neg_zero'],))
    assert np.signbit(CASES['neg_zero'][2]).any() and not np.signbit(out['neg_zero']).any()
    assert {10.0, -10.0} <= set(CASES['dw_pm10'][2][..., 2:].ravel().tolist())
    e = CASES['overflow_edge'][2][..., 2].ravel().astype(F64)
    assert (e == 709).any() and (e > 709).any() and ((e < 709) & (e > 708.99)).any()
    assert (e == -708).any() and (e < -708).any() and ((e > -708) & (e < -707.99)).any()
    assert np.isinf(ds.E(e)).any() and (ds.E(e) == 0).any()
    for n in ('nonfinite_roi', 'nonfinite_delta'):
        src = CASES[n][1] if n.endswith('roi') else CASES[n][2]
        assert np.isnan(src).any() and np.isposinf(src).any() and np.isneginf(src).any()
    zr = CASES['zero_width'][1]
    assert (zr[:, 0] == zr[:, 2]).all()
    iv = CASES['inverted'][1]
    assert (iv[:, 2] < iv[:, 0]).any() and (iv[:, 3] < iv[:, 1]).any()
    fr = CASES['f64_rois'][1]
    assert fr.dtype == F64 and (fr.astype(F32).astype(F64) != fr).all()
    assert not same_bits(out['f64_rois'], ds.decode(fr.astype(F32), CASES['f64_rois'][2], CASES['f64_rois'][3]))
    assert any(c[1].dtype == F64 for c in dc.cases()) and any(c[1].dtype == F32 for c in dc.cases())
