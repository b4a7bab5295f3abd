"""Runs without a GPU: the two references the seam tests of tests/test_temporal_seams_gpu.py lean on agree with each other
(tests/temporal_cases.py's numpy statement of the temporal operators == the C oracle, on every case those tests run), and
the case set is what it claims to be (every "seamed" shape really splits into >= 3 frame chunks under the host's formulas,
all four tilings of the fused pass occur, video borders fall on, before and behind a seam, ...)."""
import numpy as np
import pytest

import temporal_cases as tc

N_CU = 256          # an MI355X


def _per_video(fn, vol, off):
    return np.concatenate([fn(vol[a:b]) for a, b in zip(off[:-1], off[1:])])


def _case_id(case):
    label, shape, W, taps, pm, pc, border = case
    return "%s-%dx%dx%d-W%d-%g-%s" % (label, shape[0], shape[1], shape[2], W, pm, border)


@pytest.mark.parametrize("case", tc.reference_cases(), ids=_case_id)
def test_references_equal_the_oracle(oracle, case):
    label, shape, W, taps, pm, pc, border = case
    vol = tc.seam_volume(*shape, tc.seed_of(*shape))
    off = np.array([0, shape[0]]) if border is None else tc.border_table(border, shape[0])
    got = tc.cached_maxpool(shape, W, pm, border)
    want = _per_video(lambda v: oracle.temporal_maxpool(v, W, pm), vol, off)
    assert got.dtype == np.float32 and np.array_equal(got, want, equal_nan=True)
    if taps is not None:
        got = tc.cached_conv(shape, W, pc, border)
        want = _per_video(lambda v: oracle.temporal_conv(v, taps, tc.BIAS, pc), vol, off)
        assert got.dtype == np.float32 and np.array_equal(got, want, equal_nan=True)
        if shape[1] * shape[2] > 30 and shape[0] > 3:      # (at S = 8 the specials of 4 series per frame swamp a wide window)
            assert np.isnan(got).any() and np.isfinite(got).any()


def test_one_video_is_no_table():
    shape = tc.FUSED[0]
    vol = tc.seam_volume(*shape, tc.seed_of(*shape))
    one = tc.border_table("one", shape[0])
    assert np.array_equal(tc.ref_maxpool(vol, 5, 0.5, one), tc.ref_maxpool(vol, 5, 0.5), equal_nan=True)
    assert np.array_equal(tc.ref_conv(vol, tc.taps_for(5), tc.BIAS, -1.0, one), tc.ref_conv(vol, tc.taps_for(5), tc.BIAS, -1.0),
                          equal_nan=True)


def test_seam_volume_puts_every_special_on_every_frame():
    for shape in tc.FUSED + tc.STANDALONE:
        F, B, C = shape
        v = tc.seam_volume(F, B, C, tc.seed_of(*shape)).reshape(F, B * C)
        S = B * C
        for f in range(F):
            assert np.isnan(v[f, (3 * f) % S]) and v[f, (3 * f + 1) % S] == np.inf and v[f, (3 * f + 2) % S] == -np.inf
            if S > 8:
                assert v[f, (5 * f + 7) % S] == 0 and np.signbit(v[f, (5 * f + 7) % S])
    F, B, C = tc.FUSED[2]
    v = tc.seam_volume(F, B, C, tc.seed_of(F, B, C))
    ties = sum(B - len(np.unique(v[f, :, c])) for f in range(F) for c in range(C))
    assert ties >= F * B * C // 200, "the volume has (almost) no tied scores"
    o, n = tc.cached_keys_order((F, B, C), 0.25)
    assert 0 < n.min() and n.max() < B          # the threshold cuts every list somewhere inside


def test_keys_reference_and_tail():
    s = np.array([[[0.5], [np.nan], [-0.0], [0.5], [0.0], [-np.inf], [np.inf]]], dtype=np.float32)
    o, n = tc.ref_keys_order(s)
    assert o[0, 0].tolist() == [1, 6, 3, 0, 4, 2, 5] and n[0, 0] == 7
    o, n = tc.ref_keys_order(s, 0.25)
    assert o[0, 0].tolist() == [6, 3, 0, 5, 4, 2, 1] and n[0, 0] == 3
    shuffled = np.array([[[6, 3, 0, 2, 5, 1, 4]]])
    assert np.array_equal(tc.canonical_tail(shuffled, n), o)
    assert not np.array_equal(tc.canonical_tail(np.array([[[3, 6, 0, 2, 5, 1, 4]]]), n), o)      # candidates stay put


def test_border_tables():
    for F in sorted({s[0] for s in tc.FUSED} | {c[0] for c in tc.BATCH_FALLBACK}):
        for name in tc.BORDER_SETS:
            off = tc.border_table(name, F)
            assert off[0] == 0 and off[-1] == F and np.all(np.diff(off) > 0), (name, F)
        assert np.all(np.diff(tc.border_table("each", F)) == 1)
        assert np.diff(tc.border_table("cycle", F))[:7].tolist() == [1, 2, 1, 3, 5, 1, 9]
        d = np.diff(tc.border_table("long", F))
        assert d.max() >= min(40, F - 2) and d[0] == 1 and d[-1] == 1 and sorted(d)[-2] == 1
        assert tc.border_table("one", F).tolist() == [0, F]
    assert np.diff(tc.border_table("long", 51)).max() == 40


def _plan(kind, F, B, C):
    return tc.chunk_plan(kind, F, B, C, N_CU)


def test_seamed_cases_have_their_seams():
    for F, B, C in tc.STANDALONE:
        chunks, fchunk, tiling = _plan("standalone", F, B, C)
        assert chunks >= 3 and tiling is None, tc.REPICK % ("standalone %dx%d" % (F, B * C))
    assert _plan("standalone", 51, 2, 4)[:2] == (3, 17) and _plan("standalone", 64, 257, 4)[:2] == (4, 16)
    tilings, odd, ragged_b, short_tile = set(), False, False, False
    for F, B, C in tc.FUSED:
        chunks, fchunk, tiling = _plan("fused", F, B, C)
        assert chunks >= 3 and tiling == tc.FUSED_TILINGS[C], tc.REPICK % ("fused %dx%dx%d" % (F, B, C))
        tilings.add(tiling)
        odd |= fchunk % 2 == 1 and any(f0 % 2 == 1 for f0 in tc.seams(chunks, fchunk))
        ragged_b |= B % 4 != 0
        short_tile |= B % tiling[1] != 0
    assert tilings == {(256, 64), (256, 32), (512, 32), (512, 16)}
    assert odd and ragged_b and short_tile
    assert _plan("fused", 36, 70, 8) == (4, 9, (256, 64)) and _plan("fused", 27, 45, 200) == (3, 9, (512, 32))
    for F, B, C, W, taps, kernel in tc.BATCH_FALLBACK:
        chunks, fchunk, tiling = _plan("fused", F, B, C)
        if kernel == "scalar":
            assert (B * C) % 4 != 0 and chunks == 1
        else:
            # these windows / class counts are not the fused kernel's: its plan does not apply, the standalone one does
            assert W > 5 or tiling is None
            assert _plan("standalone", F, B, C)[0] >= 3, tc.REPICK % ("fallback %dx%dx%d" % (F, B, C))
    assert all((B * C) % 4 != 0 for F, B, C in tc.ODD_S)


def test_video_borders_meet_the_seams():
    """over the tables that are not one-video-per-frame (where it would hold trivially): some border ON a seam, some one
    frame before, some one frame behind"""
    rel = set()
    shapes = [(s, "fused") for s in tc.FUSED] + [(c[:3], "standalone") for c in tc.BATCH_FALLBACK if c[5] != "scalar"]
    for (F, B, C), kind in shapes:
        chunks, fchunk, _ = _plan(kind, F, B, C)
        for name in ("cycle", "long"):
            inner = set(tc.border_table(name, F)[1:-1].tolist())
            for s in tc.seams(chunks, fchunk):
                rel |= {d for d in (-1, 0, 1) if s + d in inner}
    assert rel == {-1, 0, 1}
    # and with every frame its own video all three hold at every seam
    assert len(tc.border_table("each", 36)) == 37


def test_chunk_plan_follows_the_device_width():
    """fewer compute units -> fewer chunks; the guard is a function of n_cu, which the GPU tests read from the device"""
    assert tc.chunk_plan("fused", 36, 70, 8, 256)[0] == 4
    assert tc.chunk_plan("fused", 300, 10000, 200, 256)[:2] == (7, 43)
    assert tc.chunk_plan("standalone", 300, 10000, 200, 256)[0] == 1
    assert tc.chunk_plan("standalone", 64, 128, 1, 1)[0] == 4 and tc.chunk_plan("standalone", 64, 4096, 1, 1)[0] == 1
    assert tc.chunk_plan("fused", 36, 70, 30, 256) == tc.chunk_plan("standalone", 36, 70, 30, 256)
    assert tc.chunk_plan("fused", 36, 70, 400, 256, max_lds=64 * 1024)[2] is None
