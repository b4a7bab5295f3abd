"""CPU-only checks of the tubelet re-scoring's specification helper (tests/rescore_spec.py), its input recipe, the recorded
reference outputs it must reproduce, and the C-ABI binding of vdet_rescore_tubelets[_batch]."""
import os
import re

import numpy as np
import pytest

import rescore_spec as R
import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the recipe's checked outcomes, C = 2, T = 3: (F, B, seed) -> hits, misses, hits with >= 2 candidates, tied maxima,
# leading / trailing gaps, tubelets with an inner hole, floor: detection wins / floor wins
TABLE = {(9, 5, 9100): (23, 16, 23, 11, 3, 2, 4, 15, 8), (9, 300, 9101): (19, 20, 19, 8, 1, 3, 5, 14, 5),
         (70, 300, 9102): (211, 113, 172, 96, 4, 1, 6, 116, 95), (9, 1100, 9103): (29, 15, 29, 7, 2, 1, 3, 20, 9)}


@pytest.mark.parametrize('key', sorted(TABLE))
def test_recipe_outcomes(oracle, key):
    F, B, seed = key
    boxes, scores = R.volume(seed, F, B, 2)
    tracks, floor = R.tubelets(seed, boxes, 2, 3)
    cz = R.census(tracks, np.full(2, 3), boxes, scores, floor)
    got = tuple(cz[k] for k in ('hits', 'misses', 'multi', 'tied', 'leading', 'trailing', 'inner_hole', 'det_wins', 'floor_wins'))
    assert got == TABLE[key], cz
    assert cz['all_miss'] == 0 and cz['interior'] >= 1
    R.check_census(cz, [0, F])


@pytest.mark.parametrize('B', [5, 300, 1100])
@pytest.mark.parametrize('off', [[0, 9], [0, 1, 2], [0, 3, 4, 13]])
def test_parity_cases_are_not_vacuous(oracle, B, off):
    cz = R.batch_case(R.PARITY_SEEDS[B], off, B)[5]
    R.check_census(cz, off)


def test_holes_are_no_list_elements(oracle):
    """A hand-made tubelet on frames 0, 2, 3, 6 (holes on 1, 4, 5): hit 0.25, miss, miss, hit 1.0 -> the two misses are
    interpolated on ORDINALS (0.5, 0.75) and the pool's neighbours are list neighbours."""
    F, B = 7, 2
    boxes = np.zeros((F, B, 4), np.float32)
    boxes[:, 0] = [10, 10, 50, 50]
    boxes[:, 1] = [300, 300, 340, 340]
    scores = np.zeros((F, B, 1), np.float32)
    scores[0, 0, 0], scores[6, 0, 0] = 0.25, 1.0
    tracks = np.full((1, 1, F, 5), np.nan, np.float32)
    for f, hit in ((0, True), (2, False), (3, False), (6, True)):
        tracks[0, 0, f] = [10, 10, 50, 50, 1] if hit else [600, 600, 640, 640, 1]
    det, pooled, tb, src, err = R.spec(tracks, [1], boxes, scores, window=3)
    assert not err
    assert det[0, 0, [0, 2, 3, 6]].tolist() == [0.25, 0.5, 0.75, 1.0] and np.all(np.isnan(det[0, 0, [1, 4, 5]]))
    assert pooled[0, 0, [0, 2, 3, 6]].tolist() == [0.5, 0.75, 1.0, 1.0] and np.all(np.isnan(pooled[0, 0, [1, 4, 5]]))
    assert src[0, 0].tolist() == [0, -1, -1, -1, -1, -1, 0]
    assert np.array_equal(tb[0, 0, 2], tracks[0, 0, 2, :4]) and np.array_equal(tb[0, 0, 6], boxes[6, 0])
    # with a floor nothing is completed: the floor stands where nothing beats it
    floor = np.full((1, 1, F), 0.5)
    det, pooled, tb, src, err = R.spec(tracks, [1], boxes, scores, floor=floor, window=1)
    assert det[0, 0, [0, 2, 3, 6]].tolist() == [0.5, 0.5, 0.5, 1.0] and src[0, 0].tolist() == [-1, -1, -1, -1, -1, -1, 0]
    assert np.array_equal(pooled, det, equal_nan=True)
    # every box misses: the reference's IndexError
    tracks[0, 0, [0, 6], :4] = [600, 600, 640, 640]
    det, pooled, tb, src, err = R.spec(tracks, [1], boxes, scores)
    assert err and np.all(np.isnan(pooled)) and det[0, 0, [0, 2, 3, 6]].tolist() == [-1e5] * 4


def test_spec_equals_oracle_on_the_trackers_tubelets(oracle):
    """On hole-free tubelets the list form is the frame form: spec() reproduces oracle.rescored_tubelets."""
    boxes, scores = synth.coherent_video(9110, 8, 120, 2)
    wtr, wnt, wsc, wbx, wdet = oracle.rescored_tubelets(boxes, scores, 0.3, 0.0, 3, 0.5, 0.7, 3, return_det=True)
    det, pooled, tb, src, err = R.spec(wtr, wnt, boxes, scores, overlap_thres=0.7, window=3)
    assert not err and wnt.min() >= 1
    assert np.array_equal(det, wdet, equal_nan=True) and np.array_equal(pooled, wsc, equal_nan=True)
    assert np.array_equal(tb, wbx, equal_nan=True)


def test_spec_equals_the_reference(oracle):
    for case in R.load_golden():
        boxes, scores, tracks, floor = R.golden_inputs(case)
        nt = np.full(case['C'], case['T'])
        assert np.isnan(tracks[:, :, :, 0]).any()                  # tubelets WITH holes
        g = R.golden_arrays(case, 'maxpool')
        for window, key in ((3, 'pool3'), (5, 'pool5')):
            det, pooled, tb, _, err = R.spec(tracks, nt, boxes, scores, overlap_thres=case['overlap_thres'], window=window)
            assert not err
            assert np.array_equal(det, g['det_score'], equal_nan=True), (case['seed'], window)
            assert np.array_equal(pooled, g[key], equal_nan=True), (case['seed'], window)
            assert np.array_equal(tb.astype(np.float64), g['bbox'], equal_nan=True)
        g = R.golden_arrays(case, 'sampling')
        det, pooled, tb, src, err = R.spec(tracks, nt, boxes, scores, floor=floor, overlap_thres=case['overlap_thres'], window=1)
        assert np.array_equal(det, g['det_score'], equal_nan=True) and np.array_equal(tb.astype(np.float64), g['bbox'], equal_nan=True)
        assert (src >= 0).any() and ((src < 0) & ~np.isnan(det)).any()


def test_golden_is_small_and_holds_no_program_text():
    path = os.path.join(ROOT, 'tests', 'golden', 'rescore_golden.json.gz')
    assert os.path.getsize(path) < 200 * 1024
    for case in R.load_golden():
        assert set(case) == {'seed', 'F', 'B', 'C', 'T', 'overlap_thres', 'maxpool', 'sampling'}


def _prototype(name):
    src = open(os.path.join(ROOT, 'include', 'vdet_hip.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    m = re.search(r'\bint\s+%s\s*\(([^)]*)\)\s*;' % name, src)
    return [' '.join(a.split()) for a in m.group(1).split(',')]


def test_binding_matches_the_header():
    import ctypes
    from vdetlib_amd import _lib
    common = ['int64_t B', 'int64_t C', 'int T', 'const float *d_tracks', 'const int32_t *d_ntracks', 'const float *d_boxes',
              'const float *d_scores', 'const void *d_floor', 'int floor_f64', 'double overlap_thres', 'int complete', 'int window',
              'double *d_det', 'double *d_pooled', 'float *d_tboxes', 'int32_t *d_src']
    assert _prototype('vdet_rescore_tubelets') == ['vdet_ctx *ctx', 'int64_t F'] + common
    assert _prototype('vdet_rescore_tubelets_batch') == ['vdet_ctx *ctx', 'const int64_t *h_frame_off', 'int64_t V'] + common
    vp, ci, i64, f64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_double
    tail = [i64, i64, ci, vp, vp, vp, vp, vp, ci, f64, ci, ci, vp, vp, vp, vp]
    assert _lib.SYMBOLS['vdet_rescore_tubelets'] == (ci, [vp, i64] + tail)
    assert _lib.SYMBOLS['vdet_rescore_tubelets_batch'] == (ci, [vp, vp, i64] + tail)
    L = _lib.load_library()
    nul = [None] * 5 + [0, 0.7, 1, 3] + [None] * 4
    off = (ctypes.c_int64 * 2)(0, 4)
    assert L.vdet_rescore_tubelets(None, 4, 5, 2, 3, *nul) == _lib.VDET_EINVAL          # no context: refused, nothing touched
    assert L.vdet_rescore_tubelets_batch(None, off, 1, 5, 2, 3, *nul) == _lib.VDET_EINVAL
