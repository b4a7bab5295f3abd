"""The counting sort's inherited key -> bin map (csrc/binsort_kernels.hpp): a workgroup sorts a list with the map of the list it
sorted before, builds the list's own map again where that one does not fit (a redo, then a back-off), and does not pass a
crowded map on.  Everything goes through ``ops.argsort_volume`` and is compared with the order ``test_argsort_gpu.py`` uses
(descending key, ties by descending index), at B = 1 025 (8 keys per thread: the counting sort takes frames of more than 1 024
boxes, smaller ones go to the LSD kernels) and B = 4 500 (20), for both key forms: float rows (layout FCB) and sortable keys
(layout FBC: the key format of the volume pass).  With VDET_BINSORT_GRID=1 one workgroup sorts
the lists in order (list p = f * C + c), so the tests decide which list follows which; vdet_query 16 / 17 / 9 count the lists
sorted with an inherited map / sorted again with their own / handed to the LSD kernel."""
import os

import numpy as np
import pytest
import torch

from temporal_cases import expected
from vdetlib_amd import ops, _lib
from test_argsort_gpu import make as make_volume

pytestmark = pytest.mark.gpu

_ctxs = {}


def ctx_for(grid, inherit=True):
    """one context per setting (the switches are read when the context is created)"""
    key = (grid, inherit)
    if key not in _ctxs:
        want = {"VDET_BINSORT": "1", "VDET_BINSORT_INHERIT": "1" if inherit else "0",
                "VDET_BINSORT_GRID": None if grid is None else str(grid)}
        old = {k: os.environ.get(k) for k in want}
        for k, v in want.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        try:
            _ctxs[key] = _lib.Context(torch.cuda.current_device())
        finally:
            for k, v in old.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v
    return _ctxs[key]


def run(lists, form, grid=1, inherit=True, F=1):
    """lists [P, B] float32 (list p = f * C + c) -> order [P, B], (query 16, query 17, query 9)"""
    P, B = lists.shape
    vol = torch.from_numpy(np.ascontiguousarray(lists.reshape(F, P // F, B))).cuda()      # [F, C, B] float rows
    if form == "keys":
        vol = vol.permute(0, 2, 1).contiguous()                                           # [F, B, C]: sorted from keys
    ctx = ctx_for(grid, inherit)
    o, n = ops.argsort_volume(vol, layout="FCB" if form == "floats" else "FBC", ctx=ctx)
    q = (ctx.query(16), ctx.query(17), ctx.query(9))
    assert bool((n == B).all())
    return (o.cpu().numpy().astype(np.int64) & 0xFFFF).reshape(P, B), q


def reference(lists):
    eo, _ = expected(np.ascontiguousarray(lists.T)[None])        # [1, B, P] -> [1, P, B]
    return eo[0]


def draw(kind, rng, B):
    if kind == "high":                       # one octave
        return (0.5 + 0.5 * rng.random(B, dtype=np.float32)).astype(np.float32)
    if kind == "tiny":                       # another one, far away
        return (np.float32(2.0 ** -20) * (1.0 + rng.random(B, dtype=np.float32))).astype(np.float32)
    if kind == "negative":                   # and one on the other side of zero
        return (-(1.0 + rng.random(B, dtype=np.float32))).astype(np.float32)
    if kind == "narrow":                     # 1 / 32 of an octave
        return (0.5 + np.float32(2.0 ** -6) * rng.random(B, dtype=np.float32)).astype(np.float32)
    if kind == "narrow16":                   # 1 / 16
        return (0.5 + np.float32(2.0 ** -5) * rng.random(B, dtype=np.float32)).astype(np.float32)
    if kind == "quantised":                  # 65 distinct values: no map spreads them
        return (np.round(rng.random(B, dtype=np.float32) * 64) / 64).astype(np.float32)
    if kind == "constant":                   # (a padded frame looks like this)
        return np.full(B, -np.inf, dtype=np.float32)
    return make_volume(kind, rng, 1, B, 1)[0, :, 0]              # test_argsort_gpu.py's recipes


def stack(kinds, rng, B):
    return np.stack([draw(k, rng, B) for k in kinds]).astype(np.float32)


SHAPES = [(1025, "floats"), (1025, "keys"), (4500, "floats"), (4500, "keys")]


@pytest.mark.parametrize("kind", ["uniform", "normal"])
@pytest.mark.parametrize("B,form", SHAPES)
def test_lists_of_one_distribution_inherit_the_first_map(B, form, kind):
    lists = stack([kind] * 24, np.random.default_rng(B + len(kind)), B)
    o, q = run(lists, form)
    assert np.array_equal(o, reference(lists))
    assert q == (23, 0, 0)


@pytest.mark.parametrize("B,form", SHAPES)
def test_disjoint_exponent_ranges_are_redone_and_back_off(B, form):
    lists = stack(["high", "tiny", "negative"] * 8, np.random.default_rng(B + 1), B)
    o, (inherited, redone, lsd) = run(lists, form)
    assert np.array_equal(o, reference(lists))
    assert redone > 0
    assert inherited + redone < 23, "after a redo the next lists build their own maps without trying the inherited one"
    assert lsd == 0, "a list that does not fit the inherited map is not the LSD kernel's business"


@pytest.mark.parametrize("B,form", SHAPES)
def test_octaves_absent_from_the_inherited_map_keep_bins_of_their_own(B, form):
    """the m = 0 hazard: without the floor of phase 2 the two planted octaves would share a bin and come out in the wrong order"""
    rng = np.random.default_rng(B + 2)
    lists = stack(["high", "high"], rng, B)
    for j in range(9):                       # (fewer than kBinMax keys per planted octave: each fills ONE bin)
        lists[1, j * 5] = np.float32(2.0 ** -40) * np.float32(1.0 + j * 2.0 ** -23)
        lists[1, j * 5 + 1] = -np.float32(2.0 ** 30)
    o, q = run(lists, form)
    assert np.array_equal(o, reference(lists))
    assert q == (1, 0, 0)


@pytest.mark.parametrize("B,form", SHAPES)
def test_lists_for_the_lsd_kernel_between_normal_ones(B, form):
    """Two lists that no map spreads -- quantised scores and a constant list -- each between normal lists; the `dups` recipe
    (pairs of equal keys: two to a bin) is a normal list.  Query 9 counts the two.  (Through argsort_volume every key of the
    counting sort's lists is a candidate -- thresholds take the LSD kernel from the start, NaN is a key like any other -- so an
    excluded key, which the kernel hands over the same way, cannot be planted from here.)"""
    lists = stack(["uniform", "quantised", "uniform", "dups", "constant", "uniform", "nonfinite"], np.random.default_rng(B + 3), B)
    o, (inherited, redone, lsd) = run(lists, form)
    assert np.array_equal(o, reference(lists))
    assert lsd == 2


_mixed = {}


def mixed(B):
    if B not in _mixed:
        rng = np.random.default_rng(B + 4)
        kinds = ["uniform", "normal", "softmax", "octaves", "sparse_exp", "dups", "high", "tiny", "negative", "narrow"]
        lists = stack([kinds[i] for i in rng.integers(0, len(kinds), 1200)], rng, B)
        _mixed[B] = (lists, reference(lists))
    return _mixed[B]


@pytest.mark.parametrize("B,form", SHAPES)
def test_mixed_lists_on_the_default_grid(B, form):
    """1 200 lists (4 frames x 300 classes), more than the resident workgroups: inheriting on and off give the same, exact lists.
    (The narrow lists do not spread under a map of their own either -- a map is linear inside an octave -- so some lists go to
    the LSD kernel in both runs; inheriting adds none: a list whose inherited map overflows is sorted again with its own.)"""
    lists, ref = mixed(B)
    o1, (inherited, redone, lsd) = run(lists, form, grid=None, inherit=True, F=4)
    o0, (inherited0, redone0, lsd0) = run(lists, form, grid=None, inherit=False, F=4)
    assert np.array_equal(o1, ref) and np.array_equal(o0, ref)
    assert (inherited0, redone0) == (0, 0)
    assert lsd <= lsd0
    assert inherited > 0 and redone > 0


@pytest.mark.parametrize("B,form", SHAPES)
def test_the_list_after_a_list_the_map_did_not_fit_does_not_inherit(B, form):
    """A list of 1 / 32 of an octave after a U(0, 1) list, then another U(0, 1) list.  Under the inherited map the narrow list has
    ~4 (B = 1 025) or ~18 (B = 4 500) keys per bin: it finishes crowded, or is sorted again with its own map, or -- its own map
    overflows too at B = 4 500 -- goes to the LSD kernel.  Whichever it is, exactly ONE list took the inherited map: the third
    list builds its own."""
    lists = stack(["uniform", "narrow", "uniform"], np.random.default_rng(B + 5), B)
    o, (inherited, redone, lsd) = run(lists, form)
    assert np.array_equal(o, reference(lists))
    assert inherited + redone + lsd == 1


@pytest.mark.parametrize("form", ["floats", "keys"])
def test_a_crowded_map_is_not_passed_on(form):
    """The crowding rule alone: 1 / 16 of an octave, B = 1 025, after a U(0, 1) list whose map gives that range ~500 bins: ~2 keys
    per bin (Poisson: ~110 keys at rank >= 3 against the limit of B / 32 = 32; a bin of more than 10 keys has probability 1e-5),
    so the list finishes under the inherited map, the next one must build its own, and the one after that inherits again."""
    B = 1025
    lists = stack(["uniform", "narrow16", "uniform", "uniform"], np.random.default_rng(B + 6), B)
    o, q = run(lists, form)
    assert np.array_equal(o, reference(lists))
    assert q == (2, 0, 0)
