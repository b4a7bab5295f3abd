"""The counting sort's key -> bin map (csrc/binsort_kernels.hpp, phases 2 and 3) as a numpy model: a map built from list A
and applied to list B -- what a workgroup does when it passes the map of the list it sorted before on to the next one.  The
order the kernel produces does not depend on the map as long as the map is monotone, keeps exponent values in bins of their
own and gives fractions that never contradict the keys inside a bin; phase 6 settles everything else from the full keys.
The second property needs the floor of phase 2 (every exponent value gets at least one sub-bin): the planted case shows that
the model sees the hazard without it."""
import itertools

import numpy as np
import pytest

from temporal_cases import score_key

N = 4500
BIN_TOTAL = 4 * 4096            # binsort_words(20) counter words, four byte-wide bins each
BIN_SUB = BIN_TOTAL - 512       # handed out proportionally; the rest is the floor's


def make(kind, rng, n=N):
    if kind == "uniform":
        return rng.random(n, dtype=np.float32)
    if kind == "normal":
        return rng.standard_normal(n).astype(np.float32)
    if kind == "softmax":
        return np.exp(-rng.exponential(6.0, n)).astype(np.float32)
    if kind == "octave":            # a single octave
        return (0.5 + 0.5 * rng.random(n, dtype=np.float32)).astype(np.float32)
    if kind == "sparse_exp":        # test_argsort_gpu.py's recipe: a handful of keys in far-away octaves
        s = rng.random(n, dtype=np.float32)
        for j in range(8):
            s[j * 7] = np.float32(2.0 ** -40) * np.float32(1.0 + j * 2.0 ** -23)
            s[j * 7 + 1] = -np.float32(2.0 ** 30) * np.float32(1.0 + (j % 3) * 2.0 ** -23)
        return s
    raise ValueError(kind)


KINDS = ["uniform", "normal", "softmax", "octave", "sparse_exp"]


def inverted_keys(scores):
    return (~score_key(scores)).astype(np.uint32)           # ascending inverted key = descending score


def build_map(ikeys, floor=True):
    """phase 2: (first bin, sub-bins) per exponent value (the inverted key's top 9 bits)"""
    n = len(ikeys)
    cnt = np.bincount(ikeys >> 23, minlength=512).astype(np.int64)
    m = (cnt * BIN_SUB + n - 1) // n
    if floor:
        m = np.maximum(m, 1)
    first = np.cumsum(m) - m
    assert first[-1] + m[-1] <= BIN_TOTAL
    return first, m


def apply_map(ikeys, first, m):
    """phase 3: bin and 16-bit fraction of every key"""
    e = ikeys >> 23
    prod = (ikeys & 0x7FFFFF).astype(np.int64) * m[e]
    return first[e] + (prod >> 23), (prod >> 7) & 0xFFFF


def check(ikeys, first, m):
    """-> (monotone, one exponent value per bin, fractions agree with keys)"""
    o = np.argsort(ikeys, kind="stable")
    k = ikeys[o]
    b, fr = apply_map(k, first, m)
    monotone = bool(np.all(np.diff(b) >= 0))
    same_bin = b[1:] == b[:-1]
    one_exp = bool(np.all((k[1:] >> 23)[same_bin] == (k[:-1] >> 23)[same_bin]))
    # inside a bin (sorted by key): the fraction never decreases, so a smaller fraction always means a smaller key
    frac_ok = bool(np.all(fr[1:][same_bin] >= fr[:-1][same_bin]))
    return monotone, one_exp, frac_ok


@pytest.mark.parametrize("ka,kb", list(itertools.product(KINDS, KINDS)))
def test_a_map_built_from_one_list_orders_another(ka, kb):
    rng = np.random.default_rng(KINDS.index(ka) * 7 + KINDS.index(kb) + 1)
    a, b = inverted_keys(make(ka, rng)), inverted_keys(make(kb, rng))
    first, m = build_map(a)
    assert np.all(m >= 1) and first[-1] + m[-1] <= BIN_TOTAL
    assert check(b, first, m) == (True, True, True)
    assert check(a, first, m) == (True, True, True)


def planted(rng, n=512):
    """GPU test 3's pair: a U(0.5, 1) list, then one that also holds keys in octaves the first does not have"""
    a = (0.5 + 0.5 * rng.random(n, dtype=np.float32)).astype(np.float32)
    b = (0.5 + 0.5 * rng.random(n, dtype=np.float32)).astype(np.float32)
    for j in range(9):
        b[j * 5] = np.float32(2.0 ** -40) * np.float32(1.0 + j * 2.0 ** -23)
        b[j * 5 + 1] = -np.float32(2.0 ** 30)
    return a, b


def test_the_floor_is_what_keeps_absent_octaves_apart():
    a, b = planted(np.random.default_rng(3))
    ia, ib = inverted_keys(a), inverted_keys(b)
    assert check(ib, *build_map(ia)) == (True, True, True)
    monotone, one_exp, _ = check(ib, *build_map(ia, floor=False))
    assert monotone and not one_exp, "without the floor the absent octaves share a bin: the model must see it"
    # a list's own map never needed the floor (a value without keys has no bin to share)
    assert check(ib, *build_map(ib, floor=False)) == (True, True, True)
