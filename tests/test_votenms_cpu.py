"""CPU-only: ops.vote_nms_tracks / ops.vote_nms_tracks_batch (box voting on the per-frame detection lists) -- the C-ABI symbols
and prototypes, the ops signatures and every ValueError that starts no device work; hand-made lists that pin each clause of the
rule of tests/votenms_spec.py with every output written out (pins(), which test_votenms_gpu.py runs on the device); the
knife-edge pairs as two-row lists; the vote_thresh > 1 property against test_nms_tracks_cpu.expected; and the input condition
of the GPU cases: boxes move, a list keeps more than 64 rows, and the confident rows of the unsuppressed cases end up closer
to their planted objects."""
import functools
import inspect
import math
import os

import numpy as np
import pytest

import knife_spec as K
import votenms_spec as V
from test_nms_tracks_cpu import (CASES, SRC_PAD, _host_args, _oracle, _prototype, _still_with, expected as hard_expected, list_rows,
                                 same_bits, still_of)
from test_softnms_cpu import A, A2, NANBOX, ZERO_UNION, gpu_cases as soft_gpu_cases, knife_lists, one_list

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
INF = math.inf
CASE_THRESH, CASE_VOTE = 0.3, 0.5       # the settings the input condition of the generated cases is stated at
CONFIDENT = 0.5                         # "rows scoring at least 0.5": the planted objects' proposals score 0.6 .. 0.99
KEYS = ('tracks', 'score', 'src', 'box0', 'votes')


@functools.lru_cache(maxsize=None)
def gpu_cases():
    """the generated cases of the GPU file: test_softnms_cpu's four (CASES, and unsuppressed(CASES[1])), then
    unsuppressed(CASES[0]) and unsuppressed(CASES[2]).  UNSUPPRESSED names the three with every box in its keep list."""
    from test_nms_tracks_gpu import unsuppressed
    return tuple(soft_gpu_cases()) + (unsuppressed(CASES[0]), unsuppressed(CASES[2]))


UNSUPPRESSED = (4, 3, 5)                # gpu_cases()[...] = unsuppressed(CASES[0]), (CASES[1]), (CASES[2])


def case_args(case):
    return case['tracks'], case['ntracks'], case['score'], case['tboxes'], still_of(case)


@functools.lru_cache(maxsize=None)
def case_spec(k, thresh=CASE_THRESH, vote_thresh=CASE_VOTE, weights='score'):
    """the spec's result on generated case k, computed once and shared (read-only)"""
    out = V.expected(*case_args(gpu_cases()[k]), thresh=thresh, vote_thresh=vote_thresh, weights=weights)
    for v in out.values():
        v.setflags(write=False)
    return out


def outputs_equal(got, want):
    """tracks, score, src, box0 and votes by bit pattern (a NaN equal to a NaN), cnt and ntracks equal"""
    return all(same_bits(got[k], want[k]) for k in KEYS) and \
        np.array_equal(got['cnt'], want['cnt']) and np.array_equal(got['ntracks'], want['ntracks']) and \
        got['cnt'].dtype == np.int32 and got['ntracks'].dtype == np.int32 and got['votes'].dtype == np.int32


# ---- symbols, prototypes, signatures -------------------------------------------------------------------------------------
def test_symbols_and_prototypes():
    from vdetlib_amd import _lib
    hard = _prototype('vdet_nms_tracks')[2:]
    common = hard[:16] + ['double vote_thresh', 'int weights'] + hard[16:] + ['float *d_box0_out', 'int32_t *d_votes_out']
    assert hard[15] == 'int R' and len(common) == 25
    assert _prototype('vdet_vote_nms_tracks') == ['vdet_ctx *ctx', 'int64_t F'] + common
    assert _prototype('vdet_vote_nms_tracks_batch') == ['vdet_ctx *ctx', 'const int64_t *h_frame_off', 'int64_t V'] + common
    assert len(_lib.SYMBOLS['vdet_vote_nms_tracks'][1]) == 2 + len(common)
    assert len(_lib.SYMBOLS['vdet_vote_nms_tracks_batch'][1]) == 3 + len(common)
    L = _lib.load_library()
    assert hasattr(L, 'vdet_vote_nms_tracks') and hasattr(L, 'vdet_vote_nms_tracks_batch')
    hdr = open(os.path.join(ROOT, 'include', 'vdet_hip.h')).read()
    assert 'Box voting on the per-frame lists' in hdr and 'ASCENDING row index' in hdr and 'd_box0_out' in hdr


def test_ops_signatures():
    from vdetlib_amd import ops
    hard = inspect.signature(ops.nms_tracks).parameters
    p = inspect.signature(ops.vote_nms_tracks).parameters
    assert list(p) == ['tracks', 'ntracks', 'score', 'tboxes', 'still', 'thresh', 'top_still', 'cap', 'vote_thresh', 'weights', 'sync',
                       'ctx']
    assert {k: v.default for k, v in p.items() if k != 'tracks'} == \
        dict({k: v.default for k, v in hard.items() if k != 'tracks'}, vote_thresh=0.5, weights='score')
    hardb = inspect.signature(ops.nms_tracks_batch).parameters
    q = inspect.signature(ops.vote_nms_tracks_batch).parameters
    assert list(q) == ['batch_out', 'score', 'still', 'thresh', 'top_still', 'cap', 'vote_thresh', 'weights', 'use_tboxes', 'sync',
                       'ctx']
    assert {k: v.default for k, v in q.items() if k != 'batch_out'} == \
        dict({k: v.default for k, v in hardb.items() if k != 'batch_out'}, vote_thresh=0.5, weights='score')
    assert ops._VN_WEIGHTS == V.WEIGHTS
    assert {k: p[k].default for k in V.DEFAULTS} == V.DEFAULTS


VOTE_BAD = [dict(weights='iou'), dict(weights=0), dict(weights=None), dict(vote_thresh=math.nan), dict(vote_thresh=None),
            dict(vote_thresh='half')]


def test_value_errors_start_no_device_work():
    """host tensors throughout: whatever passes the checks ends at the device check, a ValueError as well"""
    import torch
    from vdetlib_amd import ops
    a = _host_args()
    z = torch.zeros
    bad = [
        dict(tracks=z(2, 3, 4, 4)), dict(tracks=z(2, 3, 4, 5, dtype=torch.float64)), dict(tracks=z(2, 3, 0, 5), score=z(2, 3, 0)),
        dict(ntracks=z(2, dtype=torch.int64)), dict(ntracks=z(3, dtype=torch.int32)), dict(ntracks=None),
        dict(score=z(2, 3, 5)), dict(score=z(2, 3, 4, dtype=torch.float16)), dict(score=None), dict(score=1),
        dict(tboxes=z(2, 3, 4, 5)), dict(tboxes=z(2, 3, 4, 4, dtype=torch.float64)),
        dict(still=a['still'][:3]), dict(still=_still_with(a, 0, z(4, 5, 5))), dict(still=_still_with(a, 0, z(3, 5, 4))),
        dict(still=_still_with(a, 0, z(4, 5, 4, dtype=torch.float64))), dict(still=_still_with(a, 1, z(4, 2, 5))),
        dict(still=_still_with(a, 2, z(4, 2, 5, dtype=torch.int64))), dict(still=_still_with(a, 2, z(4, 3, 5, dtype=torch.int32))),
        dict(still=_still_with(a, 3, z(4, 3, dtype=torch.int32))), dict(still=_still_with(a, 3, z(4, 2, dtype=torch.int64))),
        dict(still=None, top_still=2), dict(top_still=-1), dict(top_still=1022), dict(cap=0), dict(cap=1025),
        dict(still=(z(4, 40000, 4), z(4, 40000, 2), a['still'][2], a['still'][3])),
    ] + VOTE_BAD + [
        {}, dict(weights='uniform', vote_thresh=INF, thresh=-INF),      # every check passes: host tensors
    ]
    for kw in bad:
        args = dict(a, **kw)
        with pytest.raises(ValueError) as e:
            ops.vote_nms_tracks(args.pop('tracks'), args.pop('ntracks'), args.pop('score'), **args)
        assert ('same GPU' in str(e.value)) == (kw in bad[-2:]), (kw.keys(), str(e.value))
    d = dict(tracks=a['tracks'], ntracks=a['ntracks'], series=(a['score'],), tboxes=a['tboxes'])
    for kw in (dict(ntracks=a['ntracks']), dict(score=1), dict(score='pooled'), {}):
        with pytest.raises(ValueError):
            ops.vote_nms_tracks(d, **kw)
    with pytest.raises(ValueError):
        ops.vote_nms_tracks(dict(tracks=a['tracks']))
    with pytest.raises(ValueError, match="2\\^31"):
        ops.vote_nms_tracks(torch.empty(3000, 0, 1000, 5, device='meta'), torch.empty(3000, dtype=torch.int32, device='meta'),
                            torch.empty(3000, 0, 1000, device='meta'), cap=1000)


def test_batch_value_errors_start_no_device_work():
    import torch
    from vdetlib_amd import ops
    C, T = 2, 3
    off = np.array([0, 2, 5], np.int64)

    def views(per, dtype):
        flat = torch.zeros(C * T * 5 * per, dtype=dtype)
        return [flat[C * T * per * int(off[v]): C * T * per * int(off[v + 1])].view(*((C, T, int(off[v + 1] - off[v])) + ((per,) if per > 1 else ())))
                for v in range(2)]
    bo = dict(tracks=views(5, torch.float32), pooled=views(1, torch.float64), det=views(1, torch.float32), tboxes=views(4, torch.float32),
              ntracks=torch.zeros(2, C, dtype=torch.int32), frame_off=off)
    still = (torch.zeros(5, 7, 4), torch.zeros(5, 7, C), torch.zeros(5, C, 7, dtype=torch.int32), torch.zeros(5, C, dtype=torch.int32))
    bad = [
        (dict(bo, frame_off=np.array([0, 2, 2])), {}), ({k: v for k, v in bo.items() if k != 'ntracks'}, {}), (bo, dict(score='nope')),
        (dict(bo, pooled=bo['pooled'][:1]), {}), (dict(bo, tboxes=bo['tracks']), {}), (bo, dict(still=(still[0][:4],) + still[1:])),
        (bo, dict(top_still=3)), (bo, dict(still=still, top_still=1022)), (bo, dict(cap=0)),
    ] + [(bo, kw) for kw in VOTE_BAD] + [
        (bo, {}), (bo, dict(score='det', still=still, weights='uniform')),             # every check passes: host tensors
    ]
    for i, (b, kw) in enumerate(bad):
        with pytest.raises(ValueError) as e:
            ops.vote_nms_tracks_batch(b, **kw)
        assert ('same GPU' in str(e.value)) == (i >= len(bad) - 2), (i, str(e.value))


# ---- hand-made lists --------------------------------------------------------------------------------------------------------
def shifted(d):
    """box A moved by d pixels along both axes: IoU with A is (100 - d)^2 / (20000 - (100 - d)^2) -- 0.92, 0.85, 0.79 for d = 2, 4, 6"""
    return [10 + d, 10 + d, 109 + d, 109 + d]


K1, MID, K2 = [0, 0, 99, 99], [20, 0, 119, 99], [40, 0, 139, 99]         # IoU(K1, MID) = IoU(MID, K2) = 2/3, IoU(K1, K2) = 3/7
TALL, NEG = [10, 10, 109, 119], [500, 10, 399, 109]                      # areas 11000 and -10000 (A's is 10000): union(NEG, A) == 0
INFBOX = [12, 12, INF, 111]


def pins():
    """name -> (list, settings, want): want = the kept rows in rank order as src, score (f32), box (voted), box0 (own), votes;
    'cnt' where it is not the number of rows written out (a cap)"""
    q = lambda *v: [x / v[-1] for x in v[:-1]]          # float64 quotients, rounded to f32 when compared
    three = one_list((), [(A, 0.75), (shifted(2), 0.5), (shifted(4), 0.25)])
    weightless = one_list((), [(A, 0.75), (shifted(2), 0.0), (shifted(4), -0.5), (shifted(6), -0.0)])
    return {
        # a survivor and the two rows it suppressed: sw = 1.5, sx = 7.5 + 6 + 3.5 and 81.75 + 55.5 + 28.25
        'survivor_with_two_suppressed_voters': (three, dict(), dict(src=[-1], score=[0.75], box=[q(17.0, 17.0, 165.5, 165.5, 1.5)],
                                                                    box0=[A], votes=[3])),
        'uniform_weights': (three, dict(weights='uniform'), dict(src=[-1], score=[0.75], box=[shifted(2)], box0=[A], votes=[3])),
        # IoU(A, A2) == 0.5 exactly: below thresh 0.7 both are kept, at vote_thresh 0.5 they vote for each other
        'two_kept_rows_vote_for_each_other': (one_list((), [(A, 0.75), (A2, 0.25)]), dict(thresh=0.7),
                                              dict(src=[-1, -2], score=[0.75, 0.25], box=[[10, 10, 109, 96.5]] * 2, box0=[A, A2], votes=[2, 2])),
        'vote_thresh_just_above_the_overlap': (one_list((), [(A, 0.75), (A2, 0.25)]), dict(thresh=0.7, vote_thresh=np.nextafter(0.5, 1.0)),
                                               dict(src=[-1, -2], score=[0.75, 0.25], box=[A, A2], box0=[A, A2], votes=[1, 1])),
        # MID is suppressed by K1 and votes for K1 AND for K2, which K1 does not reach
        'voter_suppressed_by_another_survivor': (one_list((), [(K1, 0.75), (MID, 0.25), (K2, 0.5)]), dict(),
                                                 dict(src=[-1, -3], score=[0.75, 0.5], box=[[5, 0, 104, 99], q(25.0, 0.0, 99.25, 74.25, 0.75)],
                                                      box0=[K1, K2], votes=[2, 2])),
        # 0.0, a negative score and -0.0 weigh nothing under 'score' and are still counted ...
        'zero_and_negative_voters': (weightless, dict(), dict(src=[-1], score=[0.75], box=[A], box0=[A], votes=[4])),
        'zero_and_negative_voters_uniform': (weightless, dict(weights='uniform'),
                                             dict(src=[-1], score=[0.75], box=[shifted(3)], box0=[A], votes=[4])),
        # ... and where every weight is zero the own box stays
        'all_weights_zero': (one_list((), [(A, 0.0), (shifted(2), -0.25)]), dict(), dict(src=[-1], score=[0.0], box=[A], box0=[A], votes=[2])),
        # sw = inf, sx = inf: NaN quotients, the own box stays
        'infinite_score': (one_list((), [(A, INF), (shifted(2), 0.5)]), dict(), dict(src=[-1], score=[INF], box=[A], box0=[A], votes=[2])),
        # an infinite coordinate: ovr == 0 against A (no suppression, no vote); the row's own quotient is inf, the own box stays
        'infinite_coordinate': (one_list((), [(A, 0.75), (INFBOX, 0.5)]), dict(),
                                dict(src=[-1, -2], score=[0.75, 0.5], box=[A, INFBOX], box0=[A, INFBOX], votes=[1, 1])),
        # a NaN coordinate in a still-image row: every ovr with it is NaN -- kept, no voter, and its own mean is NaN
        'nan_coordinate_in_a_still_row': (one_list([(NANBOX, 0.75), (A, 0.5)], [(shifted(2), 0.25)]), dict(),
                                          dict(src=[0, 1], score=[0.75, 0.5], box=[NANBOX, q(5.0 + 3.0, 5.0 + 3.0, 54.5 + 27.75, 54.5 + 27.75, 0.75)],
                                               box0=[NANBOX, A], votes=[1, 2])),
        # union(NEG, A) == 0, and A is suppressed by TALL before NEG is kept: the NMS never evaluates the pair, the voting pass
        # meets it and must raise nothing
        'zero_union_met_by_the_voting_pass_only': (one_list((), [(TALL, 0.75), (A, 0.5), (NEG, 0.25)]), dict(),
                                                   dict(src=[-1, -3], score=[0.75, 0.25], box=[[10, 10, 109, 115], NEG], box0=[TALL, NEG],
                                                        votes=[2, 1])),
        # equal f32 scores, a still-image row and a tubelet row: the tubelet row (the higher index) is kept, the sums still run
        # in ascending row index
        'tie_still_tubelet': (one_list([(A, 0.75)], [(shifted(2), 0.75)]), dict(),
                              dict(src=[-1], score=[0.75], box=[shifted(1)], box0=[shifted(2)], votes=[2])),
        # float64 scores that round to 0.0f: a tie in f32 (the higher row is kept) and NO weight -- with the float64 values as
        # weights the box would be the mean, shifted(2)
        'f64_scores_that_round_to_zero_in_f32': (one_list((), [(A, 1e-60), (shifted(4), 1e-60)]), dict(),
                                                 dict(src=[-2], score=[0.0], box=[shifted(4)], box0=[shifted(4)], votes=[2])),
        # ... and one that rounds DOWN to 0.75f: the weights are 0.75 and 0.25 exactly
        'f64_score_rounded_to_f32_is_the_weight': (one_list((), [(A, np.nextafter(0.75, 1.0)), (shifted(4), 0.25)]), dict(),
                                                   dict(src=[-1], score=[0.75], box=[shifted(1)], box0=[A], votes=[2])),
        # three kept rows, two output rows: the count stays, nothing past the cap
        'cap_below_the_count': (one_list((), [(K1, 0.75), (MID, 0.25), (K2, 0.5)]), dict(thresh=0.7, cap=2),
                                dict(src=[-1, -3], score=[0.75, 0.5], box=[[5, 0, 104, 99], q(25.0, 0.0, 99.25, 74.25, 0.75)], box0=[K1, K2],
                                     votes=[2, 2], cnt=3)),
    }


def run_spec(lst, **kw):
    kw = dict(kw)
    return V.expected(lst['tracks'], lst['ntracks'], lst['score'], None, lst['still'], R=kw.pop('cap', None), **kw)


def pin_matches(out, want):
    """every output of a C = F = 1 result against the written-out rows"""
    n = len(want['src'])
    cnt = want.get('cnt', n)
    f32 = lambda x: np.array(x, np.float64).astype(F32)
    return out['cnt'].tolist() == [[cnt]] and out['ntracks'].tolist() == [n] and \
        out['src'][0, :n, 0].tolist() == want['src'] and (out['src'][0, n:, 0] == SRC_PAD).all() and \
        same_bits(out['tracks'][0, :n, 0, 4], f32(want['score'])) and same_bits(out['tracks'][0, :n, 0, :4], f32(want['box'])) and \
        same_bits(out['box0'][0, :n, 0], f32(want['box0'])) and out['votes'][0, :n, 0].tolist() == want['votes'] and \
        np.isnan(out['tracks'][0, n:]).all() and np.isnan(out['score'][0, n:]).all() and np.isnan(out['box0'][0, n:]).all() and \
        (out['votes'][0, n:] == 0).all()


@pytest.mark.parametrize("name", sorted(pins()))
def test_hand_made_lists(name):
    lst, kw, want = pins()[name]
    out = run_spec(lst, **kw)
    assert pin_matches(out, want), {k: out[k][0, :, 0].tolist() for k in ('tracks', 'box0', 'votes', 'src')}
    n = len(want['src'])
    rows = list_rows(0, 0, lst['tracks'], lst['ntracks'], lst['score'], None, lst['still'])
    by_src = {int(s): s64 for _, s64, s in zip(*rows)}
    assert out['score'][0, :n, 0].tolist() == [by_src[s] for s in want['src']]               # the source's own unrounded score


def test_zero_union_of_the_nms_raises():
    """a zero-union pair the hard NMS evaluates raises as nms_tracks does, whatever the vote settings"""
    for kw in (dict(), dict(vote_thresh=1.5), dict(weights='uniform')):
        with pytest.raises(ZeroDivisionError):
            run_spec(ZERO_UNION, **kw)
    lst = dict(ZERO_UNION, score=np.array([[[0.9], [np.nan], [0.5]]]))       # the NaN-scored one is no row: nothing is evaluated
    assert run_spec(lst)['cnt'].tolist() == [[2]]


def test_sums_are_the_sequential_loop():
    """np.cumsum in vote() against the rule's own loop, statement by statement, on the longest lists of a generated case"""
    case = gpu_cases()[3]
    o = _oracle()
    checked = 0
    for c, f in ((0, 0), (0, 1), (1, 0), (1, 1)):
        dets, _, _ = list_rows(c, f, *case_args(case))
        keep = list(o.nms(dets, CASE_THRESH))
        for weights in V.WEIGHTS:
            voted, votes = V.vote(dets, keep, CASE_VOTE, weights)
            w = V.weights_of(dets, weights)
            for r, i in enumerate(keep):
                sw, sx = 0.0, [0.0] * 4
                idx = V.voters(dets, i, CASE_VOTE)
                for j in idx:
                    sw += float(w[j])
                    for k in range(4):
                        sx[k] += float(w[j]) * float(dets[j, k])
                want = np.array([x / sw for x in sx]).astype(F32) if sw > 0 else dets[i, :4]
                assert same_bits(voted[r], want) and votes[r] == len(idx)
                checked += len(idx) > 2
    assert checked > 20


@pytest.mark.parametrize("t", K.THRESHOLDS)
def test_overlap_exactly_at_the_vote_threshold(t):
    """the knife-edge pairs as two-row lists, nothing suppressed (thresh = 1.5): both rows count two voters iff the reference's
    nms suppresses the pair at that threshold"""
    o = _oracle()
    tracks, nt, score = knife_lists(t)
    out = V.expected(tracks, nt, score, thresh=1.5, vote_thresh=t)
    assert (out['cnt'] == 2).all() and (out['src'][0, 0] == -2).all() and (out['src'][0, 1] == -1).all()
    hard = np.array([len(o.nms(np.concatenate([tracks[0, ::-1, f, :4], [[0.9], [0.5]]], 1).astype(F32), t)) == 1
                     for f in range(tracks.shape[2])])
    assert np.array_equal(out['votes'][0, 0] == 2, hard) and np.array_equal(out['votes'][0, 1] == 2, hard)
    assert ((out['votes'] == 1) | (out['votes'] == 2)).all() and hard.any() and not hard.all()


# ---- cross-check against the hard NMS ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(6))
def test_no_voter_but_the_row_itself_is_the_hard_nms(k):
    """vote_thresh = 1.5: every output nms_tracks also has equals test_nms_tracks_cpu.expected bit for bit, both weights"""
    want = hard_expected(*case_args(gpu_cases()[k]), thresh=CASE_THRESH)
    for weights in V.WEIGHTS:
        out = case_spec(k, CASE_THRESH, 1.5, weights)
        live = out['src'] != SRC_PAD
        # (under 'score' a row whose score is <= 0 weighs nothing and keeps its own box: the same bits again)
        assert all(same_bits(out[key], want[key]) for key in ('tracks', 'score', 'src'))
        assert np.array_equal(out['cnt'], want['cnt']) and np.array_equal(out['ntracks'], want['ntracks'])
        assert same_bits(out['box0'], want['tracks'][..., :4]) and (out['votes'][live] == 1).all() and (out['votes'][~live] == 0).all()
        assert live.sum() == min(want['cnt'].sum(), live.size) > 0


# ---- the input condition of the GPU cases -------------------------------------------------------------------------------------
def moved_rows(out):
    """the kept rows whose voted box is no longer their own box, by bit pattern"""
    live = out['src'] != SRC_PAD
    return live & (out['tracks'][..., :4].view(np.uint32) != out['box0'].view(np.uint32)).any(-1)


def planted_iou(case, boxes, c, f):
    """[m,4] boxes of list (c, f) -> the IoU (+1 areas, float64) of each with the nearest planted object of class c + 1"""
    gts = [t['bbox'] for a in case['annot']['annotations'] for t in a['track'] if t['frame'] == f + 1 and t['class_index'] == c + 1]
    best = np.zeros(len(boxes))
    b = boxes.astype(np.float64)
    for g in gts:
        w = np.maximum(0.0, np.minimum(b[:, 2], g[2]) - np.maximum(b[:, 0], g[0]) + 1)
        h = np.maximum(0.0, np.minimum(b[:, 3], g[3]) - np.maximum(b[:, 1], g[1]) + 1)
        inter = w * h
        uni = (b[:, 2] - b[:, 0] + 1) * (b[:, 3] - b[:, 1] + 1) + (g[2] - g[0] + 1) * (g[3] - g[1] + 1) - inter
        best = np.maximum(best, inter / uni)
    return best


def confident_iou(case, out):
    """(rows, mean IoU of the own boxes, mean IoU of the voted boxes, rows better, rows worse) over the kept rows scoring >= 0.5"""
    before, after = [], []
    C, R, F = out['src'].shape
    for c in range(C):
        for f in range(F):
            rows = np.flatnonzero((out['src'][c, :, f] != SRC_PAD) & (out['tracks'][c, :, f, 4] >= F32(CONFIDENT)))
            before += planted_iou(case, out['box0'][c, rows, f], c, f).tolist()
            after += planted_iou(case, out['tracks'][c, rows, f, :4], c, f).tolist()
    before, after = np.array(before), np.array(after)
    return len(before), before.mean(), after.mean(), int((after > before).sum()), int((after < before).sum())


@pytest.mark.parametrize("k", range(6))
def test_generated_cases_move_boxes(k):
    out = case_spec(k)                                   # (raises ZeroDivisionError: the condition "no zero union in the NMS")
    moved, most = int(moved_rows(out).sum()), int(out['cnt'].max())
    live = out['src'] != SRC_PAD
    print("case %d: %d kept rows, %d moved, at most %d kept in a list, %.2f voters per kept row"
          % (k, live.sum(), moved, most, out['votes'][live].mean()))
    assert moved >= 30
    assert (out['votes'][live] >= 1).all() and (out['votes'][live] > 1).any()


def test_a_generated_list_keeps_more_than_64_rows():
    """the second pass of the voting loop (ranks 64 ...) runs on at least one case"""
    assert max(int(case_spec(k)['cnt'].max()) for k in range(6)) > 64


@pytest.mark.parametrize("weights", V.WEIGHTS)
@pytest.mark.parametrize("k", UNSUPPRESSED)
def test_voting_moves_confident_rows_towards_the_planted_objects(k, weights):
    out = case_spec(k, CASE_THRESH, CASE_VOTE, weights)
    n, before, after, better, worse = confident_iou(gpu_cases()[k], out)
    print("case %d, %r: %d rows scoring >= %.1f, mean IoU with the planted object %.4f -> %.4f (%d better, %d worse)"
          % (k, weights, n, CONFIDENT, before, after, better, worse))
    assert n > 0 and after > before
