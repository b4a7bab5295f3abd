"""Seq-NMS without a GPU: the numpy rule (tests/seqnms_spec.py) against a hand-worked example, an exhaustive search and its own
invariants, and the binding -- prototypes, signatures, and every ValueError of ops.seq_nms / ops.seq_nms_batch raised before any
device work (host tensors throughout)."""
import inspect
import os

import numpy as np
import pytest

import seqnms_cases as sc
import seqnms_spec as spec
import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
NAN, NONE = np.nan, spec.NO_NODE


# ---- the hand-worked example: three lanes of 10 x 10 boxes that never overlap each other; a box links to the same lane only
A, B, C_, X = (0, 0, 9, 9), (100, 0, 109, 9), (200, 0, 209, 9), (NAN,) * 4
HAND_BOX = [[A, B, A, C_],           # row 0, frames 0 .. 3
            [A, A, B, B],            # row 1
            [B, X, C_, A]]           # row 2
HAND_S = [[1.0, 0.5, 1.0, -1.0],
          [1.0, 2.0, 3.0, 0.5],
          [0.5, 9.0, 4.5, 0.5]]


def hand_tracks():
    return np.concatenate([np.array(HAND_BOX, F32), np.array(HAND_S, F32)[..., None]], 2)


def test_hand_worked_example():
    """Round 0: best is 4.5 at (frame 2, row 2) -- alone in lane C -- and at (3, 1) and (3, 2), the ends of lanes B and A: the
    lowest FRAME wins, sequence 0 is that one node.  Round 1: (3, 1) and (3, 2) tie at 4.5 in one frame: the lowest SLOT wins,
    lane B = (0,2) (1,0) (2,1) (3,1), 0.5 + 0.5 + 3.0 + 0.5.  Round 2: lane A; its node (1, 1) has two predecessors with best
    1.0, rows 0 and 1 of frame 0: the lowest takes it, the other -- an identical box -- is suppressed.  Round 3: what is left
    is (3, 0) with -1.0 < min_score: a leftover, not exhausted."""
    out = spec.seq_nms(hand_tracks(), 3, link_thres=0.5, nms_thres=0.3, rescore='avg', max_seqs=5, min_score=-0.5)
    assert out['nseq'] == 3 and out['ntracks'] == 3 and out['exhausted'] == 0
    assert np.array_equal(out['seq'], np.array([[2, 1, 2, -1], [-2, 2, 1, 1], [1, NONE, 0, 2]], np.int32))
    want = np.array([[1.125, 1.125, 1.125, -1.0], [NAN, 1.125, 1.125, 1.125], [1.125, NAN, 4.5, 1.125]])
    assert np.array_equal(out['score'], want, equal_nan=True)
    assert np.array_equal(out['seq_sum'], [4.5, 4.5, 4.5, NAN, NAN], equal_nan=True)
    assert np.array_equal(out['seq_len'], [1, 4, 4, 0, 0])
    assert np.array_equal(out['seq_end'], [[2, 2], [3, 1], [3, 2], [-1, -1], [-1, -1]])
    t = hand_tracks()
    t[..., 4] = want
    t[np.isnan(want)] = NAN
    assert np.array_equal(out['tracks'], t, equal_nan=True) and out['tracks'].dtype == F32
    assert out['score'].dtype == np.float64 and out['seq'].dtype == np.int32 and out['seq_len'].dtype == np.int32
    # 'max': the largest old score of each sequence; one more round allowed takes the last node and exhausts the class
    out = spec.seq_nms(hand_tracks(), 3, rescore='max', max_seqs=5)
    want = np.array([[2.0, 3.0, 2.0, -1.0], [NAN, 2.0, 3.0, 3.0], [3.0, NAN, 4.5, 2.0]])
    assert np.array_equal(out['score'], want, equal_nan=True)
    assert out['nseq'] == 4 and out['exhausted'] == 1 and out['seq'][0, 3] == 3
    assert np.array_equal(out['seq_sum'], [4.5, 4.5, 4.5, -1.0, NAN], equal_nan=True)
    # ntracks cuts rows off: row 2 is no node, lane B starts in frame 1
    out = spec.seq_nms(hand_tracks(), 2, max_seqs=5)
    assert (out['seq'][2] == NONE).all() and out['ntracks'] == 2
    assert np.array_equal(out['seq_sum'][:2], [4.0, 4.0]) and np.array_equal(out['seq_end'][:2], [[2, 0], [3, 1]])


def brute_case(seed):
    boxes, scores = synth.coherent_video(seed, 5, 3, 1, jitter=25)
    t = np.concatenate([boxes.transpose(1, 0, 2), scores.transpose(1, 0, 2)], 2).astype(F32)          # [R,F,5]
    if seed % 2:
        t[..., 4] -= F32(0.4)
    t[np.random.RandomState(1000 + seed).rand(3, 5) < 0.15] = NAN
    return t


def test_first_sequence_is_the_best_of_all_linked_paths():
    neg = 0
    for seed in range(40):
        t = brute_case(seed)
        neg += int((t[..., 4] < 0).any())
        out = spec.seq_nms(t, 3, link_thres=0.3, max_seqs=1)
        assert out['nseq'] == 1
        assert out['seq_sum'][0] == spec.best_path_brute(t, 3, link_thres=0.3), seed
    assert neg >= 15                 # negative scores do occur


INVARIANT_CASES = ('tie_free', 'all_equal', 'mixed_sign_zeros', 'no_nodes_col4', 'no_nodes_f32', 'empty_middle_frame', 'R33_all',
                   'R65_few', 'F3', 'link0_avg', 'max_seqs_10_of_11')


@pytest.mark.parametrize('name', INVARIANT_CASES)
def test_invariants(name):
    c = sc.case(name)
    kw = c['kw']
    out = sc.expect(c)
    lt, nt = kw.get('link_thres', 0.5), kw.get('nms_thres', 0.3)
    for ci in range(len(c['tracks'])):
        t, seq = c['tracks'][ci], out['seq'][ci]
        node, s, _ = spec.nodes_of(t, c['ntracks'][ci], None if c['score'] is None else c['score'][ci])
        assert np.array_equal(seq != NONE, node)
        n = int(out['nseq'][ci])
        for k in range(n):
            rows, frames = np.nonzero(seq == k)
            order = np.argsort(frames)
            rows, frames = rows[order], frames[order]
            # consecutive frames, one member per frame, each linked to the next; the table describes it
            assert np.array_equal(frames, np.arange(frames[0], frames[0] + len(frames)))
            assert len(frames) == out['seq_len'][ci, k] and tuple(out['seq_end'][ci, k]) == (frames[-1], rows[-1])
            for a in range(len(frames) - 1):
                assert spec.hit_matrix(t[rows[a], frames[a], None, :4], t[rows[a + 1], frames[a + 1], None, :4], lt)[0, 0]
            # left to right, the sum; and the new score
            total = s[rows[0], frames[0]]
            for a in range(1, len(frames)):
                total = total + s[rows[a], frames[a]]
            assert total == out['seq_sum'][ci, k]
            new = total / len(frames) if kw.get('rescore', 'avg') == 'avg' else s[rows, frames].max()
            assert (out['score'][ci][rows, frames] == new).all()
            old = s[rows, frames]
            assert old.min() <= new <= old.max()
            # nothing that survived in a member's frame hits it, if it belongs to a later round or to none
            for r, f in zip(rows, frames):
                later = (seq[:, f] > k) | (seq[:, f] == spec.LEFTOVER)
                assert not (spec.hit_matrix(t[r, f, None, :4], t[:, f, :4], nt)[0] & later).any()
        assert bool(out['exhausted'][ci]) == (not (seq == spec.LEFTOVER).any())
        left = seq == spec.LEFTOVER
        assert np.array_equal(out['score'][ci][left], s[left])
        gone = seq < spec.LEFTOVER
        assert np.isnan(out['score'][ci][gone]).all() and np.isnan(out['tracks'][ci][gone]).all()
        assert np.array_equal(out['tracks'][ci][~gone][:, :4], t[~gone][:, :4])
        assert np.array_equal(out['tracks'][ci][~gone][:, 4], out['score'][ci][~gone].astype(F32))
        assert np.isnan(out['seq_sum'][ci, n:]).all() and (out['seq_len'][ci, n:] == 0).all() and (out['seq_end'][ci, n:] == -1).all()


def test_sums_do_not_increase_while_nothing_is_suppressed():
    """nms_thres > 1 suppresses nothing (a quotient is at most 1), so a round removes its own path and nothing else: every
    path of a later round was there before with the same left-to-right sum, and the sums cannot grow."""
    for name in ('tie_free', 'mixed_sign_zeros', 'no_nodes_col4'):
        c = sc.case(name)
        out = sc.expect(c, nms_thres=1.5, max_seqs=4096)
        assert out['exhausted'].all() and not (out['seq'] == spec.SUPPRESSED).any()
        for ci in range(len(c['tracks'])):
            sums = out['seq_sum'][ci, :out['nseq'][ci]]
            assert (np.diff(sums) <= 0).all()


def test_a_shorter_run_is_a_prefix_of_a_longer_one():
    c = sc.case('tie_free')
    full = sc.expect(c, max_seqs=64)
    for n in (1, 2, 7, 20):
        part = sc.expect(c, max_seqs=n)
        assert (part['nseq'] == n).all()
        assert np.array_equal(part['seq_sum'], full['seq_sum'][:, :n]) and np.array_equal(part['seq_end'], full['seq_end'][:, :n])
        for k in range(n):
            assert np.array_equal(part['seq'] == k, full['seq'] == k)
        member = part['seq'] >= 0
        assert np.array_equal(part['score'][member], full['score'][member])


def planted():
    boxes, scores, annot = synth.vid_with_objects(7, 12, 40, 3)
    C, (F, B) = scores.shape[2], boxes.shape[:2]
    t = np.empty((C, B, F, 5), F32)
    t[..., :4] = boxes.transpose(1, 0, 2)[None]
    t[..., 4] = scores.transpose(2, 1, 0)
    return t, annot


def test_planted_objects():
    t, _ = planted()
    out = spec.seq_nms_classes(t, np.full(3, 40, np.int32), max_seqs=4096)
    assert out['exhausted'].all() and out['nseq'].tolist() == [247, 247, 247]          # pinned: what this rule gives on this input
    assert (out['seq_len'][:, :3] == 12).all() and (out['seq_len'][:, 3:] < 12).all()
    for c in (0, 1):
        for k in range(3):
            rows, frames = np.nonzero(out['seq'][c] == k)
            assert sorted(frames) == list(range(12)) and (rows < 18).all()             # the planted proposals
    for c in range(3):
        for k in range(int(out['nseq'][c])):
            m = out['seq'][c] == k
            old = t[c][m][:, 4].astype(np.float64)
            assert (out['score'][c][m] >= old.min()).all() and (out['score'][c][m] <= old.max()).all()


def test_cases_sit_on_their_seams():
    assert sc.lds_frames(64) == 1008 and sc.lds_frames(65) == 508 and sc.lds_frames(256) == 255
    for c in sc.cases():
        R, F = c['tracks'].shape[1:3]
        S = c['kw'].get('max_seqs', 32)
        if c['seam'] is None:
            assert F < sc.lds_frames(R), c['name']
        elif c['seam'][0] == 'lds':
            assert (1 if F <= sc.lds_frames(R) else 2) == c['seam'][1] and abs(F - sc.lds_frames(R) - 0.5) < 1, c['name']
        else:
            assert sc.launch_plan(F, S)[1] == c['seam'][1], c['name']
    # the rounds really go beyond the first launch where the case says so
    for name in ('launches_2_one_short', 'launches_3_exact'):
        c = sc.case(name)
        assert sc.expect(c)['nseq'][0] > sc.launch_plan(c['tracks'].shape[2], c['kw']['max_seqs'])[0]


# ---- the binding ---------------------------------------------------------------------------------------------------------
def test_prototypes_and_header():
    from vdetlib_amd import _lib
    one, batch = _lib.SYMBOLS['vdet_seq_nms'], _lib.SYMBOLS['vdet_seq_nms_batch']
    assert len(one[1]) == 22 and len(batch[1]) == 23
    assert batch[1][3:] == one[1][2:]                   # (ctx, off, V | ctx, F) and then the same tail
    hdr = open(os.path.join(ROOT, 'include', 'vdet_hip.h')).read()
    for word in ('vdet_seq_nms(', 'vdet_seq_nms_batch(', 'VDET_SEQNMS_LDS', 'what = 14', 'max_seqs <= 4096', 'R <= 256'):
        assert word in hdr, word


def test_ops_signatures():
    from vdetlib_amd import ops
    p = inspect.signature(ops.seq_nms).parameters
    assert list(p) == ['dets', 'ntracks', 'score', 'link_thres', 'nms_thres', 'rescore', 'max_seqs', 'min_score', 'sync', 'ctx']
    assert [p[k].default for k in list(p)[1:]] == [None, None, 0.5, 0.3, 'avg', 32, -np.inf, True, None]
    q = inspect.signature(ops.seq_nms_batch).parameters
    assert list(q) == ['batch_dets', 'score', 'link_thres', 'nms_thres', 'rescore', 'max_seqs', 'min_score', 'sync', 'ctx']
    assert [q[k].default for k in list(q)[1:]] == [None, 0.5, 0.3, 'avg', 32, -np.inf, True, None]
    assert 'untuned' in ops.seq_nms.__doc__


def test_value_errors_start_no_device_work():
    """host tensors throughout: whatever passes the shape checks ends at the device check, a ValueError as well"""
    import torch
    from vdetlib_amd import ops
    z = torch.zeros
    a = dict(dets=z(2, 3, 4, 5), ntracks=z(2, dtype=torch.int32), score=z(2, 3, 4, dtype=torch.float64))
    bad = [
        dict(dets=z(2, 3, 4, 4)), dict(dets=z(2, 3, 4, 5, dtype=torch.float64)), dict(dets=z(2, 3, 0, 5), score=None),
        dict(dets=z(0, 3, 4, 5), ntracks=z(0, dtype=torch.int32), score=None), dict(dets=z(2, 0, 4, 5), score=None),
        dict(dets=z(2, 257, 4, 5), score=None), dict(dets=None),
        dict(ntracks=z(2, dtype=torch.int64)), dict(ntracks=z(3, dtype=torch.int32)), dict(ntracks=None),
        dict(score=z(2, 3, 5)), dict(score=z(2, 3, 4, dtype=torch.float16)), dict(score=1), dict(score='score'),
        dict(link_thres=np.inf), dict(link_thres=np.nan), dict(nms_thres=-np.inf), dict(nms_thres=np.nan), dict(min_score=np.nan),
        dict(rescore='mean'), dict(rescore=0), dict(max_seqs=0), dict(max_seqs=4097),
        {}, dict(score=None),                           # every shape is right: host tensors
    ]
    for kw in bad:
        args = dict(a, **kw)
        with pytest.raises(ValueError) as e:
            ops.seq_nms(args.pop('dets'), args.pop('ntracks'), args.pop('score'), **args)
        assert ('same GPU' in str(e.value)) == (kw in ({}, dict(score=None))), (kw.keys(), str(e.value))
    # the dict form: ntracks must stay None; score a tensor, the name of a tensor field or the index of a series
    d = dict(tracks=a['dets'], ntracks=a['ntracks'], score=a['score'], series=(a['score'],))
    for kw in (dict(ntracks=a['ntracks']), dict(score=1), dict(score='pooled'), dict(score='series'), dict(score=2.5)):
        with pytest.raises(ValueError) as e:
            ops.seq_nms(d, **kw)
        assert 'same GPU' not in str(e.value)
    for kw in ({}, dict(score='score'), dict(score=0), dict(score=a['score'])):
        with pytest.raises(ValueError, match='same GPU'):
            ops.seq_nms(d, **kw)
    with pytest.raises(ValueError):
        ops.seq_nms(dict(tracks=a['dets']))
    # C*R*F, the link words and C*max_seqs below 2^31 - 16 (meta tensors: no memory behind them)
    m = lambda *s, **k: torch.empty(*s, device='meta', **k)
    for C, R, F, S in ((3000, 256, 3000, 32), (40000, 256, 30, 32), (600000, 1, 1, 4096)):
        with pytest.raises(ValueError, match="2\\^31"):
            ops.seq_nms(m(C, R, F, 5), m(C, dtype=torch.int32), max_seqs=S)


def test_batch_value_errors_start_no_device_work():
    import torch
    from vdetlib_amd import ops
    C, R = 2, 3
    off = np.array([0, 2, 5], np.int64)

    def views(per, dtype, R=R):
        flat = torch.zeros(C * R * 5 * per, dtype=dtype)
        return [flat[C * R * per * int(off[v]): C * R * per * int(off[v + 1])].view(*((C, R, int(off[v + 1] - off[v])) + ((per,) if per > 1 else ())))
                for v in range(2)]
    bo = dict(tracks=views(5, torch.float32), score=views(1, torch.float64), det=views(1, torch.float32), half=views(1, torch.float16),
              ntracks=torch.zeros(2, C, dtype=torch.int32), frame_off=off)
    bad = [
        (dict(bo, tracks=None), {}), (dict(bo, ntracks=torch.zeros(2, C, dtype=torch.int64)), {}), (dict(bo, frame_off=[0, 2, 4]), {}),
        (dict(bo, tracks=bo['tracks'][::-1]), {}), ('nothing', {}),
        (dict(bo, tracks=views(5, torch.float32, 257)), {}),
        (bo, dict(score='pooled')), (bo, dict(score='half')), (bo, dict(score=0)), (bo, dict(score=bo['score'])), (bo, dict(score='ntracks')),
        (bo, dict(link_thres=np.inf)), (bo, dict(nms_thres=np.nan)), (bo, dict(min_score=np.nan)), (bo, dict(rescore='both')),
        (bo, dict(max_seqs=0)), (bo, dict(max_seqs=4097)),
    ]
    for b, kw in bad:
        with pytest.raises(ValueError) as e:
            ops.seq_nms_batch(b, **kw)
        assert 'same GPU' not in str(e.value), (kw, str(e.value))
    for kw in ({}, dict(score='score'), dict(score='det')):
        with pytest.raises(ValueError, match='same GPU'):
            ops.seq_nms_batch(bo, **kw)
