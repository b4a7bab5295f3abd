"""Device against spec, BIT-EQUAL, no tolerance: ops.seq_nms / ops.seq_nms_batch (csrc/seqnms_kernels.hpp) against
tests/seqnms_spec.py on the cases of tests/seqnms_cases.py -- tracks and score by NaN-aware equality of the values and their
signs, every integer output exactly.
  a. every case; the cases on a seam took the path they name (vdet_query 14, the launches of the timing buckets)
  b. the knife-edge pairs of tests/golden/knife_pairs.npz as link decisions and as suppression decisions
  c. batches: identical boxes on both sides of every video border, V = 1, sync=False
  d. robustness: outputs pre-filled with garbage through the C entry point, misaligned views
  e. every VDET_EINVAL of the limits row, with no launch
  f. end to end: nms_volume -> nms_tracks -> seq_nms -> DetEvaluator against eval.evaluate on the spec's result
  g. a third of a., and b., with VDET_SEQNMS_LDS=0 (the predecessor table in global scratch) in a fresh child process: the
     switch is read at vdet_create"""
import os
import subprocess
import sys

import numpy as np
import pytest

import knife_spec as K
import seqnms_cases as sc
import seqnms_spec as spec
import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = os.path.join(ROOT, 'tests', 'golden', 'knife_pairs.npz')
F32 = np.float32
INT_KEYS = ('seq', 'ntracks', 'nseq', 'seq_len', 'seq_end', 'exhausted')
DTYPES = dict(tracks=np.float32, score=np.float64, seq=np.int32, ntracks=np.int32, nseq=np.int32, seq_sum=np.float64,
              seq_len=np.int32, seq_end=np.int32, exhausted=np.uint8)


def g(x):
    import torch
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def same_floats(a, b):
    """NaN where NaN, else the same value with the same sign."""
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a[~na], b[~nb]) and \
        np.array_equal(np.signbit(a[~na]), np.signbit(b[~nb]))


def assert_same(got, want, who=""):
    for k in spec.KEYS:
        x = got[k].cpu().numpy() if hasattr(got[k], 'cpu') else got[k]
        assert x.dtype == DTYPES[k] and x.shape == np.shape(want[k]), (who, k, x.dtype, x.shape)
        if k in INT_KEYS:
            assert np.array_equal(x, want[k]), (who, k)
        else:
            assert same_floats(x, np.asarray(want[k])), (who, k)


def run_case(c, ctx=None):
    from vdetlib_amd import ops
    got = ops.seq_nms(g(c['tracks']), g(c['ntracks']), g(c['score']), ctx=ctx, **c['kw'])
    assert_same(got, sc.expect(c), c['name'])
    return got


# a. -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sc.cases(), ids=lambda c: c["name"])
def test_case(case):
    import torch
    from vdetlib_amd import _lib
    ctx = _lib.get_context(torch.cuda.current_device())
    if case['seam'] is None:
        run_case(case)
        assert ctx.query(14) == 1
        return
    ctx.set_timing(1)
    try:
        run_case(case)
        launches = ctx.last_timing()
    finally:
        ctx.set_timing(0)
    kind, n = case['seam']
    if kind == 'lds':
        assert ctx.query(14) == n
    else:
        assert launches['track_link'][1] == 1 and launches['track_loop'][1] == 1      # one timed span each ...
        F, S = case['tracks'].shape[2], case['kw']['max_seqs']
        assert sc.launch_plan(F, S)[1] == n                                             # ... and the plan the host restates


def test_dict_forms_and_consumers():
    """a tubelet dict goes in as it is; a score by name, by series index, as a tensor; the result feeds nms_tracks unchanged"""
    from vdetlib_amd import ops
    c = sc.case('score_f64')
    t, nt, s = g(c['tracks']), g(c['ntracks']), g(c['score'])
    want = sc.expect(c)
    for d, score in ((dict(tracks=t, ntracks=nt, score=s), 'score'), (dict(tracks=t, ntracks=nt, series=(s,)), 0),
                     (dict(tracks=t, ntracks=nt), s)):
        assert_same(ops.seq_nms(d, score=score, **c['kw']), want)
    col4 = sc.expect(dict(c, score=None))
    got = ops.seq_nms(dict(tracks=t, ntracks=nt, score=s), **c['kw'])                 # the default is column 4, dict or not
    assert_same(got, col4)
    again = ops.nms_tracks(got['tracks'], got['ntracks'], got['score'], thresh=0.3)
    kept = int((got['seq'] >= spec.LEFTOVER).sum())
    assert 0 < int(again['cnt'].sum()) <= kept


# b. -------------------------------------------------------------------------------------------------------------------
def knife_decisions():
    """{key: (a, b, t, decision)}: the quotient rule on every pair of the fixture, false where the union is zero."""
    out = {}
    for key, (a, b) in K.load_pairs(PAIRS).items():
        t = 1.0 if key[0] == 'unit' else key[1]
        inter, uni, q = K.quotient(a, b)
        out[key] = (a, b, t, (uni > 0) & (q >= K.thresh_to_f32(t)))
    return out


def run_knife():
    import torch
    from vdetlib_amd import ops
    total = 0
    for key, (a, b, t, want) in knife_decisions().items():
        n = len(a)
        total += n
        assert np.array_equal(want, np.array([spec.hit_matrix(a[i:i + 1], b[i:i + 1], t)[0, 0] for i in range(n)])), key
        # two-frame videos, one pair per class: a in frame 0, b in frame 1; linked <=> the first sequence has two members
        tr = np.zeros((n, 1, 2, 5), F32)
        tr[:, 0, 0, :4], tr[:, 0, 1, :4], tr[..., 4] = a, b, 1.0
        nt = torch.ones(n, dtype=torch.int32, device='cuda')
        out = ops.seq_nms(g(tr), nt, link_thres=t, nms_thres=2.0, max_seqs=2)
        assert np.array_equal(out['seq_len'][:, 0].cpu().numpy() == 2, want), (key, 'link')
        assert_same(out, spec.seq_nms_classes(tr, np.ones(n, np.int32), link_thres=t, nms_thres=2.0, max_seqs=2), key)
        # one-frame videos holding both: a scores higher, is taken first, and suppresses b or does not
        tr = np.zeros((n, 2, 1, 5), F32)
        tr[:, 0, 0, :4], tr[:, 1, 0, :4], tr[:, 0, 0, 4], tr[:, 1, 0, 4] = a, b, 2.0, 1.0
        nt = torch.full((n,), 2, dtype=torch.int32, device='cuda')
        out = ops.seq_nms(g(tr), nt, link_thres=2.0, nms_thres=t, max_seqs=1)
        assert np.array_equal(out['seq'][:, 1, 0].cpu().numpy() == spec.SUPPRESSED, want), (key, 'suppress')
        assert (out['seq'][:, 0, 0] == 0).all()
        assert_same(out, spec.seq_nms_classes(tr, np.full(n, 2, np.int32), link_thres=2.0, nms_thres=t, max_seqs=1), key)
    return total


def test_knife_edge_pairs():
    d = knife_decisions()
    assert any(w.any() for _, _, _, w in d.values()) and any((~w).any() for _, _, _, w in d.values())
    assert run_knife() > 100


# c. -------------------------------------------------------------------------------------------------------------------
def pack(vids, nt, off, with_score=False):
    """video_batch's layout: per-video views of one flat allocation"""
    import torch
    from vdetlib_amd import ops
    C, R = vids[0].shape[:2]
    flat = torch.cat([g(v).reshape(-1) for v in vids])
    bo = dict(tracks=ops._batch_views(flat, off, C, R, 5), ntracks=g(nt), frame_off=off)
    if with_score:
        sflat = torch.cat([g(v[..., 4].astype(np.float64) * 0.5 - 0.1).reshape(-1) for v in vids])
        bo['pooled'] = ops._batch_views(sflat, off, C, R, 1)
    return bo


def assert_batch(out, vids, nt, off, kw, score=None):
    for k in ('ntracks', 'nseq', 'exhausted', 'seq_sum', 'seq_len', 'seq_end'):
        assert out[k].shape[0] == len(vids)
    assert np.array_equal(out['frame_off'], off)
    for v, t in enumerate(vids):
        s = None if score is None else t[..., 4].astype(np.float64) * 0.5 - 0.1
        want = spec.seq_nms_classes(t, nt[v], s, **kw)
        got = {k: (out[k][v] if isinstance(out[k], list) else out[k][v]) for k in spec.KEYS}
        assert_same(got, want, 'video %d' % v)


def test_batch_borders_hold_identical_boxes():
    import torch
    from vdetlib_amd import _lib, ops
    vids, nt, off = sc.border_batch()
    for a, b in zip(vids, vids[1:]):
        assert np.array_equal(a[:, :, -1], b[:, :, 0])                # a link across the border would be taken
    kw = dict(link_thres=0.5, nms_thres=0.3, max_seqs=16)
    bo = pack(vids, nt, off, with_score=True)
    cx = _lib.Context()
    try:
        assert cx.query(11) == 0 and cx.query(14) == -1
        ops.seq_nms_batch(bo, ctx=cx, **kw)
        out = ops.seq_nms_batch(bo, ctx=cx, **kw)
        assert cx.query(11) == 1 and cx.query(14) == 1              # the staged per-video table, staged once
    finally:
        cx.close()
    assert_batch(out, vids, nt, off, kw)
    for v, t in enumerate(vids):                                      # ... and per video the single call's bits
        one = ops.seq_nms(g(t), g(nt[v]), **kw)
        assert_same({k: out[k][v] for k in spec.KEYS}, {k: one[k].cpu().numpy() for k in spec.KEYS}, 'single %d' % v)
    assert_batch(ops.seq_nms_batch(bo, score='pooled', rescore='max', **kw), vids, nt, off, dict(kw, rescore='max'), score='pooled')
    assert out['seq_len'].max() <= max(t.shape[2] for t in vids)
    for k in ('tracks', 'score', 'seq'):                              # views of ONE allocation per field, video after video
        ops._batch_flat(out[k])


def test_batch_of_one_and_async():
    import torch
    from vdetlib_amd import _lib, ops
    vids, nt, off = sc.border_batch()
    kw = dict(max_seqs=16)
    one = pack(vids[4:5], nt[4:5], np.array([0, 12], np.int64))
    assert_batch(ops.seq_nms_batch(one, **kw), vids[4:5], nt[4:5], np.array([0, 12], np.int64), kw)
    cx = _lib.Context()
    try:
        side = torch.cuda.Stream()
        bo = pack(vids, nt, off)
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            out = ops.seq_nms_batch(bo, sync=False, ctx=cx, **kw)
            single = ops.seq_nms(g(vids[2]), g(nt[2]), sync=False, ctx=cx, **kw)
            cx.sync()
        assert_batch(out, vids, nt, off, kw)
        assert_same(single, spec.seq_nms_classes(vids[2], nt[2], **kw))
    finally:
        cx.close()


# d. -------------------------------------------------------------------------------------------------------------------
def c_call(ctx, t, nt, s, F, C, R, S, outs, link=0.5, nms=0.3, rescore=0, floor=-np.inf, score_f64=1):
    ptr = lambda x: None if x is None else (x if isinstance(x, int) else x.data_ptr())
    return ctx.lib.vdet_seq_nms(ctx.h, F, C, R, ptr(t), ptr(nt), ptr(s), score_f64, link, nms, rescore, S, floor, *[ptr(o) for o in outs])


def out_buffers(C, R, F, S, fill, guard=0):
    import torch
    shapes = ((C * R * F * 5, torch.float32), (C * R * F, torch.float64), (C * R * F, torch.int32), (C, torch.int32), (C, torch.int32),
              (C * S, torch.float64), (C * S, torch.int32), (C * S * 2, torch.int32), (C, torch.uint8))
    return [torch.full((n + guard,), fill, dtype=d).cuda() for n, d in shapes]


def test_outputs_are_fully_overwritten_and_nothing_beyond():
    import torch
    from vdetlib_amd import _lib
    c = sc.case('no_nodes_f64')
    C, R, F = c['tracks'].shape[:3]
    S, G = 64, 9
    ctx = _lib.get_context(torch.cuda.current_device())
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    want = sc.expect(c)
    for fill in (77, 0):
        outs = out_buffers(C, R, F, S, fill, G)
        ctx.check(c_call(ctx, g(c['tracks']), g(c['ntracks']), g(c['score']), F, C, R, S, outs))
        ctx.sync()
        for o, k in zip(outs, spec.KEYS):
            x = o.cpu().numpy()
            assert (x[-G:] == fill).all(), k                          # the guard behind every output
            got = x[:-G].reshape(np.shape(want[k]))
            assert np.array_equal(got, want[k]) if k in INT_KEYS else same_floats(got, np.asarray(want[k])), (k, fill)


def test_misaligned_views():
    """every input sliced off by one element of a larger buffer: 4-byte aligned rows, 8-byte aligned f64 scores, no more"""
    import torch
    from vdetlib_amd import ops
    for name in ('score_f64', 'score_f32', 'R65_all'):
        c = sc.case(name)

        def off_by_one(x):
            if x is None:
                return None
            buf = torch.zeros(x.size + 5, dtype=g(x).dtype, device='cuda')
            v = buf[1:1 + x.size].view(x.shape)
            v.copy_(g(x))
            assert v.data_ptr() % 16 != 0 and v.is_contiguous()
            return v
        got = ops.seq_nms(off_by_one(c['tracks']), off_by_one(c['ntracks']), off_by_one(c['score']), **c['kw'])
        assert_same(got, sc.expect(c), name)


# e. -------------------------------------------------------------------------------------------------------------------
def test_c_level_limits_launch_nothing():
    import torch
    from vdetlib_amd import _lib
    c = sc.case('tie_free')
    C, R, F = c['tracks'].shape[:3]
    S = 8
    t, nt = g(c['tracks']), g(c['ntracks'])
    ctx = _lib.get_context(torch.cuda.current_device())
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    ctx.set_timing(2)
    try:
        ctx.last_timing()
        outs = out_buffers(C, R, F, S, 55)
        E = _lib.VDET_EINVAL
        call = lambda **kw: c_call(ctx, kw.pop('t', t), kw.pop('nt', nt), None, kw.pop('F', F), kw.pop('C', C), kw.pop('R', R),
                                   kw.pop('S', S), kw.pop('outs', outs), **kw)
        for kw in (dict(R=0), dict(R=257), dict(S=0), dict(S=4097), dict(F=0), dict(C=0), dict(F=-1),
                   dict(C=1 << 22, R=256, F=2),                       # C*R*F = 2^31
                   dict(C=1 << 20, R=256, F=2),                       # the link words: C*R*F*8 = 2^32
                   dict(C=1 << 20, R=1, F=1, S=4096),                 # C*max_seqs = 2^32
                   dict(link=np.inf), dict(link=np.nan), dict(nms=-np.inf), dict(nms=np.nan), dict(floor=np.nan),
                   dict(rescore=2), dict(rescore=-1), dict(t=None), dict(nt=None)) + \
                tuple(dict(outs=outs[:i] + [None] + outs[i + 1:]) for i in range(len(outs))):
            assert call(**kw) == E, kw
        off = np.array([0, 2, 2], np.int64)
        tail = (C, R, t.data_ptr(), nt.data_ptr(), None, 0, 0.5, 0.3, 0, S, -np.inf) + tuple(o.data_ptr() for o in outs)
        assert ctx.lib.vdet_seq_nms_batch(ctx.h, off.ctypes.data, 2, *tail) == E
        assert ctx.lib.vdet_seq_nms_batch(ctx.h, None, 2, *tail) == E
        big = np.arange(65537, dtype=np.int64)
        assert ctx.lib.vdet_seq_nms_batch(ctx.h, big.ctypes.data, 65536, *tail) == E
        assert ctx.lib.vdet_seq_nms(None, F, *tail) == E                # no context
        assert sum(n for _, n in ctx.last_timing().values()) == 0, "a refused call launched something"
        ctx.sync()
        assert all((o == 55).all() for o in outs), "a refused call wrote something"
        # the context still works
        ctx.check(c_call(ctx, t, nt, None, F, C, R, S, outs))
        ctx.sync()
        assert np.array_equal(outs[4].cpu().numpy(), sc.expect(c, max_seqs=S)['nseq'])
    finally:
        ctx.set_timing(0)


# f. -------------------------------------------------------------------------------------------------------------------
def test_end_to_end_with_the_evaluator(capsys):
    import torch
    from test_eval_gpu import _check
    from vdetlib_amd import ops
    from vdetlib_amd import eval as veval
    boxes, scores, annot = synth.vid_with_objects(7, 12, 40, 3)
    tb, ts = g(boxes), g(scores)
    idx, cnt = ops.nms_volume(tb, ts, 0.3)
    F, B, C = scores.shape
    empty = torch.zeros((C, 0, F, 5), dtype=torch.float32, device='cuda')
    dets = ops.nms_tracks(empty, torch.zeros(C, dtype=torch.int32, device='cuda'), torch.zeros((C, 0, F), dtype=torch.float64, device='cuda'),
                          still=(tb, ts, idx, cnt), thresh=0.3, cap=64)
    out = ops.seq_nms(dets, score='score', max_seqs=32)
    want = spec.seq_nms_classes(dets['tracks'].cpu().numpy(), dets['ntracks'].cpu().numpy(), dets['score'].cpu().numpy(), max_seqs=32)
    assert_same(out, want)
    assert (out['nseq'] > 0).all()
    gt = veval.gt_table_from_annots([annot])
    ev0 = ops.DetEvaluator(gt)
    ev0.add_detections(annot['video'], dets)
    before = ev0.compute()[1]
    ev = ops.DetEvaluator(gt)
    assert ev.add_detections(annot['video'], out) > 0
    # device == host on the spec's detections: APs and mAP within the evaluator's stated 1e-12, identical tp sequences
    aps, after = _check(ev, veval.detections_from_tracks(annot['video'], want['tracks'], want['ntracks'], want['score']), [annot], 'voc')
    with capsys.disabled():
        print("\nseq_nms end to end: mAP %.6f before, %.6f after" % (before, after))
    assert after > 0


# g. -------------------------------------------------------------------------------------------------------------------
CHILD = """
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import seqnms_cases as sc
import test_seqnms_gpu as t
import torch
from vdetlib_amd import _lib
cx = _lib.get_context(torch.cuda.current_device())        # (the context ops uses)
assert cx.query(14) == -1
third = sc.cases()[::3]
for case in third:
    t.run_case(case)
    assert cx.query(14) == 2, case["name"]
n = t.run_knife()
assert cx.query(14) == 2
print("predecessor table in global scratch: %%d cases and %%d knife-edge pairs ok" %% (len(third), n))
"""


def test_a_third_of_the_cases_with_the_table_in_global_scratch():
    env = dict(os.environ, VDET_SEQNMS_LDS="0")
    r = subprocess.run([sys.executable, "-c", CHILD % (ROOT, os.path.join(ROOT, "tests"))], env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "knife-edge pairs ok" in r.stdout
