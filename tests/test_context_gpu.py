"""Device against spec, BIT-EQUAL, no tolerance: ops.context_classes / ops.suppress_context (csrc/context_kernels.hpp) against
tests/context_spec.py on the cases of tests/context_cases.py -- thresh by its bits, n, hits, high, and every output element by
its uint32 view.
  a. every case: the record path where the records fit, the natural fallback where they do not
  b. every case again with VDET_CTX_RECORDS=0 (the full-read passes forced), in a fresh child process: the switch is read at
     vdet_create
  c. a scores view that starts one float off a 16-byte boundary; batches against the single-video call on each slice
  d. suppress_context: out of place, in place, misaligned against each other, NaN payloads, -inf, penalties 0.4 / 0.0 / 1e30
  e. asynchronous use on a side context
  f. end to end: context_classes -> suppress_context -> nms_volume(score_thresh) -> DetEvaluator on a small synthetic video"""
import os
import subprocess
import sys

import numpy as np
import pytest

import context_cases as cc
import context_spec as spec

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def g(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def u32(x):
    return np.ascontiguousarray(x, dtype=F32).view(np.uint32)


def assert_classes(got, want, who=""):
    gt, gn, gh, gg = (x.cpu().numpy() for x in got)
    wt, wn, wh, wg = want
    assert gt.dtype == F32 and gn.dtype == np.int64 and gh.dtype == np.int32 and gg.dtype == bool, who
    assert gt.shape == np.shape(wt) and gh.shape == wh.shape and gg.shape == wg.shape, who
    assert np.array_equal(u32(gt), u32(wt)), (who, gt, wt)
    assert np.array_equal(gn, wn), (who, gn, wn)
    assert np.array_equal(gh, wh), who
    assert np.array_equal(gg, wg), who


def run_case(case, ctx=None, offset=0):
    """Both calls of one case against the spec; offset: the scores live `offset` floats into a 16-byte aligned buffer."""
    import torch
    from vdetlib_amd import ops
    s, kw = case["scores"], case["kw"]
    want = spec.context_classes(s, **kw)
    if offset:
        buf = torch.zeros(s.size + 8, dtype=torch.float32, device='cuda')
        assert buf.data_ptr() % 16 == 0
        ts = buf[offset:offset + s.size].view(s.shape)
        ts.copy_(g(s))
        assert ts.data_ptr() % 16 == 4 * offset and ts.is_contiguous()
    else:
        ts = g(s)
    got = ops.context_classes(ts, ctx=ctx, **kw)
    assert_classes(got, want, case["name"])
    fo = kw.get("frame_off")
    for penalty in (0.4, 1e30):
        out = ops.suppress_context(ts, got[3], penalty=penalty, frame_off=fo, ctx=ctx)
        assert np.array_equal(u32(out.cpu().numpy()), u32(spec.suppress_context(s, want[3], penalty, fo))), (case["name"], penalty)
    assert np.array_equal(u32(ts.cpu().numpy()), u32(s))         # the input is left alone


# a. -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cc.cases(), ids=lambda c: c["name"])
def test_case(case):
    run_case(case)


def test_natural_fallback_is_taken_where_the_cases_say():
    """The cases named *_beyond_records hold more keys at or above the chosen bin than their video has record slots (the formula
    restated in context_cases.record_cap), so they reach the full-read passes without the switch; the others named here fit."""
    for name in ("all_equal_beyond_records", "tied_top_beyond_records"):
        s = cc.case(name)["scores"]
        t = cc.case(name)["expect"]["thresh"]
        assert int((s >= t).sum()) > cc.record_cap(s.size)
    s = cc.case("all_equal_small")["scores"]
    assert s.size <= cc.record_cap(s.size)
    # ... and the device took the paths named (vdet_query 13: full reads of the volume the last call needed)
    from vdetlib_amd import _lib, ops
    cx = _lib.Context()
    try:
        assert cx.query(13) == -1
        for name, reads in (("all_equal_beyond_records", 4), ("tied_top_beyond_records", 4), ("late_records_uniform", 3),
                            ("dense_records", 2),
                            ("all_equal_small", 2), ("shape_4x129x200_ratio", 2), ("seam_video_border", 2), ("all_nan", 0)):
            c = cc.case(name)
            ops.context_classes(g(c["scores"]), ctx=cx, **c["kw"])
            assert cx.query(13) == reads, name
    finally:
        cx.close()


# b. -------------------------------------------------------------------------------------------------------------------
CHILD = """
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import context_cases as cc
import test_context_gpu as t
import torch
from vdetlib_amd import _lib
cx = _lib.get_context(torch.cuda.current_device())        # (the context ops uses)
for case in cc.cases():
    t.run_case(case)
    nonempty = bool((t.spec.context_classes(case["scores"], **case["kw"])[1] > 0).any())
    assert cx.query(13) == (4 if nonempty else 0), case["name"]        # four full reads wherever there is a candidate
    t.run_case(case, offset=3)
print("forced full-read path: %%d cases ok" %% len(cc.cases()))
"""


def test_every_case_with_the_records_switched_off():
    env = dict(os.environ, VDET_CTX_RECORDS="0")
    r = subprocess.run([sys.executable, "-c", CHILD % (ROOT, os.path.join(ROOT, "tests"))], env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0 and "cases ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


# c. -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("shape_4x129x200_ratio", "shape_2x65x201_top", "shape_3x7x3_top", "seam_last_first",
                                  "seam_video_border", "tied_top_beyond_records", "late_records_uniform", "dense_records",
                                  "batch_v3_high_sets_differ"))
@pytest.mark.parametrize("offset", (1, 2, 3))
def test_scores_off_a_16_byte_boundary(name, offset):
    run_case(cc.case(name), offset=offset)


@pytest.mark.parametrize("name", ("batch_v3_high_sets_differ", "batch_v3_top", "video_all_nan", "seam_video_border"))
def test_batch_equals_video_by_video(name):
    from vdetlib_amd import ops
    case = cc.case(name)
    s, kw = case["scores"], dict(case["kw"])
    off = kw.pop("frame_off")
    ts = g(s)
    bt, bn, bh, bg = (x.cpu().numpy() for x in ops.context_classes(ts, frame_off=off, **kw))
    assert bt.shape == (len(off) - 1,) and bh.shape == (len(off) - 1, s.shape[2])
    out = ops.suppress_context(ts, g(bg), frame_off=off).cpu().numpy()
    for v, (a, b) in enumerate(zip(off[:-1], off[1:])):
        one = ops.context_classes(ts[a:b], **kw)
        assert_classes(one, (bt[v], bn[v], bh[v], bg[v]), "%s video %d" % (name, v))
        assert np.array_equal(u32(ops.suppress_context(ts[a:b], one[3]).cpu().numpy()), u32(out[a:b]))


# d. -------------------------------------------------------------------------------------------------------------------
def special_volume():
    s = cc._rand(77, (4, 129, 200), nan_frac=0.0)
    r = np.random.RandomState(78)
    v = s.view(np.uint32).reshape(-1)
    pos = r.choice(v.size, 600, replace=False)
    v[pos[:200]] = 0x7FC00000 | r.randint(1, 1 << 22, 200).astype(np.uint32)         # quiet NaN with payloads
    v[pos[200:300]] = 0xFFC00000 | r.randint(1, 1 << 22, 100).astype(np.uint32)       # ... negative ones
    v[pos[300:400]] = 0x7F800001 + r.randint(0, 1 << 20, 100).astype(np.uint32)       # signalling patterns
    s.reshape(-1)[pos[400:500]] = -np.inf
    s.reshape(-1)[pos[500:]] = np.inf
    return s


@pytest.mark.parametrize("penalty", (0.4, 0.0, 1e30))
def test_suppress_out_of_place_in_place_and_specials(penalty):
    import torch
    from vdetlib_amd import ops
    s = special_volume()
    high = np.zeros(200, bool)
    high[[0, 3, 77, 199]] = True
    want = spec.suppress_context(s, high, penalty)
    nan = np.isnan(s)
    assert np.array_equal(u32(want)[nan], u32(s)[nan]) and np.all(want[s == -np.inf] == -np.inf)
    assert np.array_equal(u32(want)[:, :, high], u32(s)[:, :, high])
    ts, th = g(s), g(high)
    out = ops.suppress_context(ts, th, penalty=penalty)
    assert out.data_ptr() != ts.data_ptr() and np.array_equal(u32(out.cpu().numpy()), u32(want))
    assert np.array_equal(u32(ts.cpu().numpy()), u32(s))
    given = torch.empty_like(ts)
    assert ops.suppress_context(ts, th, penalty=penalty, out=given) is given
    assert np.array_equal(u32(given.cpu().numpy()), u32(want))
    # out and scores on different 16-byte phases: the element-wise form
    buf = torch.zeros(s.size + 8, dtype=torch.float32, device='cuda')
    shifted = buf[1:1 + s.size].view(s.shape)
    ops.suppress_context(ts, th, penalty=penalty, out=shifted)
    assert np.array_equal(u32(shifted.cpu().numpy()), u32(want)) and float(buf[0]) == 0.0 and not buf[1 + s.size:].any()
    # in place
    same = ops.suppress_context(ts, th, penalty=penalty, out=ts)
    assert same is ts and np.array_equal(u32(ts.cpu().numpy()), u32(want))
    # in place on a view off the boundary; the floats around it stay
    buf.zero_()
    view = buf[3:3 + s.size].view(s.shape)
    view.copy_(g(s))
    ops.suppress_context(view, th, penalty=penalty, out=view)
    assert np.array_equal(u32(view.cpu().numpy()), u32(want)) and not buf[:3].any() and not buf[3 + s.size:].any()


def test_suppress_overlapping_out_is_refused():
    import torch
    from vdetlib_amd import ops
    buf = torch.zeros(2 * 3 * 4 + 4, dtype=torch.float32, device='cuda')
    s, o = buf[:24].view(2, 3, 4), buf[4:28].view(2, 3, 4)
    with pytest.raises(ValueError, match="overlap"):
        ops.suppress_context(s, torch.zeros(4, dtype=torch.bool, device='cuda'), out=o)


def test_many_classes_beyond_the_lds_tables():
    """C above the classes a workgroup keeps in LDS (4096): the global form of the hit counts and of the high flags, both paths"""
    s = cc._rand(79, (1, 9, 5000))
    s[0, :, 4500] = 9.0
    s[0, 4, 17] = 9.0
    case = dict(name="C5000", scores=s, kw=dict(top=10))
    run_case(case)
    cx = cc.records_off_context()
    try:
        run_case(case, ctx=cx)
        assert cx.query(13) == 4
    finally:
        cx.close()


# e. -------------------------------------------------------------------------------------------------------------------
def test_asynchronous_use_on_a_side_context():
    import torch
    from vdetlib_amd import _lib, ops
    case = cc.case("batch_v3_high_sets_differ")
    s, kw = case["scores"], case["kw"]
    want = spec.context_classes(s, **kw)
    ts = g(s)
    cx = _lib.Context(torch.cuda.current_device())
    try:
        cx.sync()
        before = cx.query(8)
        got = ops.context_classes(ts, sync=False, ctx=cx, **kw)
        out = ops.suppress_context(ts, got[3], frame_off=kw["frame_off"], sync=False, ctx=cx)
        one = ops.context_classes(ts[1:6], ratio=kw["ratio"], sync=False, ctx=cx)
        assert cx.query(8) == before            # no host wait between the entries and the returns
        cx.sync()
        assert_classes(got, want)
        assert np.array_equal(u32(out.cpu().numpy()), u32(spec.suppress_context(s, want[3], 0.4, kw["frame_off"])))
        assert_classes(one, spec.context_classes(s[1:6], ratio=kw["ratio"]))
    finally:
        cx.close()


# f. -------------------------------------------------------------------------------------------------------------------
def test_end_to_end_on_a_small_synthetic_video(oracle):
    """context_classes -> suppress_context -> nms_volume(score_thresh) -> DetEvaluator: at a threshold that kept them before, the
    keep lists of a suppressed class are empty and a high class's lists are unchanged; the lists equal oracle.nms_volume on the
    spec's output, and the evaluator has nothing left to score for the suppressed classes."""
    import synth
    from vdetlib_amd import ops
    F, B, C, TH, NMS = 6, 40, 5, 0.6, 0.3
    boxes, scores = synth.video(4242, F, B, C)              # scores in (0, 1), tie-free per (frame, class)
    scores[:, ::3, 1] += F32(1.0)                           # the video's objects: classes 1 and 3
    scores[:, 1::5, 3] += F32(1.0)
    scores[:, 0, 0] = F32(0.995)                            # box 0 leads column 0 on every frame: the ground truth below
    tb, ts = g(boxes), g(scores)
    t, n, hits, high = ops.context_classes(ts, ratio=0.02)
    want = spec.context_classes(scores, ratio=0.02)
    assert_classes((t, n, hits, high), want)
    assert want[3].tolist() == [False, True, False, True, False]
    sup = ops.suppress_context(ts, high, penalty=0.4)
    want_sup = spec.suppress_context(scores, want[3], 0.4)
    assert np.array_equal(u32(sup.cpu().numpy()), u32(want_sup))
    idx0, cnt0 = (x.cpu().numpy() for x in ops.nms_volume(tb, ts, NMS, score_thresh=TH))
    idx1, cnt1 = ops.nms_volume(tb, sup, NMS, score_thresh=TH)
    widx, wcnt = oracle.nms_volume(boxes, want_sup, NMS, score_thresh=TH)
    assert np.array_equal(idx1.cpu().numpy(), widx) and np.array_equal(cnt1.cpu().numpy(), wcnt)
    for c in range(C):
        if want[3][c]:
            assert np.array_equal(wcnt[:, c], cnt0[:, c]) and np.array_equal(widx[:, c], idx0[:, c])
        else:
            assert cnt0[:, c].min() > 0 and not wcnt[:, c].any()
    # the evaluator: one ground-truth box per frame for a suppressed class (box 0, class column 0) and a high one (column 1)
    fr = np.arange(1, F + 1, dtype=np.int64)
    table = {'videos': ['v'], 'video': np.zeros(2 * F, np.int32), 'frame': np.concatenate([fr, fr]),
             'class_index': np.concatenate([np.full(F, 1), np.full(F, 2)]).astype(np.int64),
             'bbox': np.concatenate([boxes[:, 0], boxes[:, 0]]).astype(np.float64)}
    plain, supp = ops.DetEvaluator(table), ops.DetEvaluator(table)
    n_plain = plain.add_keep_lists('v', tb, ts, g(idx0), g(cnt0))
    n_supp = supp.add_keep_lists('v', tb, sup, idx1, cnt1)
    assert 0 < n_supp < n_plain
    ap_plain, ap_supp = plain.compute()[0], supp.compute()[0]
    assert ap_plain[1] > 0.0 and ap_supp[1] == 0.0 and ap_supp[2] == ap_plain[2]
