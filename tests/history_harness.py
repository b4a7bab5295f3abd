"""What test_call_history_cpu.py and test_call_history_gpu.py share: a registry of STAGES whose results must not depend on what
the context ran before.  No GPU and no product code at import; torch is imported where a function needs the device.

A ``Call`` is (stage name, numpy inputs, keyword arguments).  A stage knows how to run a call of its kind on a context
(``run``), what the call must return (``want``: the numpy rule its own GPU test file already compares against, imported from
there and never restated) and how that file compares (``same``).  ``probe()`` is the call whose result the tests pin;
``wears()`` names sequences of calls -- of this stage or of another one that shares its state -- which leave the context's
scratch and resident tables in the state that is most likely to leak into the probe: every link and live bit set, a table
of the same byte length built from other offsets, a wider stride, an emptied histogram.  All inputs are valid.

The offset pair: A = (0, 4, 6) and B = (0, 2, 6) (A8 / B8 for the 8-frame stages): two videos either way, the same key
length, the same total, so that a stale per-video table stays inside every buffer and only moves the border.

``fresh(ctx_env)`` makes a new context, optionally under an environment switch that is read at creation."""
import collections
import contextlib
import functools
import os

import numpy as np

F32, F64 = np.float32, np.float64
OFF_A, OFF_B = (0, 4, 6), (0, 2, 6)
OFF_A8, OFF_B8 = (0, 5, 8), (0, 3, 8)

Call = collections.namedtuple('Call', 'stage inputs kw')


def fresh(ctx_env=None, device=-1):
    """A new context on the current device, created with the variables of ``ctx_env`` set (and restored afterwards): the
    switches are read at vdet_create.  The caller closes it."""
    from vdetlib_amd import _lib
    env = dict(ctx_env or {})
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return _lib.Context(device)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


@contextlib.contextmanager
def context(ctx_env=None, cache=False, asynchronous=False):
    cx = fresh(ctx_env)
    try:
        cx.set_cache(cache)
        if asynchronous:
            cx.set_async(True)
        yield cx
    finally:
        cx.close()


def g(x):
    import torch
    return None if x is None else torch.from_numpy(np.array(x)).cuda()            # (a copy: cached cases are read-only)


def host(out):
    """a stage's outputs -> numpy (per-video lists stay lists); what a stage holds for the device's sake ('_held') is dropped"""
    def one(x):
        if isinstance(x, (list, tuple)):
            return [one(y) for y in x]
        return x.cpu().numpy() if hasattr(x, 'cpu') else np.asarray(x)
    return {k: one(v) for k, v in out.items() if k != '_held'}


def same_array(a, b):
    """shape, dtype and bits, a NaN equal to any NaN; lists element by element"""
    if isinstance(a, list) or isinstance(b, list):
        return isinstance(a, list) and isinstance(b, list) and len(a) == len(b) and all(same_array(x, y) for x, y in zip(a, b))
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != 'f':
        return bool(np.array_equal(a, b))
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and a[~na].tobytes() == b[~nb].tobytes())


def bitwise(a, b):
    """two device results of ONE call: every byte, NaN payloads included"""
    def eq(x, y):
        if isinstance(x, list):
            return len(x) == len(y) and all(eq(p, q) for p, q in zip(x, y))
        x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
        return x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes()
    return sorted(a) == sorted(b) and all(eq(a[k], b[k]) for k in a)


def passes(check, *args):
    """an asserting comparator of a test file as a predicate"""
    try:
        check(*args)
    except AssertionError:
        return False
    return True


class _Host(object):
    """numpy behind the two methods the comparators of the GPU files call on a tensor"""

    def __init__(self, x):
        self.x = x

    def cpu(self):
        return self

    def numpy(self):
        return self.x


def views(flat, off, C, T, per):
    from vdetlib_amd import ops
    return ops._batch_views(flat, np.asarray(off, np.int64), C, T, per)


def flat_of(arrays, dtype):
    import torch
    return torch.from_numpy(np.concatenate([np.ascontiguousarray(a, dtype).ravel() for a in arrays])).cuda()


class Stage(object):
    """One entry of the registry.  ``keys``: the compared outputs; ``envs``: the environments a context of this stage's tests
    is created under; ``path(ctx)``: None, or a check that the call took the path its environment names; ``tab``: the
    frame offsets a call stages in the context's per-video table (None: it stages nothing)."""
    name, keys, envs, device_rule = None, (), (None,), False

    def probe(self):
        raise NotImplementedError

    def wears(self):
        return []

    def run(self, ctx, call, sync=True):
        raise NotImplementedError

    def want(self, call):
        raise NotImplementedError

    def same(self, got, want):
        return all(same_array(got[k], want[k]) for k in self.keys)

    def check_path(self, ctx, env):
        pass

    def tab(self, call):
        return None


STAGES = collections.OrderedDict()


def register(stage):
    assert stage.name not in STAGES
    STAGES[stage.name] = stage
    return stage


def run_call(ctx, call, sync=True):
    return STAGES[call.stage].run(ctx, call, sync)


@functools.lru_cache(maxsize=None)
def _want(name, which):
    st = STAGES[name]
    call = st.probe() if which == 'probe' else dict(st.wears())[which][-1]
    return STAGES[call.stage].want(call)


def want_probe(name):
    """the rule's result of a stage's probe, computed once and shared; never modified"""
    return _want(name, 'probe')


def want_wear(name, wear):
    """the rule's result of the LAST call of a wear"""
    return _want(name, wear)


def pairs(device_rules=True):
    return [(n, w) for n, st in STAGES.items() if device_rules or not st.device_rule for w, _ in st.wears()]


def tab_of(call):
    return STAGES[call.stage].tab(call)


# ---- top_anchors ---------------------------------------------------------------------------------------------------------------------
class TopAnchors(Stage):
    """topa_hist + topa_hist_clean, anchor_tab (staged directly, V = 1 included when offsets are given)"""
    name, keys = 'top_anchors', ('frames', 'boxes', 'scores', 'index')

    @staticmethod
    @functools.lru_cache(maxsize=None)
    def volume(seed, F, B, C):
        import test_top_anchors_gpu as TA
        return TA.make(seed, F, B, C)

    def call(self, seed, F, B, C, top, **kw):
        boxes, scores = self.volume(seed, F, B, C)
        return Call(self.name, dict(boxes=boxes, scores=scores), dict(kw, top_num=top))

    def probe(self):
        return self.call(9801, 7, 40, 3, 5)         # 280 rows: two 256-row segments

    def wears(self):
        wide = self.call(9802, 7, 40, 70, 5, frame_off=(0, 2, 5, 7))       # two class tiles, V*C = 210 histograms
        return [('batch_v3_c70', [wide]),
                ('thresh_above_all', [self.call(9801, 7, 40, 3, 5, score_thresh=1e9)]),
                ('frame_mode', [self.call(9801, 7, 40, 3, 3, mode='frame')]),
                ('top_beyond_candidates', [self.call(9801, 7, 40, 3, 300)]),
                ('regrow', [self.call(9803, 2, 5, 1, 2), self.call(9804, 7, 40, 130, 4, mode='frame')])]

    def run(self, ctx, call, sync=True):
        from vdetlib_amd import ops
        tb, ts = g(call.inputs['boxes']), g(call.inputs['scores'])
        out = ops.top_anchors(tb, ts, sync=sync, ctx=ctx, **call.kw)
        return dict(zip(self.keys, out), _held=(tb, ts))

    def want(self, call):
        import test_top_anchors_gpu as TA
        kw = dict(call.kw)
        boxes, scores, top, thr = call.inputs['boxes'], call.inputs['scores'], kw['top_num'], kw.get('score_thresh')
        if kw.get('mode') == 'frame':
            w = TA.want_frame(boxes, scores, top, thr)
        elif kw.get('frame_off') is not None:
            off = kw['frame_off']
            per = [TA.want_video(boxes[a:b], scores[a:b], top, thr) for a, b in zip(off[:-1], off[1:])]
            w = tuple(np.stack([p[k] for p in per]) for k in range(4))
        else:
            w = TA.want_video(boxes, scores, top, thr)
        return dict(frames=w[0], boxes=w[1], scores=w[2], index=w[3])

    def same(self, got, want):
        import test_top_anchors_gpu as TA
        return passes(TA.check, [_Host(got[k]) for k in self.keys], (want['frames'], want['boxes'], want['scores'], want['index']),
                      self.name)

    def tab(self, call):
        return call.kw.get('frame_off')


register(TopAnchors())


# ---- Seq-NMS -------------------------------------------------------------------------------------------------------------------------
SQ_KW = dict(link_thres=0.5, nms_thres=0.3, max_seqs=256)          # more rounds than a probe has nodes: it runs to exhaustion
SQ_WEAR_KW = dict(nms_thres=2.0, max_seqs=1)


def sq_identical(C, R, F, seed=0):
    """every box the same, every score finite: every link bit and every live bit is set; with max_seqs = 1 and no suppression
    (SQ_WEAR_KW) the rounds end with done = 1 and R - 1 live nodes left over on every frame"""
    t = np.empty((C, R, F, 5), F32)
    t[..., :4] = (10, 10, 50, 50)
    t[..., 4] = 0.25 + np.random.RandomState(9900 + seed).rand(C, R, F).astype(F32)
    return t


class SeqNms(Stage):
    """sq_link / sq_live / sq_done / sq_ptr.  The probes leave ntracks below R in one class: rows the link kernel never writes."""
    keys = ('tracks', 'score', 'seq', 'ntracks', 'nseq', 'seq_sum', 'seq_len', 'seq_end', 'exhausted')
    envs = (None, {'VDET_SEQNMS_LDS': '0'})

    def __init__(self, name, R, nt):
        self.name, self.R, self.nt = name, R, nt

    def single(self, tracks, ntracks, **kw):
        return Call(self.name, dict(tracks=tracks, ntracks=np.asarray(ntracks, np.int32)), dict(SQ_KW, **kw))

    def probe(self):
        import seqnms_cases as sc
        return self.single(sc.video(9910 + self.R, 2, self.R, 6), self.nt)

    def wears(self):
        import seqnms_cases as sc
        R = self.R
        long = sc.case('F%d_global_first' % (sc.lds_frames(64) + 1))
        return [('identical_r64', [self.single(sq_identical(2, 64, 8), (64, 64), **SQ_WEAR_KW)]),
                ('identical_same_shape', [self.single(sq_identical(2, R, 6, 1), (R, R), **SQ_WEAR_KW)]),
                ('batch_other_offsets', [SEQ_BATCH.batch(OFF_B, 9930, max_seqs=2)]),
                ('global_path_first', [Call(self.name, dict(tracks=long['tracks'], ntracks=long['ntracks']), dict(long['kw']))])]

    def run(self, ctx, call, sync=True):
        from vdetlib_amd import ops
        t, nt = g(call.inputs['tracks']), g(call.inputs['ntracks'])
        out = ops.seq_nms(t, nt, sync=sync, ctx=ctx, **call.kw)
        return dict(out, _held=(t, nt))

    def want(self, call):
        import seqnms_spec as spec
        return spec.seq_nms_classes(call.inputs['tracks'], call.inputs['ntracks'], None, **call.kw)

    def same(self, got, want):
        import test_seqnms_gpu as SQ
        return passes(SQ.assert_same, got, want, self.name)

    def check_path(self, ctx, env):
        assert ctx.query(14) == (2 if env else 1)


class SeqNmsBatch(Stage):
    """... and anchor_tab through video_table"""
    name, keys, envs = 'seq_nms_batch', SeqNms.keys, SeqNms.envs
    C, R = 2, 33

    @staticmethod
    @functools.lru_cache(maxsize=None)
    def videos(off, seed):
        import seqnms_cases as sc
        vids = tuple(sc.video(seed + v, SeqNmsBatch.C, SeqNmsBatch.R, b - a) for v, (a, b) in enumerate(zip(off[:-1], off[1:])))
        nt = np.full((len(vids), SeqNmsBatch.C), SeqNmsBatch.R, np.int32)
        nt[0, 1] = 20 + (seed % 7)                     # rows behind a count, and counts that differ between the pair
        return vids, nt

    def batch(self, off, seed, **kw):
        vids, nt = self.videos(tuple(off), seed)
        return Call(self.name, dict(vids=vids, ntracks=nt, off=np.asarray(off, np.int64)), dict(SQ_KW, **kw))

    def probe(self):
        return self.batch(OFF_A, 9920)

    def wears(self):
        other = self.batch(OFF_B, 9930, max_seqs=2)
        one = STAGES['seq_nms_w2'].probe()
        return [('other_offsets', [other]),
                ('single_between', [other, one, other]),
                ('identical_r64', [STAGES['seq_nms_w2'].wears()[0][1][0], other])]

    def run(self, ctx, call, sync=True):
        import test_seqnms_gpu as SQ
        from vdetlib_amd import ops
        bo = SQ.pack(list(call.inputs['vids']), call.inputs['ntracks'], call.inputs['off'])
        out = ops.seq_nms_batch(bo, sync=sync, ctx=ctx, **call.kw)
        return dict({k: out[k] for k in self.keys}, _held=bo)

    def want(self, call):
        import seqnms_spec as spec
        per = [spec.seq_nms_classes(t, call.inputs['ntracks'][v], None, **call.kw) for v, t in enumerate(call.inputs['vids'])]
        return {k: [np.asarray(p[k]) for p in per] for k in self.keys}

    def same(self, got, want):
        import test_seqnms_gpu as SQ
        V = len(want['seq'])
        return all(len(got[k]) == V for k in self.keys) and \
            all(passes(SQ.assert_same, {k: got[k][v] for k in self.keys}, {k: want[k][v] for k in self.keys}, v) for v in range(V))

    def check_path(self, ctx, env):
        assert ctx.query(14) == (2 if env else 1)

    def tab(self, call):
        return tuple(int(x) for x in call.inputs['off'])


register(SeqNms('seq_nms_w2', 33, (33, 20)))
register(SeqNms('seq_nms_w1', 20, (7, 20)))
SEQ_BATCH = register(SeqNmsBatch())


# ---- tubelet NMS ---------------------------------------------------------------------------------------------------------------------
TUBE_KW = dict(thresh=0.4, norm='union', reduce='mean', min_shared=1)


def tube_distinct(C, T, F, seed):
    """no two tubelets of a class overlap: any stale pair bit suppresses one of them"""
    t = np.empty((C, T, F, 5), F32)
    for s in range(T):
        for f in range(F):
            t[:, s, f, :4] = (200 * s + f, 10 + f, 200 * s + 80 + f, 90 + f)
    rng = np.random.RandomState(seed)
    t[..., 4] = rng.rand(C, T, F).astype(F32)
    return t, np.full(C, T, np.int32), rng.permutation(C * T).reshape(C, T).astype(F64)


def tube_identical(C, T, F):
    """every tubelet the same boxes on every frame: every pair's overlap is 1, every bit of every tile is set"""
    t = np.empty((C, T, F, 5), F32)
    t[..., :4] = (10, 10, 50, 50)
    t[..., 4] = 0.5
    return t, np.full(C, T, np.int32), np.tile(np.arange(T, dtype=F64), (C, 1))


class TubeNms(Stage):
    """tube_scratch: tiles past ntracks are not computed, the sub-arrays move with T and C"""

    def __init__(self, name, full, overlaps):
        self.name, self.full, self.overlaps = name, full, overlaps
        self.keys = ('tracks', 'ntracks', 'src', 'tscore', 'by') + (('overlaps',) if overlaps else ())

    def single(self, tracks, ntracks, score, **kw):
        return Call(self.name, dict(tracks=tracks, ntracks=ntracks, score=score), dict(TUBE_KW, return_overlaps=self.overlaps, **kw))

    def probe(self):
        import tubenms_cases as cases
        if self.full:
            return self.single(*tube_distinct(2, 33, 8, 9940))
        s = cases.random_set(9941, 2, 33, 8)
        return self.single(s['tracks'], np.array([20, 20], np.int32), s['score2'])       # the second 32-slot tile is skipped

    def wears(self):
        return [('identical_t33', [self.single(*tube_identical(2, 33, 8))]),
                ('batch_t64_c1', [TUBE_BATCH.batch(OFF_B8, 1, 64, 9950)]),
                ('batch_other_offsets', [TUBE_BATCH.batch(OFF_B8, 2, 33, 9951)])]

    def run(self, ctx, call, sync=True):
        from vdetlib_amd import ops
        t, nt, s = g(call.inputs['tracks']), g(call.inputs['ntracks']), g(call.inputs['score'])
        out = ops.nms_tubelets(t, nt, s, sync=sync, ctx=ctx, **call.kw)
        return dict({k: out[k] for k in self.keys}, _held=(t, nt, s))

    def want(self, call):
        import tubenms_spec as spec
        kw = call.kw
        w = spec.expected(call.inputs['tracks'], call.inputs['ntracks'], call.inputs['score'], None, None, (), kw['thresh'], kw['norm'],
                          kw['reduce'], kw['min_shared'])
        return {k: w[k] for k in self.keys}

    def same(self, got, want):
        from test_tubenms_cpu import same
        return all(same(got[k], want[k]) for k in self.keys)


class TubeNmsBatch(Stage):
    name, keys = 'nms_tubelets_batch', ('tracks', 'ntracks', 'src', 'tscore', 'by', 'overlaps')

    @staticmethod
    @functools.lru_cache(maxsize=None)
    def videos(off, C, T, seed):
        import tubenms_cases as cases
        sets = [cases.random_set(seed + v, C, T, b - a, tboxes=False) for v, (a, b) in enumerate(zip(off[:-1], off[1:]))]
        nt = np.stack([s['ntracks'] for s in sets]).astype(np.int32)
        nt[-1, 0] = 20 + seed % 5
        return tuple(s['tracks'] for s in sets), nt, np.stack([s['score2'] for s in sets])

    def batch(self, off, C, T, seed):
        tr, nt, score = self.videos(tuple(off), C, T, seed)
        return Call(self.name, dict(vids=tr, ntracks=nt, score=score, off=np.asarray(off, np.int64)), dict(TUBE_KW, return_overlaps=True))

    def probe(self):
        return self.batch(OFF_A8, 2, 33, 9960)

    def wears(self):
        other = self.batch(OFF_B8, 2, 33, 9951)
        return [('other_offsets', [other]),
                ('identical_t33', [STAGES['nms_tubelets_full'].wears()[0][1][0], other]),
                ('batch_t64_c1', [self.batch(OFF_B8, 1, 64, 9950)])]

    def run(self, ctx, call, sync=True):
        from vdetlib_amd import ops
        vids, off = call.inputs['vids'], call.inputs['off']
        C, T = vids[0].shape[:2]
        bo = dict(tracks=views(flat_of(vids, F32), off, C, T, 5), ntracks=g(call.inputs['ntracks']), frame_off=off)
        score = g(call.inputs['score'])
        out = ops.nms_tubelets_batch(bo, score=score, sync=sync, ctx=ctx, **call.kw)
        return dict({k: out[k] for k in self.keys}, _held=(bo, score))

    def want(self, call):
        import tubenms_spec as spec
        kw = call.kw
        per = [spec.expected(t, call.inputs['ntracks'][v], call.inputs['score'][v], None, None, (), kw['thresh'], kw['norm'],
                             kw['reduce'], kw['min_shared']) for v, t in enumerate(call.inputs['vids'])]
        return {k: [p[k] for p in per] for k in self.keys}

    def same(self, got, want):
        from test_tubenms_cpu import same
        V = len(want['tracks'])
        return all(len(got[k]) == V and all(same(got[k][v], want[k][v]) for v in range(V)) for k in self.keys)

    def tab(self, call):
        return tuple(int(x) for x in call.inputs['off'])


TUBE_BATCH = TubeNmsBatch()
register(TubeNms('nms_tubelets_nt20', False, False))
register(TubeNms('nms_tubelets_nt20_overlaps', False, True))
register(TubeNms('nms_tubelets_full', True, False))
register(TubeNms('nms_tubelets_full_overlaps', True, True))
register(TUBE_BATCH)


# ---- the per-frame list NMS family -------------------------------------------------------------------------------------------------
LIST_RULES = ('nms_tracks', 'soft_nms_tracks', 'vote_nms_tracks')


def list_rule(op):
    """(the ListNms of the rule's GPU file, the keyword arguments of the rule's generated cases)"""
    if op == 'nms_tracks':
        import test_nms_tracks_gpu as m
    elif op == 'soft_nms_tracks':
        import test_softnms_gpu as m
    else:
        import test_votenms_gpu as m
    return m.H, dict(thresh=m.H.case_thresh)


class ListNmsStage(Stage):
    """the list kernels' shared scratch: a wider list, the other members of the family just before"""

    def __init__(self, op):
        self.op = self.name = op

    @property
    def keys(self):
        return list_rule(self.op)[0].row_keys + ('cnt', 'ntracks')

    def of_case(self, case):
        from test_nms_tracks_cpu import still_of
        return Call(self.name, dict(tracks=case['tracks'], ntracks=case['ntracks'], score=case['score'], tboxes=case['tboxes'],
                                    still=still_of(case)), list_rule(self.op)[1])

    def probe(self):
        from test_nms_tracks_cpu import CASES, make_case
        return self.of_case(make_case(*CASES[0]))

    def wears(self):
        from listnms_harness import wide_lists
        from test_nms_tracks_cpu import CASES, make_case
        tracks, ntracks, score, still = wide_lists(300)
        others = [STAGES[o].of_case(make_case(*CASES[1])) for o in LIST_RULES if o != self.op]
        return [('wide_lists', [Call(self.name, dict(tracks=tracks, ntracks=ntracks, score=score, tboxes=None, still=still),
                                     list_rule(self.op)[1])]),
                ('batch_other_offsets', [STAGES[self.op + '_batch'].batch(OFF_B)]),
                ('same_shape_other_video', [self.of_case(make_case(*((CASES[0][0] + 100,) + CASES[0][1:])))]),
                ('family_before', others)]

    def run(self, ctx, call, sync=True):
        from vdetlib_amd import ops
        H = list_rule(self.op)[0]
        i = call.inputs
        d = [g(i[k]) for k in ('tracks', 'ntracks', 'score', 'tboxes')] + [g(x) for x in i['still']]
        out = getattr(ops, self.op)(d[0], d[1], d[2], tboxes=d[3], still=tuple(d[4:]), sync=sync, ctx=ctx, **dict(H.op_kw, **call.kw))
        return dict({k: out[k] for k in self.keys}, _held=d)

    def want(self, call):
        i = call.inputs
        return list_rule(self.op)[0].want_of(i['tracks'], i['ntracks'], i['score'], i['tboxes'], i['still'], **call.kw)

    def same(self, got, want):
        return bool(list_rule(self.op)[0].outputs_equal(got, want))


class ListNmsBatch(Stage):
    def __init__(self, op):
        self.op, self.name = op, op + '_batch'

    @property
    def keys(self):
        return list_rule(self.op)[0].row_keys + ('cnt', 'ntracks')

    def batch(self, off):
        from test_nms_tracks_cpu import make_case
        from test_nms_tracks_gpu import BB, BC, BT
        cases = tuple(make_case(41 + v + 10 * off[1], b - a, BB, BC, BT) for v, (a, b) in enumerate(zip(off[:-1], off[1:])))
        return Call(self.name, dict(cases=cases, off=np.asarray(off, np.int64)), list_rule(self.op)[1])

    def probe(self):
        return self.batch(OFF_A)

    def wears(self):
        others = [STAGES[o + '_batch'].batch(OFF_B) for o in LIST_RULES if o != self.op]
        return [('other_offsets', [self.batch(OFF_B)]),
                ('single_between', [self.batch(OFF_B), STAGES[self.op].probe(), self.batch(OFF_B)]),
                ('family_before', others)]

    def run(self, ctx, call, sync=True):
        from test_nms_tracks_gpu import pack_batch
        from vdetlib_amd import ops
        H = list_rule(self.op)[0]
        bo, still = pack_batch(list(call.inputs['cases']))
        out = getattr(ops, self.name)(bo, 'pooled', still=still, sync=sync, ctx=ctx, **dict(H.op_kw, **call.kw))
        off = [int(x) for x in call.inputs['off']]
        cnt = [out['cnt'][:, a:b] for a, b in zip(off[:-1], off[1:])]          # per video, like every other output
        return dict({k: out[k] for k in self.keys}, cnt=cnt, _held=(bo, still))

    def want(self, call):
        from test_nms_tracks_cpu import still_of
        H = list_rule(self.op)[0]
        per = [H.want_of(c['tracks'], c['ntracks'], c['score'], c['tboxes'], still_of(c), **call.kw) for c in call.inputs['cases']]
        return {k: [p[k] for p in per] for k in self.keys}

    def same(self, got, want):
        H = list_rule(self.op)[0]
        V = len(want['cnt'])
        return all(len(got[k]) == V for k in self.keys) and \
            all(H.outputs_equal({k: got[k][v] for k in self.keys}, {k: want[k][v] for k in self.keys}) for v in range(V))

    def tab(self, call):
        return tuple(int(x) for x in call.inputs['off'])


for _op in LIST_RULES:
    register(ListNmsStage(_op))
for _op in LIST_RULES:
    register(ListNmsBatch(_op))


# ---- re-scoring and merging of tubelet sets (batch forms) -------------------------------------------------------------------------
class RescoreBatch(Stage):
    name, keys = 'rescore_tubelets_batch', ('det', 'pooled', 'tboxes', 'src')

    @staticmethod
    @functools.lru_cache(maxsize=None)
    def case(off, seed):
        import rescore_spec as R
        return R.batch_case(seed, off, 5)[:4]

    def batch(self, off, seed):
        boxes, scores, tracks, ntracks = self.case(tuple(off), seed)
        return Call(self.name, dict(boxes=boxes, scores=scores, vids=tuple(tracks), ntracks=ntracks, off=tuple(off)), {})

    def probe(self):
        return self.batch(OFF_A, 9100)

    def wears(self):
        other = self.batch(OFF_B, 9140)
        one = self.batch((0, 6), 9150)
        return [('a_b_a', [self.probe(), other]),
                ('single_between', [other, one, other]),
                ('same_offsets_other_videos', [self.batch(OFF_A, 9160)]),
                ('merge_other_offsets', [MERGE_BATCH.batch(OFF_B, 5)])]

    def run(self, ctx, call, sync=True):
        from test_rescore_tubelets_gpu import batch_dict
        from vdetlib_amd import ops
        i = call.inputs
        bo, tb, ts = batch_dict(list(i['vids']), i['ntracks'], list(i['off'])), g(i['boxes']), g(i['scores'])
        out = ops.rescore_tubelets_batch(bo, tb, ts, sync=sync, ctx=ctx, **call.kw)
        return dict({k: out[k] for k in self.keys}, _held=(bo, tb, ts))

    def want(self, call):
        import rescore_spec as R
        i = call.inputs
        w, eindex = R.spec_batch(list(i['vids']), i['ntracks'], i['boxes'], i['scores'], i['off'], **call.kw)
        assert not eindex
        return dict(zip(self.keys, w))

    def same(self, got, want):
        from test_rescore_tubelets_gpu import same
        return all(len(got[k]) == len(want[k]) and all(same(x, y) for x, y in zip(got[k], want[k])) for k in self.keys)

    def tab(self, call):
        off = tuple(int(x) for x in call.inputs['off'])
        return off if len(off) > 2 else None


class MergeBatch(Stage):
    name, keys = 'merge_tracks_batch', ('tracks', 'ntracks', 'anchors', 'tboxes', 'det', 'pooled')

    @staticmethod
    @functools.lru_cache(maxsize=None)
    def pairs(off, seed):
        import test_merge_tracks_gpu as MG
        out = []
        for v, (a, b) in enumerate(zip(off[:-1], off[1:])):
            sa, sb = MG.pair(b - a, 2, True, False, False, seed=seed + v)
            sa = MG.copy_set(sa)
            sa['ntracks'][0] = 3 - seed % 3             # (pair's counts are constants: the halves of the offset pair differ in theirs)
            out.append((sa, sb))
        return tuple(out)

    def batch(self, off, seed):
        return Call(self.name, dict(pairs=self.pairs(tuple(off), seed), off=tuple(off)), dict(scheme='combine'))

    def probe(self):
        return self.batch(OFF_A, 1)

    def wears(self):
        other = self.batch(OFF_B, 5)
        return [('a_b_a', [self.probe(), other]),
                ('single_between', [other, self.batch((0, 6), 9), other]),
                ('rescore_other_offsets', [RESCORE_BATCH.batch(OFF_B, 9140)])]

    def run(self, ctx, call, sync=True):
        import test_merge_tracks_gpu as MG
        from vdetlib_amd import ops
        off = np.asarray(call.inputs['off'], np.int64)
        ba, bb = MG._pack([p[0] for p in call.inputs['pairs']], off, MG.TA), MG._pack([p[1] for p in call.inputs['pairs']], off, MG.TB)
        out = ops.merge_tracks_batch(ba, bb, call.kw['scheme'], sync=sync, ctx=ctx)
        return dict({k: out[k] for k in self.keys}, _held=(ba, bb))

    def want(self, call):
        from test_merge_tracks_cpu import mirror
        per = [mirror(a, b, call.kw['scheme'])[0] for a, b in call.inputs['pairs']]
        w = {k: [p[k] for p in per] for k in ('tracks', 'ntracks', 'anchors', 'tboxes')}
        w['det'], w['pooled'] = [p['series'][0] for p in per], [p['series'][1] for p in per]
        return w

    def same(self, got, want):
        from test_merge_tracks_cpu import sets_equal
        as_set = lambda d, v: dict(tracks=d['tracks'][v], ntracks=d['ntracks'][v], anchors=d['anchors'][v], tboxes=d['tboxes'][v],
                                   series=(d['det'][v], d['pooled'][v]))
        V = len(want['tracks'])
        return len(got['tracks']) == V and all(sets_equal(as_set(got, v), as_set(want, v)) for v in range(V))

    def tab(self, call):
        off = tuple(int(x) for x in call.inputs['off'])
        return off if len(off) > 2 else None


RESCORE_BATCH, MERGE_BATCH = RescoreBatch(), MergeBatch()
register(RESCORE_BATCH)
register(MERGE_BATCH)


# ---- multi-context suppression ---------------------------------------------------------------------------------------------------
class Context(Stage):
    """ctxs_tab (keyed by offsets and shape), ctxs_hist, ctxs_state, ctxs_rec: both calls of the stage, one after the other"""
    name, keys = 'context', ('thresh', 'n', 'hits', 'high', 'out')
    envs = (None, {'VDET_CTX_RECORDS': '0'})

    def of_case(self, name, **over):
        import context_cases as cc
        c = cc.case(name)
        return Call(self.name, dict(scores=c['scores']), dict(c['kw'], **over))

    def probe(self):
        return self.of_case('batch_v3_top')

    def wears(self):
        return [('other_offsets_same_shape', [self.of_case('batch_v3_top', frame_off=[0, 3, 5, 8], top=7)]),
                ('high_sets_differ', [self.of_case('batch_v3_high_sets_differ')]),
                ('more_classes', [self.of_case('shape_2x65x201_ratio')]),
                ('all_equal_beyond_records', [self.of_case('all_equal_beyond_records')]),
                ('video_all_nan', [self.of_case('video_all_nan')])]

    def run(self, ctx, call, sync=True):
        from vdetlib_amd import ops
        ts = g(call.inputs['scores'])
        got = ops.context_classes(ts, sync=sync, ctx=ctx, **call.kw)
        out = ops.suppress_context(ts, got[3], penalty=0.4, frame_off=call.kw.get('frame_off'), sync=sync, ctx=ctx)
        return dict(zip(self.keys, tuple(got) + (out,)), _held=ts)

    def check_path(self, ctx, env):
        if env:
            assert ctx.query(13) == 4              # records off: the four full reads on a video with candidates

    def want(self, call):
        import context_spec as spec
        w = spec.context_classes(call.inputs['scores'], **call.kw)
        out = spec.suppress_context(call.inputs['scores'], w[3], 0.4, call.kw.get('frame_off'))
        return dict(zip(self.keys, tuple(np.asarray(x) for x in w) + (out,)))

    def same(self, got, want):
        from test_context_gpu import assert_classes, u32
        return passes(assert_classes, [_Host(got[k]) for k in self.keys[:4]], [want[k] for k in self.keys[:4]]) and \
            bool(np.array_equal(u32(got['out']), u32(want['out'])))


register(Context())


# ---- the tubelet TCN -------------------------------------------------------------------------------------------------------------
class Tcn(Stage):
    """tcn_params / tcn_foff / tcn_ovtab / tcn_segs: tables keyed by their bytes.  The rule of tests/test_tcn_gpu.py is the
    per-tubelet path, which runs its layers on the device (on the process-wide context, never on the one under test), and the
    tubelets come from the device tracker: ``device_rule`` -- test_call_history_cpu.py checks the nets, the GPU file that the
    wears' answers differ from the probe's."""
    name, keys, device_rule = 'tcn_tracks', ('conv',), True
    envs = (None, {'VDET_TCN_GLOBAL': '1'})
    NETS = {'probe': ((8, 8), 5, 3), 'twin': ((8, 8), 5, 33), 'wide_first': ((192, 24), 5, 6)}       # hidden widths, K, seed

    @staticmethod
    @functools.lru_cache(maxsize=None)
    def net(key):
        import test_tcn_gpu as TG
        from vdetlib_amd.vdet.tcn import TCNNet
        hidden, k, seed = Tcn.NETS[key]
        return TCNNet.random([(n, 1) for n in TG.BASE], hidden=hidden, kernel=k, seed=seed)

    @staticmethod
    @functools.lru_cache(maxsize=None)
    def tubelets(seed, nf):
        """the tubelets of test_tcn_gpu.py's video fixture (or of a longer video), as numpy; made on a context of their own"""
        import test_tcn_gpu as TG
        from vdetlib_amd import ops
        boxes, scores, _ = TG.make_video(seed, nf=nf, objects=[(c, a, min(b, nf)) for c, a, b in TG.OBJECTS] if nf != TG.F else TG.OBJECTS)
        with context() as cx:
            tb, ts = g(boxes), g(scores)
            _, _, tr, an, nt = ops.nms_track_volume(tb, ts, nms_thres=0.3, thres=0.5, max_tracks=TG.T, link_thres=0.4, ctx=cx)
            det = ops.rescore_tracks(tr, nt, tb, ts, overlap_thres=0.5, window=3, ctx=cx)[0]
            return {k: v.cpu().numpy() for k, v in dict(tr=tr, an=an, nt=nt, det=det).items()}

    def call(self, net, seed=7, nf=24):
        return Call(self.name, dict(video=(seed, nf)), dict(net=net))

    def probe(self):
        return self.call('probe')

    def wears(self):
        return [('twin_net', [self.call('twin')]),
                ('alternating', [self.call('probe'), self.call('twin'), self.call('probe'), self.call('twin')]),
                ('wide_first_layer', [self.call('wide_first')]),
                ('larger_series', [self.call('twin', seed=8, nf=40)])]

    def run(self, ctx, call, sync=True):
        from vdetlib_amd import ops
        v = {k: g(x) for k, x in self.tubelets(*call.inputs['video']).items()}
        out = ops.tcn_tracks(self.net(call.kw['net']), v['tr'], v['nt'], v['an'], v['det'], sync=sync, ctx=ctx)
        return dict(conv=out, _held=v)

    def want(self, call):
        import test_tcn_gpu as TG
        v = {k: g(x) for k, x in self.tubelets(*call.inputs['video']).items()}
        return dict(conv=TG.per_tubelet_reference(v, self.net(call.kw['net']))[0])

    def same(self, got, want):
        import test_tcn_gpu as TG
        return bool(got['conv'].dtype == np.float32 and TG.same_bits(got['conv'], want['conv']))

    def uploads(self, call):
        """the key of the parameter table a call brings"""
        return call.kw['net']


register(Tcn())


# ---- the SVM head ----------------------------------------------------------------------------------------------------------------
class SvmHead(Stage):
    """svm_wt, the W^T copy of the call: two models of one shape in turn, a larger K and M before the probe's"""
    name, keys = 'svm_head', ('score', 'arg_flat', 'det', 'arg', 'tboxes')        # (nbad is compared too: 0 in every valid call)
    N, G, SHAPE = 20, 3, (3, 2, 5)

    @staticmethod
    @functools.lru_cache(maxsize=None)
    def data(seed, mseed, K, M):
        import test_svm_head_gpu as SV
        rng = np.random.RandomState(seed)
        feat = rng.randn(SvmHead.N * SvmHead.G, K).astype(F32)
        cols = ((np.arange(SvmHead.SHAPE[0]) * 3 + 2) % M).astype(np.int32)
        return dict(feat=feat, model=SV.model_of(mseed, K, M, 'f64'), cols=cols, slot=SV.slots_of(seed + 2, SvmHead.N, SvmHead.SHAPE),
                    sboxes=rng.uniform(1, 300, (SvmHead.N, SvmHead.G, 4)))

    def call(self, seed, mseed, K, M):
        return Call(self.name, self.data(seed, mseed, K, M), dict(group=self.G, shape=self.SHAPE))

    def probe(self):
        return self.call(9970, 9971, 65, 7)

    def wears(self):
        twin = self.call(9970, 9981, 65, 7)
        return [('twin_model', [twin]), ('alternating', [self.probe(), twin, self.probe(), twin]),
                ('larger_k_m', [self.call(9972, 9973, 257, 11)])]

    def run(self, ctx, call, sync=True):
        import test_svm_head_gpu as SV
        from vdetlib_amd import ops
        i = call.inputs
        d = dict(feat=g(i['feat']), model=SV.dev_model(i['model']), slot=g(i['slot']), cols=g(i['cols']), sboxes=g(i['sboxes']))
        out = ops.svm_head(d['feat'], d['model'], slot=d['slot'], cols=d['cols'], sboxes=d['sboxes'], sync=sync, ctx=ctx, **call.kw)
        return dict({k: out[k] for k in self.keys + ('nbad',)}, _held=d)

    def want(self, call):
        import svm_spec as ss
        import test_svm_head_gpu as SV
        i = call.inputs
        w = ss.head(i['feat'], i['model']['W'], i['model']['B'], SV.scale_of(i['model'], np.float64), np.float64, slot=i['slot'],
                    cols=i['cols'], sboxes=i['sboxes'], **call.kw)
        assert not w['bad']
        return dict({k: np.asarray(w[k]) for k in self.keys}, nbad=np.array([w['nbad']], np.int32))

    def same(self, got, want):
        import test_svm_head_gpu as SV
        return all(passes(SV.same, _Host(got[k]), want[k], k) for k in self.keys) and same_array(got['nbad'], want['nbad'])


register(SvmHead())


# ---- the anchor route over batches -----------------------------------------------------------------------------------------------
class AnchorRoute(Stage):
    """track_from_anchors_batch + anchor_propagate_tracks_batch: anchor_tab through video_table.  The rule of
    tests/test_anchor_batch_gpu.py is the pair of single-video calls on every video's slice (``per_video``), which runs on the
    device (on the process-wide context): ``device_rule``.  The anchors are top_anchors' numpy rule, per video."""
    name, keys, device_rule = 'anchor_route_batch', ('tracks', 'anchors', 'ntracks', 'det', 'best'), True
    differ_keys = ('tracks', 'anchors', 'det')
    B, C, T = 12, 2, 3

    @staticmethod
    @functools.lru_cache(maxsize=None)
    def case(off, seed):
        import test_anchor_batch_gpu as AB
        import test_top_anchors_gpu as TA
        boxes, scores = AB.coherent_video(seed, off[-1], AnchorRoute.B, AnchorRoute.C)
        per = [TA.want_video(boxes[a:b], scores[a:b], AnchorRoute.T) for a, b in zip(off[:-1], off[1:])]
        fr, ab, sc = (np.stack([p[k] for p in per]) for k in range(3))
        return dict(boxes=boxes, scores=scores, fr=fr, ab=ab, sc=sc, off=off)

    def batch(self, off, seed):
        return Call(self.name, self.case(tuple(off), seed), {})

    def probe(self):
        return self.batch(OFF_A, 9990)

    def wears(self):
        other = self.batch(OFF_B, 9991)
        return [('a_b_a', [self.probe(), other]),
                ('single_between', [other, self.batch((0, 6), 9992), other]),
                ('seq_nms_other_offsets', [SEQ_BATCH.batch(OFF_B, 9930, max_seqs=2)])]

    def device(self, call):
        i = call.inputs
        return g(i['boxes']), g(i['scores']), g(i['fr']), g(i['ab']), g(i['sc'])

    def run(self, ctx, call, sync=True):
        from vdetlib_amd import ops
        tb, ts, fr, ab, sc = d = self.device(call)
        out = ops.track_from_anchors_batch(tb, list(call.inputs['off']), fr, ab, sc, sync=sync, ctx=ctx)
        det, best = ops.anchor_propagate_tracks_batch(out, tb, ts, sync=sync, ctx=ctx)
        return dict(tracks=out['tracks'], anchors=out['anchors'], ntracks=out['ntracks'], det=det, best=best, _held=(d, out))

    def want(self, call):
        import test_anchor_batch_gpu as AB
        tb, ts, fr, ab, sc = self.device(call)
        singles = AB.per_video(tb, ts, list(call.inputs['off']), fr, ab, sc)
        n = lambda k: [s[k].cpu().numpy() for s in singles]
        return dict(tracks=n(0), anchors=np.stack(n(1)), ntracks=np.stack(n(2)), det=n(3), best=np.stack(n(4)))

    def same(self, got, want):
        import test_anchor_batch_gpu as AB
        flat = lambda d: [x for k in self.keys for x in (d[k] if isinstance(d[k], list) else [d[k]])]
        a, b = flat(got), flat(want)
        return len(a) == len(b) and all(AB.same(x, y) for x, y in zip(a, b))

    def tab(self, call):
        off = tuple(int(x) for x in call.inputs['off'])
        return off if len(off) > 2 else None


register(AnchorRoute())


# ---- interpolation of strided tubelets (batch form) ---------------------------------------------------------------------------
class InterpBatch(Stage):
    """interp_tab: sampled offsets | dense offsets | frame table, keyed by its bytes (stage_table).  The halves of the pair
    have one byte length (V = 2, six sampled rows, thirteen dense frames) and differ in every part; one video of eighteen
    rows with a frame table brings the same number of bytes in another layout.  The rule is ``expected`` of
    tests/test_interp_tracks_gpu.py (oracle.tubelet_interpolation per slot), video by video."""
    name, keys = 'interpolate_tracks_batch', ('tracks', 'tboxes', 'boxes64', 'anchor', 'det', 'pooled', 'anchors')
    C, T = 2, 4
    # sampled offsets -> (first dense frame, stride, dense frames) per video
    GEO = {OFF_A: ((1, 2, 8), (2, 2, 5)), OFF_B: ((2, 2, 5), (1, 2, 8)), (0, 6): ((2, 2, 13),), (0, 18): ((1, 3, 54),)}

    @staticmethod
    @functools.lru_cache(maxsize=None)
    def case(off, seed):
        import test_interp_tracks_gpu as IT
        vids = []
        for v, (a, b) in enumerate(zip(off[:-1], off[1:])):
            n = b - a
            f0, stride, F = InterpBatch.GEO[off][v]
            rng = np.random.RandomState(seed + 10 * v)
            knots = {(c, t): sorted(rng.permutation(n)[:rng.randint(0, n + 1)].tolist()) for c in range(InterpBatch.C)
                     for t in range(InterpBatch.T)}
            knots[(0, 0)] = list(range(n))
            vids.append(IT.build_case('v%d' % v, seed + v, n, F, np.arange(f0, f0 + stride * n, stride), knots,
                                      nt=[InterpBatch.T - v % 2, 2 + (seed + v) % 2], C=InterpBatch.C, T=InterpBatch.T, with_boxes=True))
        return tuple(vids)

    def batch(self, off, seed):
        return Call(self.name, dict(vids=self.case(tuple(off), seed), off=tuple(off)), {})

    def probe(self):
        return self.batch(OFF_A, 9300)

    def wears(self):
        other = self.batch(OFF_B, 9310)
        return [('a_b_a', [self.probe(), other]),
                ('single_between', [other, self.batch((0, 6), 9320), other]),
                ('one_video_same_bytes', [self.batch((0, 18), 9330)])]

    @staticmethod
    def table_bytes(call):
        """the bytes of the host table a call stages (restated from vdet_interp_tracks_batch: the offsets travel only for V > 1)"""
        V, rows = len(call.inputs['off']) - 1, call.inputs['off'][-1]
        return (16 * (V + 1) if V > 1 else 0) + 4 * rows

    def run(self, ctx, call, sync=True):
        from vdetlib_amd import ops
        vids, off = call.inputs['vids'], call.inputs['off']
        C, T = self.C, self.T
        bo = dict(tracks=views(flat_of([c['tracks'] for c in vids], F32), off, C, T, 5),
                  tboxes=views(flat_of([c['boxes'] for c in vids], F32), off, C, T, 4),
                  det=views(flat_of([c['series'][0] for c in vids], F64), off, C, T, 1),
                  pooled=views(flat_of([c['series'][1] for c in vids], F64), off, C, T, 1),
                  anchors=g(np.stack([c['anchors'] for c in vids])), ntracks=g(np.stack([c['nt'] for c in vids])),
                  frame_off=np.asarray(off, np.int64))
        out = ops.interpolate_tracks_batch(bo, np.concatenate([c['frames'] for c in vids]), [c['F'] for c in vids], sync=sync, ctx=ctx)
        return dict({k: out[k] for k in self.keys}, _held=bo)

    def want(self, call):
        import test_interp_tracks_gpu as IT
        from oracle import oracle as o
        o.build()
        per = [IT.expected(o, c['tracks'], c['nt'], c['anchors'], c['series'], c['boxes'], c['frames'], c['F']) for c in call.inputs['vids']]
        r32 = lambda x: np.ascontiguousarray(x).astype(F32)           # the f32 outputs: the f64 values rounded once
        return dict(tracks=[r32(p['tracks']) for p in per], tboxes=[r32(p['boxes64']) for p in per], boxes64=[p['boxes64'] for p in per],
                    anchor=[p['anchor'] for p in per], det=[p['series'][0] for p in per], pooled=[p['series'][1] for p in per],
                    anchors=np.stack([p['anchors'] for p in per]))

    def same(self, got, want):
        import test_interp_tracks_gpu as IT
        V = len(want['tracks'])
        if any(len(got[k]) != V for k in self.keys):
            return False
        for v in range(V):
            if not all(got[k][v].dtype == F64 and IT.bits64(got[k][v], want[k][v]) for k in ('boxes64', 'anchor', 'det', 'pooled')):
                return False
            if not all(got[k][v].dtype == F32 and IT.bits32(got[k][v], want[k][v]) for k in ('tracks', 'tboxes', 'anchors')):
                return False
        return True


register(InterpBatch())
