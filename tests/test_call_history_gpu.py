"""-m gpu: a result depends on the call's arguments alone, never on what the context ran before.  Every stage of
tests/history_harness.py is probed on a context that a wear call has just left in the state most likely to leak -- scratch
with every bit set, a resident per-video table of the same length from other offsets, a wider stride, an emptied histogram
-- and the probe must equal the stage's numpy rule AND, byte for byte, the same probe on a context that ran nothing else.
test_call_history_cpu.py shows from the rules alone that every wear's own answer differs from the probe's in every output, so
a probe that returned what the call before it left would fail here.

  1. test_probe_after_wear          one wear, then the probe: the prep cache off and on, one ID per environment of the stage
  2. test_round_robin_orders        every probe on ONE context in three orders, two laps each
  3. test_async_chain               the same laps without a single host wait between the calls; the waits of the second lap
                                    are exactly the changes of the resident per-video table, counted from the call list
  4. test_tables_reused_and_replaced  the resident table is taken when the offsets repeat and replaced when they change
     test_tcn_parameter_tables_...   ... and the TCN's parameter table likewise (vdet_query 10 / 11: without these two, 1. could
                                    pass without the resident-table path ever being taken)
     test_interpolation_table_...    ... and the interpolation's offset / frame table, by the host waits a replacement costs
  5. test_global_then_lds           Seq-NMS: the predecessor table moves from global scratch to LDS on one context
  6. test_two_evaluators_...        a VOC and an ILSVRC DetEvaluator interleaved on one context"""
import numpy as np
import pytest

import history_harness as H

pytestmark = pytest.mark.gpu

_ALONE = {}


def alone(stage, env, cache):
    """the probe on a context that ran nothing else: once per (stage, environment, cache), shared and never modified"""
    key = (stage, tuple(sorted((env or {}).items())), cache)
    if key not in _ALONE:
        st = H.STAGES[stage]
        with H.context(env, cache) as cx:
            _ALONE[key] = H.host(st.run(cx, st.probe()))
    return _ALONE[key]


# 1. -------------------------------------------------------------------------------------------------------------------
ENV_IDS = {None: 'default', 'VDET_SEQNMS_LDS': 'seqnms_global', 'VDET_TCN_GLOBAL': 'tcn_global', 'VDET_CTX_RECORDS': 'ctx_records_off'}


def wear_cases():
    """(stage, wear, environment) of every stage, one test ID each: a failure names the path it happened on"""
    return [pytest.param(n, w, env, id="%s-%s-%s" % (n, w, ENV_IDS[next(iter(env)) if env else None]))
            for n, w in H.pairs() for env in H.STAGES[n].envs]


@pytest.mark.parametrize("cache", [False, True], ids=["cache_off", "cache_on"])
@pytest.mark.parametrize("stage,wear,env", wear_cases())
def test_probe_after_wear(stage, wear, env, cache):
    st = H.STAGES[stage]
    want = H.want_probe(stage)
    with H.context(env, cache) as cx:
        calls = dict(st.wears())[wear]
        held = [H.run_call(cx, call) for call in calls]
        cx.sync()
        if st.device_rule and calls[-1].stage == stage:       # (what the CPU file shows for every other stage)
            assert not any(H.same_array(H.host(held[-1])[k], want[k]) for k in getattr(st, 'differ_keys', st.keys)), \
                "the wear gives the probe's answer"
        got = H.host(st.run(cx, st.probe()))
        st.check_path(cx, env)
    del held
    assert st.same(got, want), "the probe after the wear is not the rule's result"
    assert H.bitwise(got, alone(stage, env, cache)), "the probe after the wear is not the fresh context's"
    assert st.same(alone(stage, env, cache), want), "the probe on a fresh context is not the rule's result"


# 2. and 3. ------------------------------------------------------------------------------------------------------------
def orders():
    names = list(H.STAGES)
    shuffled = [names[i] for i in np.random.RandomState(17).permutation(len(names))]
    return (('registry', names), ('reversed', names[::-1]), ('shuffled', shuffled))


@pytest.mark.parametrize("order", orders(), ids=lambda o: o[0])
def test_round_robin_orders(order):
    with H.context(None, cache=True) as cx:
        for lap in range(2):
            for name in order[1]:
                got = H.host(H.STAGES[name].run(cx, H.STAGES[name].probe()))
                assert H.STAGES[name].same(got, H.want_probe(name)), (order[0], lap, name)


def table_changes(names, resident):
    """(changes of the resident per-video table over the probes of ``names``, the table resident afterwards): a probe that
    stages offsets other than the resident ones replaces the table, and -- a copy of the old one may be in flight -- waits"""
    n = 0
    for name in names:
        tab = H.tab_of(H.STAGES[name].probe())
        if tab is not None and tuple(tab) != resident:
            n += resident is not None
            resident = tuple(tab)
    return n, resident


@pytest.mark.parametrize("order", orders(), ids=lambda o: o[0])
def test_async_chain(order):
    names = order[1]
    first, resident = table_changes(names, None)
    second, _ = table_changes(names, resident)
    assert first >= 1 and second >= 2                  # (the registry does make the table change inside a lap)
    with H.context(None, cache=True, asynchronous=True) as cx:
        held, waits = [], []
        for lap in range(2):
            before = cx.query(8)
            for name in names:
                held.append((lap, name, H.STAGES[name].run(cx, H.STAGES[name].probe(), sync=False)))
            waits.append(cx.query(8) - before)
        cx.sync()
        print("host waits per lap %r; table changes from the call list: %d, %d" % (waits, first, second))
        for lap, name, out in held:
            assert H.STAGES[name].same(H.host(out), H.want_probe(name)), (order[0], lap, name)
        assert waits[1] == second, "the second lap waited for the device where no per-video table changed"


# 4. -------------------------------------------------------------------------------------------------------------------
def test_tables_reused_and_replaced():
    S = H.STAGES
    sq, tube, resc, merge, top = S['seq_nms_batch'], S['nms_tubelets_batch'], S['rescore_tubelets_batch'], S['merge_tracks_batch'], \
        S['top_anchors']
    hard, route = S['nms_tracks_batch'], S['anchor_route_batch']
    a, b = sq.probe(), sq.batch(H.OFF_B, 9930)
    steps = [(a, 1, 'the first table'), (a, 0, 'the same offsets again'), (b, 1, 'other offsets of the same length'),
             (S['seq_nms_w2'].probe(), 0, 'one video stages nothing'), (b, 0, 'and leaves the table resident'),
             (resc.batch(H.OFF_B, 9140), 0, 'another stage, the same offsets'), (merge.probe(), 1, 'another stage, other offsets'),
             (hard.probe(), 0, 'a third stage, the same offsets'), (resc.probe(), 0, 'a fourth'),
             (resc.batch((0, 6), 9150), 0, 'a batch of one video'), (resc.batch(H.OFF_B, 9140), 1, 'back to the other half'),
             (tube.probe(), 1, 'eight frames'), (tube.batch(H.OFF_B8, 2, 33, 9951), 1, 'their other half'),
             (top.wears()[0][1][0], 1, 'top_anchors stages its own offsets'), (top.probe(), 0, 'and none without'),
             (top.wears()[0][1][0], 0, 'the same offsets again'), (a, 1, 'the first offsets once more'),
             (route.probe(), 0, 'the anchor route (tracker and propagation) takes the resident table'),
             (route.batch(H.OFF_B, 9991), 1, 'and replaces it'), (route.batch(H.OFF_B, 9991), 0, 'once'),
             (route.batch((0, 6), 9992), 0, 'one video'), (b, 0, 'Seq-NMS takes the route\'s table'), (route.probe(), 1, 'back')]
    with H.context(None, cache=True) as cx:
        assert cx.query(11) == 0
        resident = None
        for k, (call, delta, what) in enumerate(steps):
            tab = H.tab_of(call)
            assert delta == int(tab is not None and tuple(tab) != resident), (k, what)      # (the steps say what tab() says)
            resident = resident if tab is None else tuple(tab)
            before = cx.query(11)
            got = H.host(H.run_call(cx, call))
            assert cx.query(11) - before == delta, (k, what)
            st = S[call.stage]
            assert st.same(got, st.want(call)), (k, what)


def test_tcn_parameter_tables_reused_and_replaced():
    st = H.STAGES['tcn_tracks']
    steps = [('probe', 1), ('probe', 0), ('twin', 1), ('twin', 0), ('probe', 1), ('wide_first', 1), ('probe', 1), ('probe', 0)]
    want = {}
    with H.context(None, cache=True) as cx:
        assert cx.query(10) == 0
        for k, (net, delta) in enumerate(steps):
            call = st.call(net)
            before = cx.query(10)
            got = H.host(st.run(cx, call))
            assert cx.query(10) - before == delta, (k, net)          # one upload per change of the net, none on a repeat
            if net not in want:
                want[net] = st.want(call)
            assert st.same(got, want[net]), (k, net)
    assert not st.same(want['probe'], want['twin'])


def test_interpolation_table_reused_and_replaced():
    """interp_tab has no upload counter; a replaced table waits for the stream once (a copy of the old bytes may be in flight),
    the same bytes again wait for nothing: vdet_query 8 in asynchronous calls"""
    st = H.STAGES['interpolate_tracks_batch']
    wears = dict(st.wears())
    a, b, one = st.probe(), wears['a_b_a'][-1], wears['one_video_same_bytes'][-1]
    steps = [(a, 0, 'the first table: nothing in flight'), (a, 0, 'the same bytes'), (b, 1, 'the other half: as many bytes, all different'),
             (b, 0, 'again'), (one, 1, 'one video, as many bytes'), (a, 1, 'back'), (a, 0, 'again')]
    with H.context(None, cache=True, asynchronous=True) as cx:
        held = []
        for k, (call, delta, what) in enumerate(steps):
            before = cx.query(8)
            held.append((call, st.run(cx, call, sync=False)))
            assert cx.query(8) - before == delta, (k, what)
        cx.sync()
        for k, (call, out) in enumerate(held):
            assert st.same(H.host(out), st.want(call)), k


# 5. -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stage", ["seq_nms_w2", "seq_nms_w1", "seq_nms_batch"])
def test_global_then_lds(stage):
    st = H.STAGES[stage]
    long = dict(H.STAGES['seq_nms_w2'].wears())['global_path_first'][0]
    with H.context(None, cache=True) as cx:
        assert cx.query(14) == -1
        H.run_call(cx, long)
        assert cx.query(14) == 2                       # the long video's table lay in global scratch ...
        got = H.host(st.run(cx, st.probe()))
        assert cx.query(14) == 1                       # ... the probe's in LDS
    assert st.same(got, H.want_probe(stage)) and H.bitwise(got, alone(stage, None, True))


# 6. -------------------------------------------------------------------------------------------------------------------
def test_two_evaluators_interleaved_on_one_context():
    """The ev_* scratch is shared by every DetEvaluator of a context.  A VOC and an ILSVRC evaluator fed video by video in turn
    (the second one the videos in reverse order): each one's stream and APs are, bit for bit, those of the same evaluator fed
    alone.  DetEvaluator takes no context: all of them run on the process-wide one, so the evaluator fed alone does not start
    from a fresh context either -- it runs after whatever the session ran before, and this test pins the interleaving only."""
    import torch
    from test_eval_gpu import _tubelet_videos
    from vdetlib_amd import eval as vev, ops
    vids = _tubelet_videos()
    gt = vev.gt_table_from_annots([v[0] for v in vids])

    def feed(evs):
        """video i to the first evaluator, then video n-1-i to the second: the two streams differ in their order at least"""
        for i in range(len(vids)):
            for ev, k in zip(evs, (i, len(vids) - 1 - i)):
                if ev is not None:
                    annot, _, _, tr, nt, pooled, ob = vids[k]
                    ev.add_tracks(annot['video'], tr, nt, pooled, ob)

    def result(ev):
        return [t.cpu() for t in ev.stream(raw=True)], ev.compute()

    solo = {}
    for rule in ('voc', 'ilsvrc'):
        ev = ops.DetEvaluator(gt, rule=rule)
        feed([ev, None] if rule == 'voc' else [None, ev])
        solo[rule] = result(ev)
    voc, ils = ops.DetEvaluator(gt, rule='voc'), ops.DetEvaluator(gt, rule='ilsvrc')
    feed([voc, ils])
    for ev, rule in ((voc, 'voc'), (ils, 'ilsvrc'), (voc, 'voc'), (ils, 'ilsvrc')):       # compute() in turn as well
        stream, (aps, m) = result(ev)
        assert len(stream) == len(solo[rule][0]) and all(torch.equal(x, y) for x, y in zip(stream, solo[rule][0])), rule
        assert aps == solo[rule][1][0] and m == solo[rule][1][1], rule
    assert solo['voc'][0][0].numel() > 50 and solo['voc'][1][1] > 0.5
    # the two do not hold one stream: an evaluator that read the other's scratch would show
    assert not all(torch.equal(x, y) for x, y in zip(solo['voc'][0], solo['ilsvrc'][0]))
