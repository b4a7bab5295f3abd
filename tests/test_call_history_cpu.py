"""CPU-only: the wear calls of tests/history_harness.py do what test_call_history_gpu.py needs of them, by the numpy rules
alone.  A probe that returned the answer of the call before it must not pass, so for every (stage, wear) the rule's result of
the wear's last call differs from the probe's in EVERY output the two share; and each wear leaves what it was built to leave
(every link and live bit, every pair bit, an emptied selection, a table of the same length from other offsets)."""
import numpy as np
import pytest

import history_harness as H


def test_registry_is_complete_and_probes_are_stable():
    assert len(H.STAGES) >= 15 and len(H.pairs()) >= 3 * len(H.STAGES) - 6
    for name, st in H.STAGES.items():
        a, b = st.probe(), st.probe()
        assert a.stage == name and sorted(a.inputs) == sorted(b.inputs) and a.kw == b.kw
        for wear, calls in st.wears():
            assert calls and all(c.stage in H.STAGES for c in calls), (name, wear)
        if st.device_rule:
            continue
        assert set(st.keys) <= set(H.want_probe(name)), name
        assert st.same(H.want_probe(name), H.want_probe(name)), name       # (the comparator accepts the rule's own result)


@pytest.mark.parametrize("stage,wear", H.pairs(device_rules=False), ids=lambda x: x)
def test_wear_result_differs_from_the_probes(stage, wear):
    """``same_array`` is false for outputs of different shapes, so a wear of another R, T, F, C or top_num, and a wear whose
    last call is a batch where the probe is a single call, passes by shape alone -- rightly: a probe cannot return an answer of
    another shape.  The assertion has content where the shapes agree: the halves of an offset pair ([V,C]-shaped outputs and
    the per-video list as a whole), ``identical_same_shape``, ``thresh_above_all``, ``identical_t33``, ``twin_model`` /
    ``alternating``, ``high_sets_differ`` / ``other_offsets_same_shape`` / ``video_all_nan``; test_shape_equal_wears_exist
    keeps that list from emptying."""
    st = H.STAGES[stage]
    last = dict(st.wears())[wear][-1]
    wp, ww = H.want_probe(stage), H.want_wear(stage, wear)
    shared = [k for k in st.keys if k in H.STAGES[last.stage].keys]
    assert shared, "the wear's last call shares no output with the probe"
    for k in shared:
        assert not H.same_array(wp[k], ww[k]), (stage, wear, k)


def shapes_of(x):
    return [shapes_of(y) for y in x] if isinstance(x, list) else (np.shape(x), np.asarray(x).dtype)


def test_shape_equal_wears_exist():
    """every stage with a numpy rule has at least one wear whose answer has the probe's shapes in some output and other values"""
    for name, st in H.STAGES.items():
        if st.device_rule:
            continue
        wp, found = H.want_probe(name), False
        for wear, calls in st.wears():
            if calls[-1].stage in H.STAGES and set(st.keys) & set(H.STAGES[calls[-1].stage].keys):
                ww = H.want_wear(name, wear)
                found = found or any(k in ww and shapes_of(wp[k]) == shapes_of(ww[k]) and not H.same_array(wp[k], ww[k]) for k in st.keys)
        assert found, name


def test_interpolation_tables_have_one_byte_length():
    st = H.STAGES['interpolate_tracks_batch']
    wears = dict(st.wears())
    a, b, one = st.probe(), wears['a_b_a'][-1], wears['one_video_same_bytes'][-1]
    assert st.table_bytes(a) == st.table_bytes(b) == st.table_bytes(one) == 72
    dense = lambda c: [v['F'] for v in c.inputs['vids']]
    frames = lambda c: np.concatenate([v['frames'] for v in c.inputs['vids']])
    assert sum(dense(a)) == sum(dense(b)) and dense(a) != dense(b) and a.inputs['off'] != b.inputs['off']
    assert not np.array_equal(frames(a), frames(b))              # offsets, dense offsets and frame table all differ


@pytest.mark.parametrize("stage", ["seq_nms_w2", "seq_nms_w1"])
@pytest.mark.parametrize("wear", ["identical_r64", "identical_same_shape"])
def test_seqnms_identical_wear_sets_every_bit_and_leaves_live_nodes(stage, wear):
    import seqnms_spec as spec
    call = dict(H.STAGES[stage].wears())[wear][-1]
    t, nt = call.inputs['tracks'], call.inputs['ntracks']
    C, R, F = t.shape[:3]
    assert (nt == R).all() and np.isfinite(t).all() and call.kw['max_seqs'] == 1 and call.kw['nms_thres'] > 1
    for f in range(F - 1):                                    # every link of every pair of neighbouring frames
        assert spec.hit_matrix(t[0, :, f, :4], t[0, :, f + 1, :4], call.kw['link_thres']).all()
    w = H.want_wear(stage, wear)
    assert (w['nseq'] == 1).all() and not w['exhausted'].any()
    left = (w['seq'] == spec.LEFTOVER).any(axis=1)            # [C,F]: frames that still hold an unassigned live node
    assert (left.sum(axis=1) >= F - 1).all()


def test_seqnms_probes_run_to_exhaustion():
    for name in ("seq_nms_w2", "seq_nms_w1"):                  # a stale done flag would stop them early
        w = H.want_probe(name)
        assert w['exhausted'].all() and (w['nseq'] > 4).all() and (w['nseq'] < H.SQ_KW['max_seqs']).all()
    for per in H.want_probe("seq_nms_batch")['exhausted']:
        assert per.all()


def test_tcn_twin_nets_share_every_shape_and_no_weight():
    st = H.STAGES['tcn_tracks']
    a, b, wide = st.net('probe'), st.net('twin'), st.net('wide_first')
    assert [w.shape for w, _ in a.layers] == [w.shape for w, _ in b.layers] and a.inputs == b.inputs
    assert all(not np.array_equal(x, y) for (x, _), (y, _) in zip(a.layers, b.layers))
    assert a.packed()[0].nbytes == b.packed()[0].nbytes and np.array_equal(a.packed()[1], b.packed()[1])
    assert wide.layers[0][0].shape[0] > 8 * a.layers[0][0].shape[0]


def test_tubelet_identical_wear_sets_every_pair_bit():
    import tubenms_spec as spec
    call = dict(H.STAGES['nms_tubelets_full'].wears())['identical_t33'][-1]
    t, nt = call.inputs['tracks'], call.inputs['ntracks']
    C, T, F = t.shape[:3]
    assert (nt == T).all() and T == 33
    for c in range(C):
        S, I, n = spec.pair_sums(t[c, :, :, :4], spec.exists(t, nt)[c])
        assert (spec.tube_overlaps(S, I, n, call.kw['norm'], call.kw['min_shared']) >= call.kw['thresh']).all()
    w = spec.expected(t, nt, call.inputs['score'], None, None, (), call.kw['thresh'], call.kw['norm'], call.kw['reduce'],
                      call.kw['min_shared'])
    assert (w['ntracks'] == 1).all()


def test_tubelet_probes_sit_where_the_issue_puts_them():
    import tubenms_cases as cases
    p20, full = H.STAGES['nms_tubelets_nt20'].probe(), H.STAGES['nms_tubelets_full'].probe()
    assert p20.inputs['tracks'].shape[1] == 33 > cases.TILE and (p20.inputs['ntracks'] == 20).all()      # the second tile is skipped
    assert np.isfinite(p20.inputs['tracks'][:, 20:, :, 0]).sum() > 40                                     # boxes behind the count: never read
    w = H.want_probe('nms_tubelets_full')
    assert (full.inputs['ntracks'] == 33).all() and (w['ntracks'] == 33).all()                            # distinct: nothing is suppressed
    assert 0 < H.want_probe('nms_tubelets_nt20')['ntracks'].min() and H.want_probe('nms_tubelets_nt20')['ntracks'].max() < 20


def test_top_anchors_probe_and_wears():
    import test_top_anchors_gpu as TA
    st = H.STAGES['top_anchors']
    p = st.probe()
    F, B, C = p.inputs['scores'].shape
    assert TA.ROWS < F * B <= 2 * TA.ROWS                    # two row segments
    wears = dict(st.wears())
    w = H.want_wear('top_anchors', 'thresh_above_all')
    assert (w['frames'] == 0).all() and (w['index'] == -1).all()       # zero candidates in every class
    assert wears['thresh_above_all'][-1].kw['score_thresh'] > p.inputs['scores'].max()
    wide = wears['batch_v3_c70'][-1]
    assert wide.inputs['scores'].shape[2] > 64 and len(wide.kw['frame_off']) == 4
    assert wears['top_beyond_candidates'][-1].kw['top_num'] > F * B
    small, big = wears['regrow']
    hist = lambda c: (c.inputs['scores'].shape[0] if c.kw.get('mode') == 'frame' else 1) * c.inputs['scores'].shape[2]
    assert hist(small) < hist(p) < hist(big)                 # the probe's histograms lie inside a regrown, re-cleared buffer


def test_offset_pairs_have_one_key_length_and_one_total():
    for a, b in ((H.OFF_A, H.OFF_B), (H.OFF_A8, H.OFF_B8)):
        ka, kb = np.asarray(a, np.int64).tobytes(), np.asarray(b, np.int64).tobytes()
        assert len(ka) == len(kb) and ka != kb and a[0] == b[0] == 0 and a[-1] == b[-1]
        assert all(y > x for x, y in zip(a[:-1], a[1:])) and all(y > x for x, y in zip(b[:-1], b[1:]))
    seen = 0
    for name, st in H.STAGES.items():
        pt = st.tab(st.probe())
        if pt is None or name == 'top_anchors':
            continue
        others = {H.tab_of(c) for _, calls in st.wears() for c in calls} - {None, pt}
        assert any(len(o) == len(pt) and o[-1] == pt[-1] for o in others), name      # a wear stages the pair's other half
        seen += 1
    assert seen >= 7
