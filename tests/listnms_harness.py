"""What the GPU files of the per-frame list NMS family share (test_nms_tracks_gpu.py, test_softnms_gpu.py, test_votenms_gpu.py):
the device call against the rule's numpy `expected` ON BITS, the guard-pattern buffers of the C-ABI tests and the wide lists that
sit on the waves-per-workgroup breaks.  A file describes its rule once -- ``ListNms(op, expected, own rows, ...)`` -- and binds
the helpers it uses.  torch is imported where a function needs the GPU, never at import."""
import functools

import numpy as np

import synth
from test_nms_tracks_cpu import same_bits, still_of

ROWS = (('tracks', 5, np.float32), ('score', 1, np.float64), ('src', 1, np.int32))      # the per-row outputs of every rule


def dev(x):
    import torch
    return None if x is None else torch.from_numpy(np.array(x)).cuda()


def guards_intact(o, sizes, G, fill=7.25, ifill=12345):
    return all(bool((o[k][n:] == (fill if o[k].dtype.is_floating_point else ifill)).all()) and o[k].numel() == n + G
               for k, n in sizes.items())


@functools.lru_cache(maxsize=None)
def wide_lists(nmax):
    """C = 1, F = 2: nmax - 11 still-image rows of overlapping boxes (every box of the frame, descending score) and 11 tubelet
    rows that are jittered copies of detection boxes"""
    rng = np.random.RandomState(nmax)
    T, B = 11, nmax - 11
    boxes = np.stack([synth.boxes_1(rng, B, degenerate=B // 3) for _ in range(2)])
    scores = np.stack([synth.tie_free_scores(rng, B) for _ in range(2)])[:, :, None]
    ki = np.stack([np.argsort(-scores[f, :, 0], kind='stable') for f in range(2)]).astype(np.int32)[:, None]
    tracks = np.zeros((1, T, 2, 5), np.float32)
    for f in range(2):
        tracks[0, :, f, :4] = boxes[f, rng.permutation(B)[:T]] + rng.randint(-3, 4, (T, 4))
    return tracks, np.array([T], np.int32), rng.rand(1, T, 2), (boxes, scores, ki, np.full((2, 1), B, np.int32))


class ListNms(object):
    """The helpers of one rule.  ``op``: the name of the single-video function of vdetlib_amd.ops; ``expected``: the rule in
    numpy; ``own``: the rule's per-row outputs behind ROWS, as ROWS; ``case_thresh``: the thresh of ``check_case`` where the
    caller names none; ``op_kw``: what ``run`` passes to the op where the caller does not; ``equal``: the file's own
    outputs_equal where it has one."""

    def __init__(self, op, expected, own=(), case_thresh=None, op_kw=None, equal=None):
        self.op, self.expected, self.rows, self.case_thresh, self.op_kw = op, expected, ROWS + tuple(own), case_thresh, op_kw or {}
        self.row_keys = tuple(k for k, _, _ in self.rows)
        if equal is not None:
            self.outputs_equal = equal

    def host(self, out):
        return {k: out[k].cpu().numpy() for k in self.row_keys + ('cnt', 'ntracks')}

    def outputs_equal(self, got, want):
        """the per-row outputs by bit pattern (a NaN equal to a NaN), cnt and ntracks equal"""
        return all(same_bits(got[k], want[k]) for k in self.row_keys) and \
            np.array_equal(got['cnt'], want['cnt']) and np.array_equal(got['ntracks'], want['ntracks']) and \
            got['cnt'].dtype == np.int32 and got['ntracks'].dtype == np.int32

    def run(self, tracks, ntracks, score, tboxes=None, still=None, **kw):
        """the op on device copies -> numpy; the inputs must come back bit-identical"""
        from vdetlib_amd import ops
        ins = [tracks, ntracks, score, tboxes] + list(still or ())
        d = [dev(x) for x in ins]
        out = self.host(getattr(ops, self.op)(d[0], d[1], d[2], tboxes=d[3], still=tuple(d[4:]) if still is not None else None,
                                              **dict(self.op_kw, **kw)))
        for x, y in zip(ins, d):
            assert x is None or same_bits(y.cpu().numpy(), np.ascontiguousarray(x))
        return out

    def want_of(self, tracks, ntracks, score, tboxes=None, still=None, **kw):
        kw = dict(kw)
        cap = kw.pop('cap', None)
        return self.expected(tracks, ntracks, score, tboxes, still, R=cap, **kw)

    def check(self, tracks, ntracks, score, tboxes=None, still=None, **kw):
        want = self.want_of(tracks, ntracks, score, tboxes, still, **kw)
        got = self.run(tracks, ntracks, score, tboxes, still, **kw)
        assert self.outputs_equal(got, want)
        return got

    def check_case(self, case, tboxes=True, still=True, score=None, **kw):
        kw.setdefault('thresh', self.case_thresh)
        return self.check(case['tracks'], case['ntracks'], case['score'] if score is None else score,
                          case['tboxes'] if tboxes else None, still_of(case) if still else None, **kw)

    # ---- the C-ABI tests: flat outputs with a guard pattern of G elements behind them -------------------------------------------
    def sizes_of(self, C, R, Ft, V):
        N = C * R * Ft
        return dict([(k, N * per) for k, per, _ in self.rows], cnt=C * Ft, ntracks=V * C)

    def c_buffers(self, C, R, Ft, V, G, fill=7.25, ifill=12345):
        import torch
        dtypes = dict([(k, dt) for k, _, dt in self.rows], cnt=np.int32, ntracks=np.int32)
        return {k: torch.full((n + G,), fill if np.dtype(dtypes[k]).kind == 'f' else ifill, dtype=getattr(torch, np.dtype(dtypes[k]).name)).cuda()
                for k, n in self.sizes_of(C, R, Ft, V).items()}

    def video_of(self, out, v, off):
        """video v of a batch result -> numpy, in the single-video layout"""
        one = {k: out[k][v].cpu().numpy() for k in self.row_keys}
        one.update(cnt=out['cnt'][:, int(off[v]):int(off[v + 1])].cpu().numpy(), ntracks=out['ntracks'][v].cpu().numpy())
        return one
