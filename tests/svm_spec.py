"""The specification of ops.svm_head in numpy, and the inputs its tests share (no GPU, no product code).

head() restates include/vdet_hip.h (vdet_svm_head): per window the ONE class column of svm_scores (reference
vdet/image_det.py:109-114), per box the max / argmax over its windows by np.argmax's rules (vdet/tubelet_cls.py:166-189), and
the scatter into [C,T,F].  Every product and sum is one rounded numpy operation in the compute dtype, in the order the header
fixes:

  1. unit u = k // 8 belongs to lane u % 64 (round u // 64): lane l owns k = (r*64 + l)*8 + i, i = 0..7, while k < K;
  2. a lane adds (feat[k]*scale) * W[k] to one accumulator from +0, k ascending; a k >= K adds nothing;
  3. the butterfly acc[l] = acc[l] + acc[l ^ d] for d = 32, 16, 8, 4, 2, 1, all lanes at once; lane 0's value;
  4. + B[col].
"""
import numpy as np

UNIT, LANES = 8, 64
ROUND = UNIT * LANES


def widen(features, cdt):
    """Feature storage -> compute dtype, exactly.  bfloat16 travels as a uint16 array of the upper halves of float32."""
    features = np.asarray(features)
    if features.dtype == np.uint16:
        return (features.astype(np.uint32) << 16).view(np.float32).astype(cdt)
    return features.astype(cdt)


def to_bf16(x):
    """float32 -> bfloat16 bits (uint16), round to nearest even (finite inputs)."""
    u = np.asarray(x, np.float32).view(np.uint32)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def window_scores(features, W, B, scale, col, cdt):
    """s [M]: features [M,K] (any storage), col [M] the column of W per window; everything in cdt, in the fixed order."""
    cdt = np.dtype(cdt)
    feat = widen(features, cdt)
    M, K = feat.shape
    col = np.asarray(col, np.int64)
    with np.errstate(all='ignore'):
        p = feat * cdt.type(scale)                                # rounded once
        acc = np.zeros((M, LANES), cdt)
        lane = np.arange(LANES)
        Wc = np.asarray(W).astype(cdt)
        for r in range((K + ROUND - 1) // ROUND):
            for i in range(UNIT):
                k = (r * LANES + lane) * UNIT + i                 # [64]
                live = k < K
                if not live.any():
                    continue
                kk = k[live]
                acc[:, live] = acc[:, live] + p[:, kk] * Wc[kk][:, col].T
        for d in (32, 16, 8, 4, 2, 1):
            acc = acc + acc[:, lane ^ d]
        s = acc[:, 0]
        if B is not None:
            s = s + np.asarray(B).reshape(-1).astype(cdt)[col]
    return s


def argmax_first(s):
    """np.argmax's rule, written out: the first maximum wins, a NaN wins at its first occurrence.  s: a non-empty 1-D list."""
    best, arg = s[0], 0
    for j in range(1, len(s)):
        if best == best and (s[j] > best or s[j] != s[j]):
            best, arg = s[j], j
    return best, arg


def head(features, W, B, scale, cdt, group=1, slot=None, count=None, shape=None, cols=None, sboxes=None, ok=None, out=None):
    """The whole call.  Returns a dict like ops.svm_head's, numpy arrays; bad = the groups the call refuses (a slot outside
    shape, a column outside W): skipped, and the device raises at its sync."""
    cdt = np.dtype(cdt)
    features = np.asarray(features)
    Mw, K = features.shape
    G = int(group)
    N = Mw // G
    Mcols = np.asarray(W).shape[1]
    n = N if count is None else max(0, min(int(count), N))
    det = arg = tboxes = None
    if slot is not None:
        if out is not None:
            det, arg = out['det'].copy(), out['arg'].copy()
            tboxes = None if out.get('tboxes') is None else out['tboxes'].copy()
            C, T, F = det.shape
        else:
            C, T, F = shape
            det = np.full((C, T, F), np.nan, cdt)
            arg = np.full((C, T, F), -1, np.int32)
            tboxes = np.full((C, T, F, 4), np.nan) if sboxes is not None else None
    else:
        C, T, F = 1, 1, 1
        tboxes = np.full((N, 4), np.nan) if sboxes is not None else None       # (the device leaves skipped rows unwritten)
    score = np.full((N,), np.nan, cdt)
    arg_flat = np.full((N,), -1, np.int32)
    okm = np.ones((N, G), bool) if ok is None else np.asarray(ok).reshape(N, G) != 0
    valid = np.zeros(N, bool)
    col = np.zeros(N, np.int64)
    bad = []
    for g in range(n):
        c, t, f = (0, 0, 0) if slot is None else (int(x) for x in slot[g])
        if not (0 <= c < C and 0 <= t < T and 0 <= f < F):
            bad.append(g)
            continue
        cg = c if cols is None else int(cols[c])
        if not 0 <= cg < Mcols:
            bad.append(g)
            continue
        valid[g], col[g] = True, cg
    rows = np.flatnonzero(np.repeat(valid, G) & okm.reshape(-1))
    s_all = np.full((N * G,), np.nan, cdt)
    if len(rows):
        s_all[rows] = window_scores(features[rows], W, B, scale, np.repeat(col, G)[rows], cdt)
    nbad = 0
    for g in np.flatnonzero(valid):
        js = np.flatnonzero(okm[g])
        if len(js):
            best, a = argmax_first([s_all[g * G + j] for j in js])
            a = int(js[a])
            box = None if sboxes is None else np.asarray(sboxes)[g, a]
        else:
            best, a, box = cdt.type(np.nan), -1, np.full(4, np.nan)
            nbad += 1
        score[g], arg_flat[g] = best, a
        if slot is not None:
            c, t, f = (int(x) for x in slot[g])
            det[c, t, f], arg[c, t, f] = best, a
            if tboxes is not None:
                tboxes[c, t, f] = box
        elif tboxes is not None:
            tboxes[g] = box
    return dict(det=det, arg=arg, tboxes=tboxes, score=score, arg_flat=arg_flat, nbad=nbad, bad=bad, windows=s_all)


# ---- the recipe the golden fixture and its tests share ------------------------------------------------------------------

def golden_model(seed, K):
    """The seeded SVM model of tests/golden/make_svmhead_golden.py: W f64 [K,200], B f64 [1,200], feat_norm_mean f64 scalar."""
    rng = np.random.RandomState(seed)
    return {'W': rng.uniform(-1, 1, (K, 200)), 'B': rng.uniform(-0.5, 0.5, (1, 200)), 'feat_norm_mean': np.float64(19.0 + rng.rand())}


def golden_features(frame_id, boxes, K):
    """The closed form that stands in for the net: f32 [n,K] from (frame, box), elementwise f64 multiplies and adds in this
    order, then one cast.  feat[i,k] = ((x1*a_k + y1*b_k) + (x2*c_k + y2*d_k)) * 0.01 + frame * e_k with a_k = 0.001*(k+1),
    b_k = 0.002*(k % 7), c_k = 0.0015*(k % 5 + 1), d_k = 0.0005*(k % 11), e_k = 0.01*(k % 3 - 1)."""
    b = np.asarray(boxes, np.float64).reshape(-1, 4)
    k = np.arange(K, dtype=np.float64)
    a_k, b_k, c_k, d_k, e_k = 0.001 * (k + 1), 0.002 * (k % 7), 0.0015 * (k % 5 + 1), 0.0005 * (k % 11), 0.01 * (k % 3 - 1)
    t1 = b[:, 0:1] * a_k[None] + b[:, 1:2] * b_k[None]
    t2 = b[:, 2:3] * c_k[None] + b[:, 3:4] * d_k[None]
    return ((t1 + t2) * 0.01 + np.float64(frame_id) * e_k[None]).astype(np.float32)


def golden_tubelets(seed, F, T):
    """T tubelets over F frames (1-based) with holes: lists of {'frame', 'bbox', 'score', 'anchor'} -- track_proto['tracks']."""
    rng = np.random.RandomState(seed + 1)
    tracks = []
    for t in range(T):
        tr = []
        for f in range(F):
            if rng.rand() < 0.25:
                continue
            x1, y1 = rng.uniform(5, 200), rng.uniform(5, 150)
            tr.append({'frame': f + 1, 'bbox': [float(x1), float(y1), float(x1 + rng.uniform(10, 120)), float(y1 + rng.uniform(10, 90))],
                       'score': float(rng.rand()), 'anchor': f})
        tracks.append(tr)
    return tracks


def golden_protos(case):
    name = 'svmhead_%d' % case['seed']
    vid = {'video': name, 'root_path': '/synthetic/' + name,
           'frames': [{'frame': f + 1, 'path': '%06d.JPEG' % f} for f in range(case['F'])]}
    return vid, {'video': name, 'method': 'recipe', 'tracks': golden_tubelets(case['seed'], case['F'], case['T'])}
