#!/usr/bin/env python3
"""Generate tests/golden/svmhead_golden.json.gz from THE REFERENCE ITSELF (see make_golden.py: runs only where the reference
is available; nothing of the reference is written into the repository -- the fixture holds seeds and recorded outputs).

rcnn_scoring and rcnn_sampling_scoring (vdet/tubelet_cls.py:102-194) run with the image reader stubbed (it returns the frame
number), svm_from_rcnn_model returning the seeded model of tests/svm_spec.py (golden_model) and googlenet_features replaced by
svm_spec.golden_features, a closed form of (frame, box) that a test rebuilds bit for bit: no features are stored.  The
reference's own svm_scores and sampling_boxes run; np.random.seed(seed) precedes every call, so a test redraws the same offsets
in the reference's frame-loop order.  Recorded per class and tubelet: frame, det_score and bbox of every box, and for the
sampling scorer the index of the winning window.

The maker ASSERTS that in every group the best and the second-best window differ by more than 1e-6: np.dot's summation order
and the device's cannot then pick different winners.

    python tests/golden/make_svmhead_golden.py
"""
import copy
import gzip
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import make_golden  # noqa: E402
import svm_spec  # noqa: E402

CASES = [dict(seed=9300, F=5, T=3, K=40, samples_per_box=4, classes=[1, 7]),
         dict(seed=9301, F=5, T=3, K=40, samples_per_box=32, classes=[1, 7])]
MARGIN = 1e-6


def record(tubelets, args=None):
    out = []
    for tub in tubelets:
        rec = {'frame': [b['frame'] for b in tub['boxes']], 'det_score': [float(b['det_score']) for b in tub['boxes']],
               'bbox': [[float(x) for x in b['bbox']] for b in tub['boxes']]}
        if args is not None:
            rec['arg'] = [int(args[(id(tub), b['frame'])]) for b in tub['boxes']]
        out.append(rec)
    return out


def main():
    R = make_golden.load_reference()
    T = R['T']
    ref_svm_scores = T.svm_scores
    out = []
    for case in CASES:
        K, spb = case['K'], case['samples_per_box']
        vid, trp = svm_spec.golden_protos(case)
        assert any(len(t) < case['F'] for t in trp['tracks'])                     # tubelets with holes
        seen = []
        T.imread = lambda path: int(os.path.splitext(os.path.basename(path))[0]) + 1
        T.svm_from_rcnn_model = lambda model: svm_spec.golden_model(case['seed'], K)
        T.googlenet_features = lambda img, bxs, net, layer: svm_spec.golden_features(img, bxs, K)

        def spy(feats, model):
            s = ref_svm_scores(feats, model)
            seen.append(s)
            return s
        T.svm_scores = spy
        rec = dict(case, plain={}, sampling={})
        for class_idx in case['classes']:
            col = R['D'].index_vdet_to_det[class_idx] - 1
            np.random.seed(case['seed'])
            rec['plain'][str(class_idx)] = record(T.rcnn_scoring(vid, copy.deepcopy(trp), None, class_idx, None))
            del seen[:]
            np.random.seed(case['seed'])
            tubs = T.rcnn_sampling_scoring(vid, copy.deepcopy(trp), None, class_idx, None, samples_per_box=spb)
            # the winners and their margins, from the reference's own window scores, frame by frame
            args, k = {}, 0
            for frame in vid['frames']:
                here = [tub for tub in tubs if any(b['frame'] == frame['frame'] for b in tub['boxes'])]
                if not here:
                    continue
                s = seen[k][:, col].reshape(len(here), spb + 1)
                k += 1
                top = np.sort(s, axis=1)
                assert (top[:, -1] - top[:, -2] > MARGIN).all(), "best and second-best window closer than %g" % MARGIN
                for tub, a in zip(here, np.argmax(s, axis=1)):
                    args[(id(tub), frame['frame'])] = a
            assert k == len(seen)
            rec['sampling'][str(class_idx)] = record(tubs, args)
        T.svm_scores = ref_svm_scores
        out.append(rec)
    path = os.path.join(HERE, 'svmhead_golden.json.gz')
    with gzip.GzipFile(path, 'wb', mtime=0) as f:
        f.write(json.dumps({'cases': out}, separators=(',', ':'), sort_keys=True).encode())
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
