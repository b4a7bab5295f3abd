#!/usr/bin/env python3
"""Generate tests/golden/rescore_golden.json.gz from THE REFERENCE ITSELF (see make_golden.py: runs only where the reference
is available; nothing of the reference is written into the repository -- the fixture holds seeds and recorded outputs).

Inputs: the recipe of tests/rescore_spec.py (volume + tubelets WITH holes), by seed.  Recorded, per class and tubelet:
  maxpool   raw_dets_spatial_max_pooling (which ends in do_score_completion): det_score and bbox of every box, then
            score_proto_temporal_maxpool with windows 3 and 5
  sampling  rcnn_sampling_dets_scoring with the image reader and the CNN / SVM scorers stubbed to return planted scores
            (rescore_spec.planted_floor): det_score and bbox of every box

    python tests/golden/make_rescore_golden.py
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
import rescore_spec  # noqa: E402

CASES = [dict(seed=9100, F=9, B=5, C=2, T=3, overlap_thres=0.7),
         dict(seed=9101, F=9, B=300, C=2, T=3, overlap_thres=0.7)]


def protos(case, boxes, scores, tracks, c):
    name = 'rescore_%d' % case['seed']
    F = case['F']
    vid = {'video': name, 'root_path': '/synthetic/' + name,
           'frames': [{'frame': f + 1, 'path': '%06d.JPEG' % f} for f in range(F)]}
    tr = []
    for t in range(case['T']):
        tr.append([{'frame': f + 1, 'bbox': [float(x) for x in tracks[c, t, f, :4]], 'score': float(tracks[c, t, f, 4]), 'anchor': f}
                   for f in range(F) if not np.isnan(tracks[c, t, f, 0])])
    return vid, {'video': name, 'method': 'recipe', 'tracks': tr}


def record(tubelets, extra=()):
    out = []
    for k, tub in enumerate(tubelets):
        rec = {'frame': [b['frame'] for b in tub['boxes']], 'det_score': [float(b['det_score']) for b in tub['boxes']],
               'bbox': [[float(x) for x in b['bbox']] for b in tub['boxes']]}
        for name, other in extra:
            rec[name] = [float(b['det_score']) for b in other[k]['boxes']]
        out.append(rec)
    return out


def main():
    R = make_golden.load_reference()
    T = R['T']
    out = []
    for case in CASES:
        boxes, scores = rescore_spec.volume(case['seed'], case['F'], case['B'], case['C'])
        tracks, floor = rescore_spec.tubelets(case['seed'], boxes, case['C'], case['T'])
        floor = rescore_spec.planted_floor(tracks, floor)
        rec = dict(case, maxpool=[], sampling=[])
        for c in range(case['C']):
            class_idx = c + 1
            vid, trp = protos(case, boxes, scores, tracks, c)
            # (a) spatial max-pool + completion, then the temporal max-pools
            f2d = {f + 1: (boxes[f].astype(np.float64), scores[f]) for f in range(case['F'])}
            sp = T.raw_dets_spatial_max_pooling(vid, copy.deepcopy(trp), f2d, class_idx, case['overlap_thres'])
            p3 = T.score_proto_temporal_maxpool(copy.deepcopy(sp), 3)
            p5 = T.score_proto_temporal_maxpool(copy.deepcopy(sp), 5)
            rec['maxpool'].append(record(sp['tubelets'], (('pool3', p3['tubelets']), ('pool5', p5['tubelets']))))
            # (b) rcnn_sampling_dets_scoring after the CNN: the scorers return the planted score of the box they are asked about
            planted = {}
            for t in range(case['T']):
                for f in range(case['F']):
                    if not np.isnan(tracks[c, t, f, 0]):
                        planted[(f + 1,) + tuple(float(x) for x in tracks[c, t, f, :4])] = float(floor[c, t, f])
            T.imread = lambda path: int(os.path.splitext(os.path.basename(path))[0]) + 1
            T.svm_from_rcnn_model = lambda model: None
            T.googlenet_features = lambda img, bxs, net, layer: np.asarray(
                [[float(img)] + [float(x) for x in b] for b in bxs], np.float64)
            T.svm_scores = lambda feats, model: np.tile(np.asarray(
                [planted.get(tuple(float(x) for x in r), 0.0) for r in feats], np.float64)[:, None], (1, 200))
            det = {'video': vid['video'], 'detections': [
                {'frame': f + 1, 'bbox': [float(x) for x in boxes[f, b]],
                 'scores': [{'class_index': class_idx, 'score': float(scores[f, b, c])}]}
                for f in range(case['F']) for b in range(case['B'])]}
            tub = T.rcnn_sampling_dets_scoring(vid, copy.deepcopy(trp), det, None, class_idx, None, case['overlap_thres'])
            rec['sampling'].append(record(tub))
        out.append(rec)
    path = os.path.join(HERE, 'rescore_golden.json.gz')
    with gzip.GzipFile(path, 'wb', mtime=0) as f:
        f.write(json.dumps({'cases': out}, separators=(',', ':'), sort_keys=True).encode())
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
