#!/usr/bin/env python3
"""Device evaluator (ops.DetEvaluator) timings against the host evaluator (vdetlib_amd/eval.py):
  python devtools/bench_eval.py [--host-frames N] [--reps R]
- c2 per-frame output: nms_volume_topk (top-100) of 300 frames x 10 000 boxes x 200 classes (~6 M detections),
- the re-scored tubelets of that c2 video (track_volume + rescore_tracks, 10 tracks per class),
- a 64-video VID-shape batch (video_batch, one match launch),
- the host evaluator on the first N frames of the c2 per-frame output (evaluation only, list already built), and the
  device evaluator on the same detections; the host's per-detection time extrapolated to the whole c2 output.
Device times are wall clock around adds + compute (torch.cuda.synchronize), ground-truth upload excluded; median of R.
Prints one JSON line."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import bench
from vdetlib_amd import eval as vev, ops


def planted_annots(name, boxes, frames, n_tracks, n_classes, seed):
    """ground-truth tracks that follow proposal boxes of the volume (so that some detections match)"""
    rng = np.random.RandomState(seed)
    bx = boxes.cpu().numpy()
    tracks = []
    for k in range(n_tracks):
        b, cls = int(rng.randint(0, 200)), int(rng.randint(1, n_classes + 1))
        tracks.append({'id': str(k), 'track': [{'frame': f + 1, 'bbox': [float(v) for v in bx[f, b] + rng.randint(-4, 5, 4)],
                                               'class_index': cls} for f in range(frames)]})
    return {'video': name, 'annotations': tracks}


def timed(fn, reps):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), out


def main():
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--host-frames", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    res = {"device": torch.cuda.get_device_name(0)}
    F, B, C = 300, 10000, 200
    boxes, scores = bench.synth_video_cuda(torch, 2000, F, B, C, dev)
    ki, kc = ops.nms_volume(boxes, scores, 0.3, topk=100, cap=100, pad=False)
    annot = planted_annots('c2', boxes, F, 8, C, 1)
    table = vev.gt_table_from_annots([annot])
    ndet = int(kc.sum())

    def c2_keep(ev_rule='voc', fr=F):
        ev = ops.DetEvaluator(table, rule=ev_rule)
        def run():
            ev._n = 0
            ev.add_keep_lists('c2', boxes[:fr], scores[:fr], ki[:fr], kc[:fr])
            return ev.compute()
        return run
    for rule in ('voc', 'ilsvrc'):
        ms, (aps, m) = timed(c2_keep(rule), a.reps)
        res["c2_keep_%s_ms" % rule] = round(ms, 3)
    res["c2_keep_detections"] = ndet
    # tubelets of the same video
    tr, an, nt = ops.track_volume(boxes, scores, nms_thres=0.3, thres=0.0, max_tracks=10, link_thres=0.5)
    det, pooled, ob = ops.rescore_tracks(tr, nt, boxes, scores, overlap_thres=0.7, window=3)
    ev = ops.DetEvaluator(table)

    def tubes():
        ev._n = 0
        ev.add_tracks('c2', tr, nt, pooled, ob)
        return ev.compute()
    ms, _ = timed(tubes, a.reps)
    res["c2_tubelets_ms"] = round(ms, 3)
    res["c2_tubelet_detections"] = int(ev._n)
    # 64-video VID-shape batch
    vb, vs, off = bench.synth_vid_batch(torch, dev, 64)
    out = ops.video_batch(vb, vs, off, nms_thres=0.3, thres=0.5, max_tracks=4, link_thres=0.5, cap=300, overlap_thres=0.7,
                          window=3)
    names = ['vid%d' % v for v in range(64)]
    annots = [planted_annots(names[v], vb[off[v]:off[v + 1]], int(off[v + 1] - off[v]), 3, 30, 10 + v) for v in range(64)]
    evb = ops.DetEvaluator(vev.gt_table_from_annots(annots))

    def batch():
        evb._n = 0
        evb.add_batch(names, out)
        return evb.compute()
    ms, _ = timed(batch, a.reps)
    res["vid64_batch_ms"] = round(ms, 3)
    res["vid64_batch_detections"] = int(evb._n)
    # host evaluator vs device on the first host-frames frames of the c2 per-frame output
    fr = a.host_frames
    dets = vev.detections_from_keep_lists('c2', boxes[:fr].cpu().numpy(), scores[:fr].cpu().numpy(), ki[:fr].cpu().numpy(),
                                          kc[:fr].cpu().numpy())
    gt = vev.ground_truth_from_annots([annot])
    t0 = time.perf_counter()
    aps_h, map_h = vev.evaluate(dets, gt)
    host_s = time.perf_counter() - t0
    ms, (aps_d, map_d) = timed(c2_keep('voc', fr), a.reps)
    res.update(host_subset_frames=fr, host_subset_detections=len(dets), host_subset_s=round(host_s, 3),
               device_subset_ms=round(ms, 3), subset_speedup=round(host_s * 1e3 / ms, 1),
               subset_map_abs_diff=abs(map_h - map_d),
               host_us_per_detection=round(host_s * 1e6 / max(len(dets), 1), 3),
               host_c2_extrapolated_s=round(host_s * ndet / max(len(dets), 1), 1),
               c2_speedup_vs_extrapolated_host=round(host_s * ndet / max(len(dets), 1) * 1e3 / res["c2_keep_voc_ms"], 1))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
