#!/usr/bin/env python3
"""The tubelet TCN three ways, on the tubelets of one c2 video (300 frames x 10 000 boxes x 200 classes, 10 tracks per
class) and of the 64-video VID-shaped batch (built like devtools/bench_eval.py builds them):
  python devtools/bench_tcn.py [--reps R] [--warmup W] [--host-classes N]
 (a) the per-tubelet path: ops.tracks_to_proto + score_conv_cls with TCNNet.forward (one upload, launch, wait and
     download per layer and tubelet), video by video; timed once (it takes seconds), proto building and scoring apart;
     --host-classes N limits it to the first N classes of every video (0 = all) and scales the time to all tubelets;
 (b) score_conv_cls_batched on the same protos (one launch per video);
 (c) ops.tcn_tracks / ops.tcn_tracks_batch on the device tensors: HIP-event time of the two launches and wall time per
     call, median [min .. max] of R calls after W warm-up calls; ops.rescore_tracks / the re-scoring share of
     ops.video_batch on the same tubelets beside it as the scale.
Nets: TCNNet.random at hidden (16, 16), K = 3 and at (64, 64), K = 5, inputs det_scores, track_scores, anchors,
abs_anchors.  Prints one JSON line."""
import contextlib
import io
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import bench
from vdetlib_amd import ops
from vdetlib_amd.utils.protocol import tubelets_proto_from_tracks_proto
from vdetlib_amd.vdet import tubelet_cls as TC
from vdetlib_amd.vdet.tcn import TCNNet

NAMES = ['det_scores', 'track_scores', 'anchors', 'abs_anchors']


def stats(ts):
    ts = np.asarray(ts, dtype=np.float64)
    return {"median": round(float(np.median(ts)), 4), "min": round(float(ts.min()), 4), "max": round(float(ts.max()), 4)}


def device_times(fn, reps, warmup):
    """(HIP-event ms of the enqueued work, wall ms per synchronous call)"""
    for _ in range(warmup):
        fn(True)
    ev_ms, wall_ms = [], []
    for _ in range(reps):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn(False)
        e1.record()
        torch.cuda.synchronize()
        ev_ms.append(e0.elapsed_time(e1))
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(True)
        torch.cuda.synchronize()
        wall_ms.append((time.perf_counter() - t0) * 1e3)
    return stats(ev_ms), stats(wall_ms)


def build_protos(name, tr, an, nt, det, n_cls):
    """score protos (one per class) of the device tubelets -- the dict form the existing path needs"""
    trh, anh, nth, deth = tr.cpu().numpy(), an.cpu().numpy(), nt.cpu().numpy(), det.cpu().numpy()
    protos = []
    for c in range(n_cls):
        tp = ops.tracks_to_proto(name, trh[c], anh[c], int(nth[c]))
        tubs = tubelets_proto_from_tracks_proto(tp['tracks'], c % 30 + 1)     # (the VID class table has 30 names; the net ignores the class)
        for t, tub in enumerate(tubs):
            for box in tub['boxes']:
                box['det_score'] = float(deth[c, t, box['frame'] - 1])
                box['gt_overlap'] = 0
        protos.append({'video': name, 'method': 'bench', 'tubelets': tubs})
    return protos


def host_paths(videos, net, n_cls):
    """videos: list of (name, tr, an, nt, det).  Returns seconds of (proto building, (a) scoring, (b) scoring), the
    number of tubelets scored, and whether (a) and (b) gave the same bits."""
    t0 = time.perf_counter()
    protos = [p for v in videos for p in build_protos(*v, n_cls=min(n_cls, v[1].shape[0]) if n_cls else v[1].shape[0])]
    t_build = time.perf_counter() - t0
    ntub = sum(len(p['tubelets']) for p in protos)
    with contextlib.redirect_stdout(io.StringIO()):
        t0 = time.perf_counter()
        for p in protos:
            TC.score_conv_cls(p, net)
        t_a = time.perf_counter() - t0
        a_scores = [b['conv_score'] for p in protos for tub in p['tubelets'] for b in tub['boxes']]
        t0 = time.perf_counter()
        for p in protos:
            TC.score_conv_cls_batched(p, net)
        t_b = time.perf_counter() - t0
    b_scores = [b['conv_score'] for p in protos for tub in p['tubelets'] for b in tub['boxes']]
    return t_build, t_a, t_b, ntub, a_scores == b_scores


def main():
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-classes", type=int, default=0)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup}
    # ---- one c2 video
    F, B, C = 300, 10000, 200
    boxes, scores = bench.synth_video_cuda(torch, 2000, F, B, C, dev)
    tr, an, nt = ops.track_volume(boxes, scores, nms_thres=0.3, thres=0.0, max_tracks=10, link_thres=0.5)
    det, pooled, ob = ops.rescore_tracks(tr, nt, boxes, scores, overlap_thres=0.7, window=3)
    ev, wall = device_times(lambda s: ops.rescore_tracks(tr, nt, boxes, scores, overlap_thres=0.7, window=3, sync=s), a.reps, a.warmup)
    has = ~torch.isnan(tr[..., 0]) & (torch.arange(tr.shape[1], device=dev)[None, :, None] < nt[:, None, None])
    res["c2"] = {"tubelets": int(nt.sum()), "boxes": int(has.sum()), "rescore_tracks_event_ms": ev, "rescore_tracks_wall_ms": wall}
    # ---- the 64-video VID-shaped batch
    vb, vs, off = bench.synth_vid_batch(torch, dev, 64)
    kw = dict(nms_thres=0.3, thres=0.5, max_tracks=4, link_thres=0.5, cap=300, overlap_thres=0.7, window=3)
    bo = ops.video_batch(vb, vs, off, **kw)
    ev_r, wall_r = device_times(lambda s: ops.video_batch(vb, vs, off, sync=s, **kw), a.reps, a.warmup)
    ev_n, wall_n = device_times(lambda s: ops.video_batch(vb, vs, off, sync=s, rescore=False, **kw), a.reps, a.warmup)
    res["vid64"] = {"tubelets": int(bo['ntracks'].sum()), "frames": int(off[-1]),
                    "video_batch_event_ms": ev_r, "video_batch_no_rescore_event_ms": ev_n,
                    "rescore_share_event_ms": round(ev_r["median"] - ev_n["median"], 4)}
    vids = [('vid%d' % v, bo['tracks'][v], bo['anchors'][v], bo['ntracks'][v], bo['det'][v]) for v in range(64)]
    for tag, hidden, k in (("h16_k3", (16, 16), 3), ("h64_k5", (64, 64), 5)):
        net = TCNNet.random([(n, 1) for n in NAMES], hidden=hidden, kernel=k, seed=1)
        # (c) device
        ev, wall = device_times(lambda s: ops.tcn_tracks(net, tr, nt, an, det, sync=s), a.reps, a.warmup)
        r = {"c_event_ms": ev, "c_wall_ms": wall}
        # (a), (b) dict API
        tb, ta, tbb, ntub, same = host_paths([('c2', tr, an, nt, det)], net, a.host_classes)
        scale = res["c2"]["tubelets"] / max(ntub, 1)
        r.update(a_tubelets_timed=ntub, a_proto_build_s=round(tb * scale, 3), a_score_conv_cls_s=round(ta * scale, 3),
                 b_score_conv_cls_batched_s=round(tbb * scale, 3), a_equals_b=same,
                 a_over_c_wall=round((tb + ta) * scale * 1e3 / wall["median"], 1),
                 a_scoring_over_b=round(ta / max(tbb, 1e-9), 2),
                 b_over_c_wall=round((tb + tbb) * scale * 1e3 / wall["median"], 1))
        res["c2"][tag] = r
        ev, wall = device_times(lambda s: ops.tcn_tracks_batch(net, bo, sync=s), a.reps, a.warmup)
        r = {"c_event_ms": ev, "c_wall_ms": wall}
        tb, ta, tbb, ntub, same = host_paths(vids, net, 0)
        r.update(a_tubelets_timed=ntub, a_proto_build_s=round(tb, 3), a_score_conv_cls_s=round(ta, 3),
                 b_score_conv_cls_batched_s=round(tbb, 3), a_equals_b=same,
                 a_over_c_wall=round((tb + ta) * 1e3 / wall["median"], 1), a_scoring_over_b=round(ta / max(tbb, 1e-9), 2),
                 b_over_c_wall=round((tb + tbb) * 1e3 / wall["median"], 1))
        res["vid64"][tag] = r
    print(json.dumps(res))


if __name__ == "__main__":
    main()
