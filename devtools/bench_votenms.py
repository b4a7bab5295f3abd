#!/usr/bin/env python3
"""Box voting on the per-frame detection lists (ops.vote_nms_tracks_batch) on the lists of devtools/bench_tracknms.py:
  python devtools/bench_votenms.py [--reps R] [--warmup W] [--boxes B]
 c2     one c2 video: 200 classes, 300 frames, 10 + 10 tubelets and the still-image top-100 -- 120 candidates per list;
 vid64  the 64-video VID batch of bench.synth_vid_batch: 30 classes, 10 + 10 tubelets per video, top-100 of 300 proposals.
Legs, per shape: weights 'score' and 'uniform' (thresh 0.5, vote_thresh 0.5) and ops.nms_tracks_batch (thresh 0.5:
bench_tracknms.py's call, the comparator) on the identical inputs -- HIP-event and wall time per call, median [min .. max] of R
calls after W warm-up calls.  The legs are run in that order TWICE; both passes are printed.  "kept" is the mean number of rows
a list keeps, "voters" the mean number of voters of a kept row (itself included).  No ratio is a pass condition.
Prints one JSON line."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch

import bench
from bench_tcn import device_times
from bench_tracknms import T1, TOP, make_inputs
from vdetlib_amd import ops

LEGS = (("score", dict(weights='score')), ("uniform", dict(weights='uniform')))


def legs(still, bo, a):
    fns = {name: (lambda s, kw=kw: ops.vote_nms_tracks_batch(bo, 'pooled', still=still, thresh=0.5, vote_thresh=0.5, use_tboxes=False,
                                                             sync=s, **kw)) for name, kw in LEGS}
    fns["nms_tracks"] = lambda s: ops.nms_tracks_batch(bo, 'pooled', still=still, thresh=0.5, use_tboxes=False, sync=s)
    res = {}
    for name, fn in fns.items():
        out = fn(True)
        res[name] = {"kept_per_list_mean": round(float(out['cnt'].float().mean()), 2), "event_ms": [], "wall_ms": []}
        if 'votes' in out:
            votes = torch.cat([x.reshape(-1) for x in out['votes']])
            res[name]["voters_per_kept_row_mean"] = round(float(votes[votes > 0].float().mean()), 2)
    torch.cuda.synchronize()
    for _ in range(2):
        for name, fn in fns.items():
            ev, wall = device_times(fn, a.reps, a.warmup)
            res[name]["event_ms"].append(ev)
            res[name]["wall_ms"].append(wall)
    hard = min(p["median"] for p in res["nms_tracks"]["event_ms"])
    for name, _ in LEGS:
        res[name]["over_nms_tracks"] = round(min(p["median"] for p in res[name]["event_ms"]) / hard, 2)
    res["lists"] = int(bo['ntracks'].shape[1]) * int(bo['frame_off'][-1])
    res["candidates_per_list"] = TOP + 2 * T1
    return res


def main():
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--boxes", type=int, default=2000)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    gen = torch.Generator(device=dev).manual_seed(2025)
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup}
    boxes, scores = bench.synth_video_cuda(torch, 7, 300, a.boxes, 200, dev)
    still, bo, _ = make_inputs(gen, boxes, scores, [0, 300])
    res["c2"] = dict(legs(still, bo, a), boxes_per_frame=a.boxes)
    print("c2: kernels timed", file=sys.stderr, flush=True)
    del boxes, scores, still, bo
    boxes, scores, off = bench.synth_vid_batch(torch, dev, 64)
    still, bo, _ = make_inputs(gen, boxes, scores, off)
    res["vid64"] = dict(legs(still, bo, a), videos=len(off) - 1, frames=int(off[-1]))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
