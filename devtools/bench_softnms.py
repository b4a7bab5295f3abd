#!/usr/bin/env python3
"""Soft-NMS of the per-frame detection lists (ops.soft_nms_tracks_batch) on the lists of devtools/bench_tracknms.py:
  python devtools/bench_softnms.py [--reps R] [--warmup W] [--boxes B] [--host-lists N]
 c2     one c2 video: 200 classes, 300 frames, 10 + 10 tubelets and the still-image top-100 -- 120 candidates per list;
 vid64  the 64-video VID batch of bench.synth_vid_batch: 30 classes, 10 + 10 tubelets per video, top-100 of 300 proposals.
Legs, per shape: 'linear' (thresh 0.3) and 'gauss' (sigma 0.5), each with min_score 0.001 and -inf, and ops.nms_tracks_batch
(thresh 0.5: bench_tracknms.py's call) on the identical inputs -- HIP-event and wall time per call, median [min .. max] of R
calls after W warm-up calls.  The legs are run in that order TWICE; both passes are printed.  "rounds" is the mean number of
rows a list emits (the kernel runs one round per emitted row), beside nms_tracks' kept rows per list.
The numpy rule (tests/softnms_spec.py) is timed on the first N lists of the c2 video and scaled to all of them: EXTRAPOLATED.
Prints one JSON line."""
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import bench
from bench_tcn import device_times
from bench_tracknms import T1, TOP, make_inputs
from vdetlib_amd import ops

LEGS = (("linear", dict(method='linear', thresh=0.3, min_score=0.001)), ("linear_nofloor", dict(method='linear', thresh=0.3, min_score=-math.inf)),
        ("gauss", dict(method='gauss', sigma=0.5, min_score=0.001)), ("gauss_nofloor", dict(method='gauss', sigma=0.5, min_score=-math.inf)))


def legs(still, bo, a):
    fns = {name: (lambda s, kw=kw: ops.soft_nms_tracks_batch(bo, 'pooled', still=still, use_tboxes=False, sync=s, **kw)) for name, kw in LEGS}
    fns["nms_tracks"] = lambda s: ops.nms_tracks_batch(bo, 'pooled', still=still, thresh=0.5, use_tboxes=False, sync=s)
    res = {name: {"rounds_per_list_mean": round(float(fn(True)['cnt'].float().mean()), 2), "event_ms": [], "wall_ms": []}
           for name, fn in fns.items()}
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


def numpy_rule(still, bo, nlists):
    """seconds the numpy rule takes on the first nlists lists of the video (class 0 .. of frame 0 ..), scaled to all: EXTRAPOLATED"""
    import softnms_spec as S
    from test_nms_tracks_cpu import list_rows
    st = tuple(x.cpu().numpy() for x in still)
    tracks, ntracks, score = bo['tracks'][0].cpu().numpy(), bo['ntracks'][0].cpu().numpy(), bo['pooled'][0].cpu().numpy()
    C, _, F = tracks.shape[:3]
    out = {"lists_timed": nlists, "EXTRAPOLATED": True}
    for name, kw in LEGS:
        t = 0.0
        for i in range(nlists):
            dets, _, _ = list_rows(i % C, i // C, tracks, ntracks, score, None, st, TOP)
            t0 = time.perf_counter()
            S.soft_nms(dets, kw['method'], kw.get('thresh', 0.3), kw.get('sigma', 0.5), kw['min_score'])
            t += time.perf_counter() - t0
        out[name + "_s"] = round(t * C * F / nlists, 2)
    return out


def main():
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--boxes", type=int, default=2000)
    ap.add_argument("--host-lists", type=int, default=8)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    gen = torch.Generator(device=dev).manual_seed(2025)
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup}
    boxes, scores = bench.synth_video_cuda(torch, 7, 300, a.boxes, 200, dev)
    still, bo, _ = make_inputs(gen, boxes, scores, [0, 300])
    res["c2"] = dict(legs(still, bo, a), boxes_per_frame=a.boxes)
    print("c2: kernels timed", file=sys.stderr, flush=True)
    res["c2"]["numpy_rule"] = numpy_rule(still, bo, max(1, a.host_lists))
    print("c2: numpy rule timed", file=sys.stderr, flush=True)
    del boxes, scores, still, bo
    boxes, scores, off = bench.synth_vid_batch(torch, dev, 64)
    still, bo, _ = make_inputs(gen, boxes, scores, off)
    res["vid64"] = dict(legs(still, bo, a), videos=len(off) - 1, frames=int(off[-1]))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
