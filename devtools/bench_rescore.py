#!/usr/bin/env python3
"""Re-scoring of any tubelet set on the device (ops.rescore_tubelets / ops.rescore_tubelets_batch) at two shapes:
  python devtools/bench_rescore.py [--reps R] [--warmup W] [--boxes B]
 c2     one c2 video: 200 classes x 10 anchor-route tubelets x 300 frames over --boxes proposals per frame (default 10 000);
 vid64  the 64-video VID batch of bench.synth_vid_batch: 30 classes x 10 anchor-route tubelets per video, 300 proposals.
The c2 proposals persist over time (frame f = frame 0 drifting 3 px per frame with +-1 px of jitter), so the anchor route
(ops.top_anchors -> ops.track_from_anchors[_batch]) makes tubelets that run through the video; they have no holes, which
lets the existing path serve as the comparator on the SAME tubelets:
 c2     ops.rescore_tracks (its window-scan path: the tubelets are not the context's last tracking result);
 vid64  a Python loop of ops.rescore_tracks over the videos.
Per leg: HIP-event and wall time per call, median [min .. max] of R calls after W warm-up calls; det / pooled / tboxes of the
two paths are checked bit-identical; the legs are timed alternately, twice, so the spread of each shows.  A floor leg (f64
floor, no completion) is timed on the new path alone.  Prints one JSON line."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import bench
from bench_tcn import device_times
from vdetlib_amd import ops

T = 10


def coherent_c2(dev, F, B, C):
    g = torch.Generator(device=dev).manual_seed(2026)
    base, _ = bench.synth_video_cuda(torch, 7, 1, B, 1, dev)
    boxes = base + 3.0 * torch.arange(F, device=dev, dtype=torch.float32)[:, None, None] + \
        torch.randint(-1, 2, (F, B, 4), generator=g, device=dev).float()
    boxes[..., 2:] = torch.maximum(boxes[..., 2:], boxes[..., :2] + 4)
    return boxes.contiguous(), torch.rand(F, B, C, generator=g, device=dev)


def same(a, b):
    return bool(torch.equal(torch.nan_to_num(a, nan=-7.0), torch.nan_to_num(b, nan=-7.0)))


def census(bo):
    live = torch.cat([(t[..., 0] == t[..., 0]).reshape(-1) for t in bo['tracks']])
    return {"tubelet_boxes": int(live.sum()), "slots": int(live.numel())}


def leg(bo, boxes, scores, a):
    off = [int(x) for x in bo['frame_off']]
    V = len(off) - 1
    new = lambda s: ops.rescore_tubelets_batch(bo, boxes, scores, sync=s)
    flo = torch.rand(sum(t[..., 0].numel() for t in bo['tracks']), device=boxes.device, dtype=torch.float64)
    new_floor = lambda s: ops.rescore_tubelets_batch(bo, boxes, scores, floor=flo, sync=s)

    def old(s):
        return [ops.rescore_tracks(bo['tracks'][v], bo['ntracks'][v], boxes[off[v]:off[v + 1]], scores[off[v]:off[v + 1]], sync=s)
                for v in range(V)]
    out, ref = new(True), old(True)
    equal = all(same(out[k][v], ref[v][i]) for v in range(V) for i, k in enumerate(('det', 'pooled', 'tboxes')))
    res = dict(census(bo), videos=V, frames=off[-1], equal_to_rescore_tracks=equal,
               hits=int(sum(int((x >= 0).sum()) for x in out['src'])))
    # the legs alternate, twice over: the second round shows the run-to-run spread of each
    for rnd in ("round1", "round2"):
        for name, fn in (("rescore_tubelets", new), ("rescore_tracks_loop" if V > 1 else "rescore_tracks", old),
                         ("rescore_tubelets_floor", new_floor)):
            ev, wall = device_times(fn, a.reps, a.warmup)
            res.setdefault(name, {})[rnd] = {"event_ms": ev, "wall_ms": wall}
    return res


def main():
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--boxes", type=int, default=10000)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup}
    boxes, scores = coherent_c2(dev, 300, a.boxes, 200)
    fr, ab, sc, _ = ops.top_anchors(boxes, scores, T)
    tr, an, nt = ops.track_from_anchors(boxes, fr, ab, sc)
    bo = dict(tracks=[tr], anchors=an[None], ntracks=nt[None], frame_off=np.array([0, 300], np.int64))
    res["c2"] = dict(leg(bo, boxes, scores, a), boxes_per_frame=a.boxes)
    print("c2 timed", file=sys.stderr, flush=True)
    del boxes, scores, bo, tr
    boxes, scores, off = bench.synth_vid_batch(torch, dev, 64)
    fr, ab, sc, _ = ops.top_anchors(boxes, scores, T, frame_off=off)
    bo = ops.track_from_anchors_batch(boxes, off, fr, ab, sc)
    res["vid64"] = leg(bo, boxes, scores, a)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
