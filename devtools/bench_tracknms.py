#!/usr/bin/env python3
"""The per-frame NMS of tubelets with still-image detections (ops.nms_tracks / ops.nms_tracks_batch) at two shapes:
  python devtools/bench_tracknms.py [--reps R] [--warmup W] [--boxes B] [--host-classes N]
 c2     one c2 video: 200 classes, 300 frames, 10 + 10 tubelets (a 'combine' of two routes), the still-image top-100 of
        ops.nms_volume(0.3, topk=100) over --boxes proposals per frame (default 2000), thresh 0.5;
 vid64  the 64-video VID batch of bench.synth_vid_batch: 30 classes, 10 + 10 tubelets per video, top-100 of 300 proposals.
The tubelets are made on the device: tubelet t of a class follows the class's t-th best survivor of every frame (its box and
its score: a re-scored tubelet box IS a detection box); the second ten are the first ten with +-3 px on the boxes.  Every
tubelet score carries noise of 1e-3, so the lists are tie-free and (b) can be compared.
Per shape: the kernel -- HIP-event and wall time per call, median [min .. max] of R calls after W warm-up calls -- against
 (a) c2 only: the dict route, the tubelet boxes and the survivors of the first N classes in one detection proto, then
     video_det.apply_vid_nms per class, timed once and scaled to all classes;
 (b) an array composition on the same GPU: gather and concatenate both sources into [F,n,C,4] / [F,n,C] with torch and run
     ops.det_nms_volume(topk=n) -- possible because n = 120 <= 128; absent rows get a score below its score threshold.  The
     kept scores of every list are checked equal, as sets, to the kernel's.
Prints one JSON line."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import bench
from bench_tcn import device_times
from vdetlib_amd import ops
from vdetlib_amd.vdet import video_det

TOP, T1 = 100, 10


def make_inputs(gen, boxes, scores, off):
    """(still = (boxes, scores, keep_idx, keep_cnt), a dict in video_batch's layout with 2 * T1 slots)"""
    dev = boxes.device
    Ft, B, C = scores.shape
    ki, kc = ops.nms_volume(boxes, scores, 0.3, topk=TOP, cap=TOP)
    V, T = len(off) - 1, 2 * T1
    idx = ki[:, :, :T1].clamp(min=0).long()                                      # [Ft,C,T1]
    live = torch.arange(T1, device=dev)[None, None, :] < kc[:, :, None]
    bx = boxes[torch.arange(Ft, device=dev)[:, None, None], idx]                # [Ft,C,T1,4]
    sc = scores.permute(0, 2, 1).gather(2, idx).double()                        # [Ft,C,T1]
    bx = torch.cat((bx, bx + torch.randint(-3, 4, bx.shape, generator=gen, device=dev)), 2)
    sc = torch.cat((sc, sc), 2) + 1e-3 * torch.randn((Ft, C, T), generator=gen, device=dev, dtype=torch.float64)
    live = torch.cat((live, live), 2)
    nan = float('nan')
    bx = torch.where(live[..., None], bx, torch.full_like(bx, nan))
    sc = torch.where(live, sc, torch.full_like(sc, nan))
    rows = torch.cat((bx, sc[..., None].float()), 3)                             # [Ft,C,T,5]
    tr = torch.empty(C * T * Ft * 5, device=dev)
    ps = torch.empty(C * T * Ft, device=dev, dtype=torch.float64)
    tv, pv = [], []
    for v in range(V):
        f0, f1 = int(off[v]), int(off[v + 1])
        tv.append(tr[C * T * 5 * f0: C * T * 5 * f1].view(C, T, f1 - f0, 5))
        pv.append(ps[C * T * f0: C * T * f1].view(C, T, f1 - f0))
        tv[v].copy_(rows[f0:f1].permute(1, 2, 0, 3))
        pv[v].copy_(sc[f0:f1].permute(1, 2, 0))
    bo = dict(tracks=tv, pooled=pv, ntracks=torch.full((V, C), T, dtype=torch.int32, device=dev), frame_off=np.asarray(off, np.int64))
    return (boxes, scores, ki, kc), bo, (bx, sc)


def composition(still, tub):
    """(b): both sources as one [F,n,C] volume through ops.det_nms_volume; absent rows score -1 under a threshold of -0.5"""
    boxes, scores, ki, kc = still
    bx, sc = tub
    Ft, B, C = scores.shape
    dev = boxes.device
    idx = ki.clamp(min=0).long()
    sb = boxes[torch.arange(Ft, device=dev)[:, None, None], idx]                # [Ft,C,TOP,4]
    ss = scores.permute(0, 2, 1).gather(2, idx)
    ss = torch.where(torch.arange(TOP, device=dev)[None, None, :] < kc[:, :, None], ss, torch.full_like(ss, -1.0))
    ab = torch.cat((sb, torch.nan_to_num(bx, nan=0.0)), 2).permute(0, 2, 1, 3).contiguous()             # [Ft,n,C,4]
    asc = torch.cat((ss, torch.nan_to_num(sc.float(), nan=-1.0)), 2).permute(0, 2, 1).contiguous()      # [Ft,n,C]
    n = asc.shape[1]
    return ops.det_nms_volume(ab, asc, score_thresh=-0.5, topk=n, nms_thresh=0.5, first_class=0, sync=False)


def kept_scores_equal(out, comp, off):
    """the kept f32 scores of every (frame, class) list, sorted: the kernel's against the composition's"""
    dets, _, _, keep, keep_cnt = comp
    Ft, C, n = keep.shape
    mine = torch.cat([x[..., 4].permute(2, 0, 1) for x in out['tracks']], 0)                            # [Ft,C,R]
    mine = torch.nan_to_num(mine, nan=float('-inf')).sort(2, descending=True)[0][:, :, :n]
    theirs = dets[..., 4].gather(2, keep.clamp(min=0).long())
    theirs = torch.where(torch.arange(n, device=keep.device)[None, None, :] < keep_cnt[:, :, None], theirs, torch.full_like(theirs, float('-inf')))
    theirs = theirs.sort(2, descending=True)[0]
    return bool(torch.equal(mine, theirs) and torch.equal(out['cnt'].t().contiguous(), keep_cnt))


def dict_route(still, tub, ncls, C):
    """(a): seconds to build the detection proto of the first ncls classes and to run apply_vid_nms on each, scaled to C"""
    boxes, scores, ki, kc = (x.cpu().numpy() for x in still)
    bx, sc = (x.cpu().numpy() for x in tub)
    t0 = time.perf_counter()
    names = [str(c + 1) for c in range(C)]
    proto = bench.kept_dets_to_det_proto('c2', ki[:, :ncls], kc[:, :ncls], boxes, scores, names, TOP)
    Ft, _, T, _ = bx.shape
    for f in range(Ft):
        for c in range(ncls):
            for t in range(T):
                if not np.isnan(sc[f, c, t]):
                    proto['detections'].append({'frame': f + 1, 'bbox': [float(v) for v in bx[f, c, t]], 'hash': '',
                                                'scores': [{'class': names[c], 'class_index': c + 1, 'score': float(sc[f, c, t])}]})
    t1 = time.perf_counter()
    kept = sum(len(video_det.apply_vid_nms(proto, c + 1)['detections']) for c in range(ncls))
    t2 = time.perf_counter()
    return {"classes_timed": ncls, "detections": len(proto['detections']), "kept": kept, "to_proto_s": round((t1 - t0) * C / ncls, 3),
            "apply_vid_nms_s": round((t2 - t1) * C / ncls, 3)}


def leg(still, bo, tub, a):
    fn = lambda s: ops.nms_tracks_batch(bo, 'pooled', still=still, thresh=0.5, use_tboxes=False, sync=s)
    comp = lambda s: (composition(still, tub), torch.cuda.synchronize() if s else None)
    out = fn(True)
    ok = kept_scores_equal(out, composition(still, tub), bo['frame_off'])
    torch.cuda.synchronize()
    ev, wall = device_times(fn, a.reps, a.warmup)
    cev, cwall = device_times(comp, a.reps, a.warmup)
    cnt = out['cnt']
    return {"event_ms": ev, "wall_ms": wall, "composition_event_ms": cev, "composition_wall_ms": cwall, "kept_scores_equal": ok,
            "lists": int(cnt.numel()), "candidates_per_list": TOP + 2 * T1, "kept_per_list_mean": round(float(cnt.float().mean()), 2),
            "composition_over_kernel": round(cev["median"] / ev["median"], 2)}


def main():
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--boxes", type=int, default=2000)
    ap.add_argument("--host-classes", type=int, default=2)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    gen = torch.Generator(device=dev).manual_seed(2025)
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup}
    boxes, scores = bench.synth_video_cuda(torch, 7, 300, a.boxes, 200, dev)
    still, bo, tub = make_inputs(gen, boxes, scores, [0, 300])
    res["c2"] = dict(leg(still, bo, tub, a), boxes_per_frame=a.boxes)
    print("c2: kernel and composition timed", file=sys.stderr, flush=True)
    res["c2"]["dict_route"] = dict_route(still, tub, max(1, min(a.host_classes, 200)), 200)
    print("c2: dict route timed", file=sys.stderr, flush=True)
    del boxes, scores, still, bo, tub
    boxes, scores, off = bench.synth_vid_batch(torch, dev, 64)
    still, bo, tub = make_inputs(gen, boxes, scores, off)
    res["vid64"] = dict(leg(still, bo, tub, a), videos=len(off) - 1, frames=int(off[-1]))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
