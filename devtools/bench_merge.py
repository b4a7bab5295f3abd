#!/usr/bin/env python3
"""The device merge of two scored tubelet sets (ops.merge_tracks / ops.merge_tracks_batch), both schemes, at two shapes:
  python devtools/bench_merge.py [--reps R] [--warmup W] [--host-classes N]
 c2     one c2 video's tubelets: 200 classes, 10 + 10 tubelets, 300 frames, two series + tboxes;
 vid64  the 64-video VID batch of bench.synth_vid_batch's frame counts: 30 classes, 10 + 10 tubelets per video.
Per shape and scheme: (a) the kernel -- HIP-event time and wall time per call, median [min .. max] of R calls after W warm-up
calls, and the bytes it has to move (every input element it must read, every output element) over the event time;
(b) the composition of torch ops a caller could write on the same GPU (torch.cat per field / torch.where on det_b > det_a;
per video and concatenated again for the ragged batch layout), checked equal to the kernel: the inputs are REGULAR (every
slot live, a box on every frame), which is where that composition can express the result -- it has no ordinal pairing, no
validation and no counts; (c) c2 only: the dict route, ops.tracks_to_proto + the det_score of every box for the first N
classes -> protocol.merge_score_protos, timed once and scaled to all classes.  Prints one JSON line."""
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
from vdetlib_amd.utils import protocol


def regular_batch(gen, dev, off, C, T):
    """a dict in video_batch's layout: every slot live, a box on every frame, anchors on frame 1"""
    V, Ft = len(off) - 1, int(off[-1])
    n = C * T * Ft
    flat = dict(tracks=(torch.rand(n * 5, generator=gen, device=dev) * 600).round(), det=torch.randn(n, generator=gen, device=dev, dtype=torch.float64),
                pooled=torch.randn(n, generator=gen, device=dev, dtype=torch.float64), tboxes=(torch.rand(n * 4, generator=gen, device=dev) * 600).round())
    per = dict(tracks=5, det=1, pooled=1, tboxes=4)
    out = {k: [x[C * T * per[k] * int(off[v]): C * T * per[k] * int(off[v + 1])].view(*((C, T, int(off[v + 1] - off[v])) + ((per[k],) if per[k] > 1 else ())))
               for v in range(V)] for k, x in flat.items()}
    anchors = torch.zeros((V, C, T, 3), device=dev)
    anchors[..., 0] = 1
    out.update(anchors=anchors, ntracks=torch.full((V, C), T, dtype=torch.int32, device=dev), frame_off=np.asarray(off, np.int64))
    return out


FIELDS = ('tracks', 'det', 'pooled', 'tboxes')


def torch_route(ba, bb, scheme):
    V = len(ba['tracks'])
    if scheme == 'combine':
        out = {k: torch.cat([torch.cat((ba[k][v], bb[k][v]), 1).reshape(-1) for v in range(V)]) for k in FIELDS}
        out['anchors'] = torch.cat((ba['anchors'], bb['anchors']), 2)
        out['ntracks'] = ba['ntracks'] + bb['ntracks']
        return out
    fa = {k: ops._batch_flat(ba[k], 1) for k in FIELDS}
    fb = {k: ops._batch_flat(bb[k], 1) for k in FIELDS}
    take = fb['det'] > fa['det']
    out = {k: torch.where(take, fb[k], fa[k]) for k in ('det', 'pooled')}
    out['tracks'] = torch.where(take[:, None], fb['tracks'].view(-1, 5), fa['tracks'].view(-1, 5)).reshape(-1)
    out['tboxes'] = torch.where(take[:, None], fb['tboxes'].view(-1, 4), fa['tboxes'].view(-1, 4)).reshape(-1)
    out['from_b'] = take.to(torch.uint8)
    return out


def same(mine, theirs, scheme):
    ok = all(torch.equal(ops._batch_flat(mine[k], 1), theirs[k]) for k in FIELDS)
    if scheme == 'combine':
        return ok and torch.equal(mine['anchors'], theirs['anchors']) and torch.equal(mine['ntracks'], theirs['ntracks'])
    return ok and torch.equal(ops._batch_flat(mine['from_b'], 1), theirs['from_b'])


def leg(ba, bb, a):
    C, T = ba['tracks'][0].shape[:2]
    n = C * T * int(ba['frame_off'][-1])
    res = {}
    for scheme in ('combine', 'max'):
        fn = lambda s: ops.merge_tracks_batch(ba, bb, scheme, sync=s)
        tf = lambda s: (torch_route(ba, bb, scheme), torch.cuda.synchronize() if s else None)
        ok = same(fn(True), torch_route(ba, bb, scheme), scheme)
        ev, wall = device_times(fn, a.reps, a.warmup)
        tev, twall = device_times(tf, a.reps, a.warmup)
        # rows 20 B + tboxes 16 B + two series 16 B per box: combine reads both sets once and writes both; max reads a whole,
        # b's rows for the ballots and b's det_score (what is taken from b comes on top), writes a's shape + from_b
        moved = n * 52 * 4 if scheme == 'combine' else n * (52 + 20 + 8 + 52 + 1)
        res[scheme] = {"event_ms": ev, "wall_ms": wall, "torch_event_ms": tev, "torch_wall_ms": twall, "equal_to_torch": bool(ok),
                       "gb_moved": round(moved / 1e9, 4), "tb_s": round(moved / (ev["median"] * 1e-3) / 1e12, 3),
                       "torch_over_kernel": round(tev["median"] / ev["median"], 2)}
    return res


def dict_route(ba, bb, ncls, C):
    """seconds of tracks_to_proto (+ det_score) and of merge_score_protos over the first ncls classes, scaled to C"""
    def protos(bo):
        tr, an, nt = bo['tracks'][0][:ncls], bo['anchors'][0][:ncls], bo['ntracks'][0][:ncls].cpu().numpy()
        det = bo['det'][0][:ncls].cpu().numpy()
        out = []
        for c in range(ncls):
            tp = ops.tracks_to_proto('c2', tr[c], an[c], int(nt[c]))
            tubs = [{'class_index': c + 1, 'class': str(c + 1), 'gt': 0,
                     'boxes': [dict(b, det_score=float(det[c, t, b['frame'] - 1]), track_score=b['score']) for b in trk]}
                    for t, trk in enumerate(tp['tracks'])]
            out.append({'video': 'c2', 'method': 'm', 'tubelets': tubs})
        return out
    t0 = time.perf_counter()
    pa, pb = protos(ba), protos(bb)
    t1 = time.perf_counter()
    res = {"classes_timed": ncls, "to_protos_s": round((t1 - t0) * C / ncls, 3)}
    for scheme in ('combine', 'max'):
        import copy
        xa, xb = copy.deepcopy(pa), copy.deepcopy(pb)
        t0 = time.perf_counter()
        for x, y in zip(xa, xb):
            protocol.merge_score_protos(x, y, scheme)
        res["merge_%s_s" % scheme] = round((time.perf_counter() - t0) * C / ncls, 3)
    return res


def main():
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-classes", type=int, default=4)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    gen = torch.Generator(device=dev).manual_seed(2024)
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup}
    ba, bb = regular_batch(gen, dev, [0, 300], 200, 10), regular_batch(gen, dev, [0, 300], 200, 10)
    res["c2"] = leg(ba, bb, a)
    res["c2"]["dict_route"] = dict_route(ba, bb, max(1, min(a.host_classes, 200)), 200)
    del ba, bb
    _, _, off = bench.synth_vid_batch(torch, dev, 64)
    ba, bb = regular_batch(gen, dev, off, 30, 10), regular_batch(gen, dev, off, 30, 10)
    res["vid64"] = dict(leg(ba, bb, a), videos=len(off) - 1, frames=int(off[-1]))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
