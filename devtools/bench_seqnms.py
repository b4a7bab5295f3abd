#!/usr/bin/env python3
"""Seq-NMS on the device (ops.seq_nms_batch) on the per-frame detections of bench_tracknms.py's shapes:
  python devtools/bench_seqnms.py [--reps R] [--warmup W] [--boxes B] [--cap R] [--host-classes N]
 c2     one c2 video: 200 classes x 300 frames, ops.nms_tracks_batch of the c2 keep lists and 10 + 10 tubelets cut to --cap
        rows per list (default 128);
 vid64  the 64-video VID batch of bench.synth_vid_batch (30 classes), the same stage, the same cap.
Legs, per shape: max_seqs 8 / 32 / 128 with rescore 'avg', and 32 with 'max'.  HIP-event ms, median [min .. max] of R calls after
W warm-up calls; the legs alternate and the whole turn runs twice, so the spread of each shows.  The split into the link launch
and the rounds is the median of the context's own stage timers ("track_link", "track_loop") over R further calls.
Comparator, c2 only: the numpy rule (tests/seqnms_spec.py) on the first N classes (default 2) at max_seqs 32, its result checked
equal to the device's, timed once and EXTRAPOLATED to all classes.  Prints one JSON line."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "devtools"))
import numpy as np
import torch

LEGS = (("max_seqs_8_avg", 8, 'avg'), ("max_seqs_32_avg", 32, 'avg'), ("max_seqs_128_avg", 128, 'avg'), ("max_seqs_32_max", 32, 'max'))


def measure(dets, a, ops, ctx):
    from bench_tcn import device_times, stats
    r = {}
    fns = {}
    for name, S, mode in LEGS:
        fns[name] = lambda s, S=S, mode=mode: ops.seq_nms_batch(dets, score='score', max_seqs=S, rescore=mode, sync=s)
        out = fns[name](True)
        r[name] = {"sequences_per_class_mean": round(float(out['nseq'].float().mean()), 2),
                   "mean_length": round(float(out['seq_len'].sum()) / max(int(out['nseq'].sum()), 1), 2),
                   "exhausted_classes": int(out['exhausted'].sum()), "predecessor_table": {1: "lds", 2: "global"}[ctx.query(14)]}
    for rnd in ("round1", "round2"):
        for name, _, _ in LEGS:
            r[name][rnd] = dict(zip(("event_ms", "wall_ms"), device_times(fns[name], a.reps, a.warmup)))
    ctx.set_timing(1)
    try:
        for name, _, _ in LEGS:
            link, loop = [], []
            for _ in range(a.reps):
                fns[name](True)
                t = ctx.last_timing()
                link.append(t['track_link'][0])
                loop.append(t['track_loop'][0])
            r[name]["link_launch_ms"], r[name]["rounds_ms"] = stats(link), stats(loop)
    finally:
        ctx.set_timing(0)
    return r


def host_rule(dets, ncls, S, ops):
    """the numpy rule on the first ncls classes of the (one-video) input, checked against the device, scaled to all classes"""
    import seqnms_spec as spec
    t, s, nt = (dets[k][0][:ncls].cpu().numpy() if isinstance(dets[k], list) else dets[k][0, :ncls].cpu().numpy()
                for k in ('tracks', 'score', 'ntracks'))
    t0 = time.perf_counter()
    want = spec.seq_nms_classes(t, nt, s, max_seqs=S)
    dt = time.perf_counter() - t0
    got = ops.seq_nms(dets['tracks'][0], dets['ntracks'][0], dets['score'][0], max_seqs=S)
    same = all(np.array_equal(got[k][:ncls].cpu().numpy(), want[k], equal_nan=k in ('tracks', 'score', 'seq_sum')) for k in spec.KEYS)
    C = dets['ntracks'].shape[1]
    return {"classes_timed": ncls, "equal_to_the_device": bool(same), "seconds_timed": round(dt, 3),
            "EXTRAPOLATED_seconds_all_classes": round(dt * C / ncls, 2)}


def main():
    import argparse
    import bench
    from bench_tracknms import make_inputs
    from vdetlib_amd import _lib, ops
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--boxes", type=int, default=2000)
    ap.add_argument("--cap", type=int, default=128)
    ap.add_argument("--host-classes", type=int, default=2)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    ctx = _lib.get_context(0)
    gen = torch.Generator(device=dev).manual_seed(2025)
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup, "cap": a.cap}
    for name in ("c2", "vid64"):
        if name == "c2":
            boxes, scores = bench.synth_video_cuda(torch, 7, 300, a.boxes, 200, dev)
            off = [0, 300]
        else:
            boxes, scores, off = bench.synth_vid_batch(torch, dev, 64)
        still, bo, _ = make_inputs(gen, boxes, scores, off)
        # (cap below what a list can keep: rows beyond it are cut and reported at the wait; the cut is the point here)
        dets = ops.nms_tracks_batch(bo, 'pooled', still=still, thresh=0.5, use_tboxes=False, cap=a.cap, sync=False)
        try:
            ctx.sync()
        except ValueError:
            pass
        C, R = dets['tracks'][0].shape[:2]
        res[name] = dict(measure(dets, a, ops, ctx), classes=C, rows=R, videos=len(off) - 1, frames=int(off[-1]),
                         nodes_per_list_mean=round(float(dets['cnt'].clamp(max=R).float().mean()), 2))
        if name == "c2":
            res[name]["numpy_rule"] = host_rule(dets, max(1, min(a.host_classes, C)), 32, ops)
        print(name + ": timed", file=sys.stderr, flush=True)
        del boxes, scores, still, bo, dets
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
