#!/usr/bin/env python3
"""Device interpolation of strided tubelets (ops.interpolate_tracks[_batch]) on the tubelets of one c2 video (300 frames x
10 000 boxes x 200 classes, 10 tracks per class; tracked on every 3rd frame, and tracked densely with a third of the
rows punched out) and of the 64-video VID-shaped batch (every 3rd frame):
  python devtools/bench_interp.py [--reps R] [--warmup W] [--host-classes N]
 (a) the route without it: ops.tracks_to_proto-style protos with the frame map applied + score_proto_interpolation,
     timed once; --host-classes N limits it to the first N classes of every video (0 = all) and scales the time;
 (b) the new call: HIP-event time and wall time per call, median [min .. max] of R calls after W warm-up calls;
 (c) ops.rescore_tracks (the re-scoring share of ops.video_batch for the batch) on the same tubelets, for scale;
 and the bytes (b) must move, C*T*(Fs*in + F*out), over its event time as a fraction of 8 TB/s.  Prints one JSON line."""
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
from vdetlib_amd.utils.protocol import tubelets_proto_from_tracks_proto
from vdetlib_amd.vdet import tubelet_cls as TC

HBM_BYTES_PER_S = 8e12


def call_bytes(C, T, Fs, F, nser, with_boxes):
    row_in = 5 * 4 + (4 * 4 if with_boxes else 0) + nser * 8
    row_out = 5 * 4 + 4 * 8 + 4 * 4 + nser * 8 + 8
    return C * T * (Fs * row_in + F * row_out)


def proto_route(name, tr, an, nt, det, ob, frames, F, n_cls):
    """seconds of (proto building, score_proto_interpolation) for the first n_cls classes, and the tubelets done"""
    trh, anh, nth, deth, obh = (x.cpu().numpy() for x in (tr, an, nt, det, ob))
    vid = {'video': name, 'frames': [{'frame': i + 1, 'path': ''} for i in range(F)]}
    t0 = time.perf_counter()
    protos = []
    for c in range(n_cls):
        tp = ops.tracks_to_proto(name, trh[c], anh[c], int(nth[c]))
        tubs = tubelets_proto_from_tracks_proto(tp['tracks'], c % 30 + 1)
        for t, tub in enumerate(tubs):
            arow = int(anh[c, t, 0]) - 1
            for box in tub['boxes']:
                row = box['frame'] - 1
                box.update(det_score=float(deth[c, t, row]), bbox=[float(v) for v in obh[c, t, row]], frame=int(frames[row]),
                           anchor=int(frames[row] - frames[arow]))
        protos.append({'video': name, 'method': 'bench', 'tubelets': tubs})
    t_build = time.perf_counter() - t0
    t0 = time.perf_counter()
    for p in protos:
        TC.score_proto_interpolation(p, vid)
    return t_build, time.perf_counter() - t0, sum(len(p['tubelets']) for p in protos)


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
    F, B, C, T = 300, 10000, 200, 10
    boxes, scores = bench.synth_video_cuda(torch, 2000, F, B, C, dev)
    for tag, stride in (("c2_stride3", 3), ("c2_stride1_holes", 1)):
        frames = np.arange(1, F + 1, stride)
        sb, ss = boxes[::stride].contiguous(), scores[::stride].contiguous()
        tr, an, nt = ops.track_volume(sb, ss, nms_thres=0.3, thres=0.0, max_tracks=T, link_thres=0.5)
        det, pooled, ob = ops.rescore_tracks(tr, nt, sb, ss, overlap_thres=0.7, window=3)
        ev_c, wall_c = device_times(lambda s: ops.rescore_tracks(tr, nt, sb, ss, overlap_thres=0.7, window=3, sync=s), a.reps, a.warmup)
        if stride == 1:      # punch a third of the rows out of every tubelet (never the anchor row)
            g = torch.Generator(device=dev).manual_seed(5)
            drop = torch.rand(tr.shape[:3], generator=g, device=dev) < 1.0 / 3
            drop[torch.arange(C, device=dev)[:, None], torch.arange(T, device=dev)[None, :], (an[..., 0].long() - 1).clamp(0, F - 1)] = False
            tr = tr.clone()
            tr[drop] = float('nan')
        fn = lambda s: ops.interpolate_tracks(tr, nt, an, [det, pooled], boxes=ob, frames=frames if stride > 1 else None,
                                              num_frames=F, sync=s)
        out = fn(True)
        ev_b, wall_b = device_times(fn, a.reps, a.warmup)
        nb = call_bytes(C, T, len(frames), F, 2, True)
        ncls = a.host_classes or C
        tb, ti, ntub = proto_route('c2', tr, an, nt, det, ob, frames, F, ncls)
        scale = int(nt.sum()) / max(ntub, 1)
        res[tag] = {"tubelets": int(nt.sum()), "rows": len(frames), "dense_boxes": int((~torch.isnan(out['tracks'][..., 0])).sum()),
                    "a_proto_build_s": round(tb * scale, 3), "a_score_proto_interpolation_s": round(ti * scale, 3),
                    "a_tubelets_timed": ntub, "b_event_ms": ev_b, "b_wall_ms": wall_b, "c_rescore_tracks_event_ms": ev_c,
                    "bytes": nb, "b_fraction_of_8TBps": round(nb / (ev_b["median"] * 1e-3) / HBM_BYTES_PER_S, 4),
                    "a_over_b_wall": round((tb + ti) * scale * 1e3 / wall_b["median"], 1)}
    # ---- the 64-video VID-shaped batch, every 3rd frame
    vb, vs, off = bench.synth_vid_batch(torch, dev, 64)
    V = len(off) - 1
    rows = [np.arange(int(off[v]), int(off[v + 1]), 3) for v in range(V)]
    frs = [r - int(off[v]) + 1 for v, r in enumerate(rows)]
    idx = torch.from_numpy(np.concatenate(rows)).to(dev)
    sb, ss = vb[idx].contiguous(), vs[idx].contiguous()
    soff = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    nf = np.diff(off)
    kw = dict(nms_thres=0.3, thres=0.5, max_tracks=4, link_thres=0.5, cap=300, overlap_thres=0.7, window=3)
    bo = ops.video_batch(sb, ss, soff, **kw)
    ev_r, _ = device_times(lambda s: ops.video_batch(sb, ss, soff, sync=s, **kw), a.reps, a.warmup)
    ev_n, _ = device_times(lambda s: ops.video_batch(sb, ss, soff, sync=s, rescore=False, **kw), a.reps, a.warmup)
    allfr = np.concatenate(frs)
    fn = lambda s: ops.interpolate_tracks_batch(bo, allfr, nf, sync=s)
    fn(True)
    ev_b, wall_b = device_times(fn, a.reps, a.warmup)
    Cb, Tb = bo['tracks'][0].shape[:2]
    nb = call_bytes(Cb, Tb, int(soff[-1]), int(off[-1]), 2, True)
    tb = ti = 0.0
    for v in range(V):
        x, y, _ = proto_route('vid%d' % v, bo['tracks'][v], bo['anchors'][v], bo['ntracks'][v], bo['det'][v], bo['tboxes'][v], frs[v],
                              int(nf[v]), Cb)
        tb, ti = tb + x, ti + y
    res["vid64_stride3"] = {"tubelets": int(bo['ntracks'].sum()), "rows": int(soff[-1]), "frames": int(off[-1]),
                            "a_proto_build_s": round(tb, 3), "a_score_proto_interpolation_s": round(ti, 3), "b_event_ms": ev_b,
                            "b_wall_ms": wall_b, "c_rescore_share_event_ms": round(ev_r["median"] - ev_n["median"], 4),
                            "bytes": nb, "b_fraction_of_8TBps": round(nb / (ev_b["median"] * 1e-3) / HBM_BYTES_PER_S, 4),
                            "a_over_b_wall": round((tb + ti) * 1e3 / wall_b["median"], 1)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
