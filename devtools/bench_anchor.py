#!/usr/bin/env python3
"""The device anchor route (ops.track_from_anchors + ops.anchor_propagate_tracks) on one c2 video (300 frames x 10 000 boxes
x 200 classes) with 2 000 anchors, 10 per class: the anchors ops.nms_track_volume itself chose, so the rows can be compared:
  python devtools/bench_anchor.py [--reps R] [--warmup W] [--host-classes N]
 (a) the dict route: track_from_det with a python IoU-linking plug-in (the oracle's iou_link_rows_box on numpy arrays) +
     anchor_propagate, on the anchors of the first N classes (default 2), timed once and scaled to all anchors; the
     det_proto holds the anchor frames' detections only (the whole video cannot travel as dicts);
 (b) the new calls: HIP-event time and wall time per call, median [min .. max] of R calls after W warm-up calls;
 (c) nms_track_volume on the same video: vdet_last_timing_ms' track_link / track_loop / track_pick stages, for scale.

 (d) --select: ops.top_anchors (choosing the anchors on the device) on the same video -- video mode T = 10 and T = 100, frame
     mode top_num = 1 -- and on the 64-video VID-shape batch (T = 10, with the batch link and propagate calls behind it),
     each next to what a caller could do before: scores.permute(2,0,1).reshape(C,-1).topk(T) + the box gather on the same
     GPU (no stable tie rule), and protocol.top_detections over the dicts of --host-classes classes, scaled to all classes.
     "volume_tb_s" is the bytes of the score volume divided by the event time (DESIGN section 8's roofline is 8 TB/s).
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
from oracle import oracle
from vdetlib_amd import _lib, ops
from vdetlib_amd.utils.protocol import tracks_proto_from_boxes
from vdetlib_amd.vdet import track as K
from vdetlib_amd.vdet import tubelet_cls as TC


def dict_route(name, boxes_h, scores_h, frames, ab, n_cls, F):
    """seconds of (track_from_det, anchor_propagate) over the anchors of the first n_cls classes, the anchors done, and
    whether the dict route's rows and scores are the device's"""
    vid = {'video': name, 'frames': [{'frame': i + 1, 'path': ''} for i in range(F)]}
    anchor_frames = sorted(set(int(f) for f in frames[:n_cls].ravel() if f >= 1))
    dets_all = [{'frame': f, 'bbox': b.tolist(), 'scores': [{'score': float(s)} for s in sc[:n_cls]]}
                for f in anchor_frames for b, sc in zip(boxes_h[f - 1], scores_h[f - 1])]

    def plug_in(vid_proto, det):
        rows = oracle.iou_link_rows_box(boxes_h, det['frame'] - 1, [int(v) for v in det['bbox']], 0.5, 0)
        return tracks_proto_from_boxes(rows.astype(np.float64), vid_proto['video'], det['frame'], 1, 1)
    t_track = t_prop = 0.0
    n = 0
    out = []
    for c in range(n_cls):
        det_proto = {'video': name, 'detections': [{'frame': int(frames[c, t]), 'bbox': ab[c, t].tolist()}
                                                   for t in range(frames.shape[1]) if frames[c, t] >= 1]}
        t0 = time.perf_counter()
        tp = K.track_from_det(vid, det_proto, plug_in)
        t1 = time.perf_counter()
        sp = TC.anchor_propagate(vid, tp, {'video': name, 'detections': dets_all}, c + 1)
        t_prop += time.perf_counter() - t1
        t_track += t1 - t0
        n += len(det_proto['detections'])
        out.append(sp)
    return t_track, t_prop, n, out


def torch_route(boxes, scores, T, frame_mode):
    """what a caller can do without ops.top_anchors: a transposed copy, torch.topk, the box gather"""
    F, B, C = scores.shape
    if frame_mode:
        v, i = scores.permute(2, 0, 1).topk(T, dim=2)            # [C,F,T]
        f = torch.arange(F, device=scores.device)[None, :, None].expand_as(i)
        return (f + 1).reshape(C, -1), boxes[f, i].reshape(C, -1, 4), v.reshape(C, -1), i.reshape(C, -1)
    v, i = scores.permute(2, 0, 1).reshape(C, -1).topk(T)
    f, b = i // B, i % B
    return f + 1, boxes[f, b], v, b


def select_legs(res, boxes, scores, a):
    from vdetlib_amd.utils import protocol
    F, B, C = scores.shape
    vol = scores.numel() * 4
    legs = {}
    for name, T, mode in (("video_T10", 10, 'video'), ("video_T100", 100, 'video'), ("frame_top1", 1, 'frame')):
        ev, wall = device_times(lambda s: ops.top_anchors(boxes, scores, T, mode=mode, sync=s), a.reps, a.warmup)
        tev, _ = device_times(lambda s: (torch_route(boxes, scores, T, mode == 'frame'), torch.cuda.synchronize() if s else None),
                              a.reps, a.warmup)
        mine = ops.top_anchors(boxes, scores, T, mode=mode)
        theirs = torch_route(boxes, scores, T, mode == 'frame')
        legs[name] = {"event_ms": ev, "wall_ms": wall, "torch_topk_event_ms": tev,
                      "volume_tb_s": round(vol / (ev["median"] * 1e-3) / 1e12, 3),
                      "same_scores_as_torch": bool(torch.equal(mine[2], theirs[2]))}
    # the host route on a few classes of a slice the dicts can hold, scaled by detections and classes
    ncls, Fh = max(1, min(a.host_classes, C)), min(F, 3)
    sh = scores[:Fh, :, :ncls].cpu().numpy()
    bh = boxes[:Fh].cpu().numpy()
    dets = {'video': 'c2', 'detections': [{'frame': f + 1, 'bbox': bh[f, b].tolist(),
                                            'scores': [{'class_index': c, 'score': float(sh[f, b, c])} for c in range(ncls)]}
                                           for f in range(Fh) for b in range(B)]}
    t0 = time.perf_counter()
    for c in range(ncls):
        protocol.top_detections(dets, 10, c)
    legs["host_top_detections_s_scaled"] = round((time.perf_counter() - t0) * (F / Fh) * (C / ncls), 2)
    legs["host_top_detections_timed"] = {"frames": Fh, "classes": ncls}
    # the 64-video VID-shape batch: select, link, propagate
    vb, vs, off = bench.synth_vid_batch(torch, boxes.device, 64)
    sel = lambda s: ops.top_anchors(vb, vs, 10, frame_off=off, sync=s)
    fr, ab, sc, _ = sel(True)
    link = lambda s: ops.track_from_anchors_batch(vb, off, fr, ab, sc, sync=s)
    out = link(True)
    prop = lambda s: ops.anchor_propagate_tracks_batch(out, vb, vs, sync=s)
    batch = {"videos": len(off) - 1, "frames": int(off[-1]), "boxes_per_frame": int(vb.shape[1]), "classes": int(vs.shape[2])}
    for name, fn in (("top_anchors", sel), ("track_from_anchors_batch", link), ("anchor_propagate_tracks_batch", prop)):
        ev, wall = device_times(fn, a.reps, a.warmup)
        batch[name] = {"event_ms": ev, "wall_ms": wall}
    batch["top_anchors"]["volume_tb_s"] = round(vs.numel() * 4 / (batch["top_anchors"]["event_ms"]["median"] * 1e-3) / 1e12, 3)
    legs["vid_batch"] = batch
    res["d_top_anchors"] = legs


def main():
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-classes", type=int, default=2)
    ap.add_argument("--select", action="store_true", help="only the top_anchors legs (d)")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup}
    F, B, C, T = 300, 10000, 200, 10
    boxes, scores = bench.synth_video_cuda(torch, 2000, F, B, C, dev)
    if a.select:
        select_legs(res, boxes, scores, a)
        print(json.dumps(res))
        return
    # ---- (c) the greedy tracker: its anchors, its tubelets, its stage times
    cx = _lib.get_context(0)
    ops.nms_track_volume(boxes, scores, max_tracks=T, pad=False)
    cx.set_timing(True)
    _, _, tr, an, nt = ops.nms_track_volume(boxes, scores, max_tracks=T, pad=False)
    stages = cx.last_timing()
    cx.set_timing(False)
    res["c_nms_track_volume_stage_ms"] = {k: {"ms": round(stages[k][0], 4), "launches": stages[k][1]}
                                          for k in ("track_link", "track_loop", "track_pick", "track_suppress")}
    live = torch.arange(T, device=dev)[None, :] < nt[:, None]
    frames = torch.where(live, an[..., 0], torch.zeros_like(an[..., 0])).to(torch.int32)
    idx = torch.where(live, an[..., 1], torch.zeros_like(an[..., 1])).long()
    ab = boxes[(frames.long() - 1).clamp(min=0), idx].contiguous()
    sc = an[..., 2].contiguous()
    # ---- (b) the new calls
    link = lambda s: ops.track_from_anchors(boxes, frames, ab, sc, sync=s)
    mt, ma, mnt = link(True)
    prop = lambda s: ops.anchor_propagate_tracks(mt, mnt, ma, boxes, scores, sync=s)
    det, best = prop(True)
    rows_equal = bool(torch.equal(torch.nan_to_num(mt, nan=-7.0)[live], torch.nan_to_num(tr, nan=-7.0)[live])) and \
        bool(torch.equal(mnt, nt))
    ev_l, wall_l = device_times(link, a.reps, a.warmup)
    ev_p, wall_p = device_times(prop, a.reps, a.warmup)
    steps = int((~torch.isnan(mt[..., 0])).sum()) - int(live.sum())
    res["b_track_from_anchors"] = {"anchors": int(live.sum()), "chains": 2 * int(live.sum()), "linked_steps": steps,
                                   "pair_tests": steps * B, "rows_equal_greedy": rows_equal, "event_ms": ev_l, "wall_ms": wall_l,
                                   "pair_tests_per_s": round(steps * B / (ev_l["median"] * 1e-3), 0)}
    res["b_anchor_propagate_tracks"] = {"event_ms": ev_p, "wall_ms": wall_p,
                                        "best_is_the_anchor": bool(torch.equal(best[live].long(), idx[live]))}
    # ---- (a) the dict route, first classes only, scaled
    ncls = max(1, min(a.host_classes, C))
    bh, sh = boxes.cpu().numpy(), scores[..., :ncls].cpu().numpy()
    fh, abh = frames.cpu().numpy(), ab.cpu().numpy()
    t_track, t_prop, n, protos = dict_route('c2', bh, sh, fh, abh, ncls, F)
    mth, deth = mt.cpu().numpy(), det.cpu().numpy()
    same = True
    for c, sp in enumerate(protos):
        for t, tub in enumerate(sp['tubelets']):
            for box in tub['boxes']:
                f = box['frame'] - 1
                same = same and box['bbox'] == [int(v) for v in mth[c, t, f, :4]] and float(box['det_score']) == deth[c, t, f]
    scale = int(live.sum()) / max(n, 1)
    res["a_dict_route"] = {"classes_timed": ncls, "anchors_timed": n, "track_from_det_s": round(t_track * scale, 2),
                           "anchor_propagate_s": round(t_prop * scale, 2), "equal_to_device": bool(same),
                           "a_over_b_wall": round((t_track + t_prop) * scale * 1e3 / (wall_l["median"] + wall_p["median"]), 1)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
