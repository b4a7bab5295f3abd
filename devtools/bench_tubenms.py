#!/usr/bin/env python3
"""NMS over whole tubelets (ops.nms_tubelets / ops.nms_tubelets_batch):
  python devtools/bench_tubenms.py [--reps R] [--warmup W] [--boxes B] [--spec-classes N] [--skip-flow]
 (a) c2: one c2 video, 200 classes x 300 frames.  "merged20": the 10 + 10 tubelets of devtools/bench_tracknms.py (the second ten
     are the first ten jittered by +/-3 px), put together by ops.merge_tracks('combine').  "dense100": five jittered copies of
     those 20 side by side -- every pair shares every frame, 300 M frame pairs, the most a T = 100 set can ask for.
     "anchors100": ops.top_anchors(100) + ops.track_from_anchors on the same video (random proposals: the chains are short, the
     extents rarely meet).  Legs per set: every norm, with and without return_overlaps; beside them ops.nms_tracks on the same
     tubelets (DIFFERENT work, per-frame lists: for scale), a torch statement of the same rule (broadcast IoU [C,T,T,F] in f32,
     sums, a T-step masked loop without a host wait; classes in chunks to bound its memory; NOT bit-equal) and the numpy spec on N
     classes, scaled to 200: EXTRAPOLATED.
 (b) vid64: the 64-video VID batch of bench.synth_vid_batch, 30 classes x 20 tubelets per video, one nms_tubelets_batch call.
 (c) flow: on devtools/bench_greedy_pixels.py's video, ops.top_anchors(3 x 10) + ops.track_pixels(step 3) + ops.nms_tubelets
     against ops.track_volume_pixels(max_tracks 10, step 3): whole-call times, tubelets per class, and the mean IoU of the kept
     tubelets' boxes with the planted track of their anchor (the texture pans by (2, 1) px a frame, so the patch under an anchor
     box moves by (-2, -1)).
HIP-event and wall ms per call, median [min .. max] of R calls after W warm-up calls; the legs of a set are run in order TWICE,
both passes are printed.  No ratio is a pass condition.  Prints one JSON line."""
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

import bench
from bench_tcn import device_times
from bench_tracknms import make_inputs
from vdetlib_amd import ops

NORMS = ('union', 'shared', 'min')
THRESH = 0.5


def torch_rule(tracks, ntracks, ts, thresh=THRESH, chunk=10):
    """the rule with norm 'union' in torch f32 / f64: (kept [C,T] bool, ovr of the last chunk).  No host wait."""
    C, T, F = tracks.shape[:3]
    order = torch.argsort(-ts, dim=1, stable=True)
    kept = torch.zeros((C, T), dtype=torch.bool, device=tracks.device)
    ar = torch.arange(T, device=tracks.device)
    for c0 in range(0, C, chunk):
        b = tracks[c0:c0 + chunk, :, :, :4]
        ex = (b[..., 0] == b[..., 0]) & (ar[None, :, None] < ntracks[c0:c0 + chunk, None, None])
        area = (b[..., 2] - b[..., 0] + 1) * (b[..., 3] - b[..., 1] + 1)
        w = (torch.minimum(b[:, :, None, :, 2], b[:, None, :, :, 2]) - torch.maximum(b[:, :, None, :, 0], b[:, None, :, :, 0]) + 1).clamp(min=0)
        h = (torch.minimum(b[:, :, None, :, 3], b[:, None, :, :, 3]) - torch.maximum(b[:, :, None, :, 1], b[:, None, :, :, 1]) + 1).clamp(min=0)
        inter = w * h
        both = ex[:, :, None] & ex[:, None, :]
        q = torch.where(both, inter / (area[:, :, None] + area[:, None, :] - inter), torch.zeros_like(inter))
        S = torch.nan_to_num(q, nan=0.0).double().sum(-1)
        I = both.sum(-1)
        n = ex.sum(-1)
        den = n[:, :, None] + n[:, None, :] - I
        hit = torch.where(den > 0, S / den.clamp(min=1), torch.zeros_like(S)) >= thresh
        present = (n > 0) & (ts[c0:c0 + chunk] == ts[c0:c0 + chunk])
        alive = present.clone()
        k = torch.zeros_like(alive)
        rows = torch.arange(alive.shape[0], device=alive.device)
        for r in range(T):
            t = order[c0:c0 + chunk, r]
            a = alive[rows, t]
            k[rows, t] = a
            alive &= ~(hit[rows, t] & a[:, None])
        kept[c0:c0 + chunk] = k
    return kept


def time_legs(fns, a, res):
    for _ in range(2):
        for name, fn in fns.items():
            ev, wall = device_times(fn, a.reps, a.warmup)
            res.setdefault(name, {}).setdefault("event_ms", []).append(ev)
            res[name].setdefault("wall_ms", []).append(wall)


def tubelet_legs(d, score, a, torch_chunk, with_spec):
    """every leg on one tubelet set d (a merge_tracks dict); score [C,T,F] f64"""
    C, T, F = score.shape
    fns = {}
    for norm in NORMS:
        fns[norm] = lambda s, norm=norm: ops.nms_tubelets(d, score=score, thresh=THRESH, norm=norm, sync=s)
        fns[norm + "+overlaps"] = lambda s, norm=norm: ops.nms_tubelets(d, score=score, thresh=THRESH, norm=norm, return_overlaps=True, sync=s)
    fns["nms_tracks"] = lambda s: ops.nms_tracks(d['tracks'], d['ntracks'], score, thresh=THRESH, sync=s)
    res = {}
    out = ops.nms_tubelets(d, score=score, thresh=THRESH, return_overlaps=True)
    ts = torch.where(torch.arange(T, device=score.device)[None, :] < d['ntracks'][:, None], torch.nanmean(score, dim=2),
                     torch.full((C, T), float('nan'), device=score.device, dtype=score.dtype))
    fns["torch_rule_union"] = lambda s: (torch_rule(d['tracks'], d['ntracks'], ts, chunk=torch_chunk), s and torch.cuda.synchronize())
    kept_t = torch_rule(d['tracks'], d['ntracks'], ts, chunk=torch_chunk)
    time_legs(fns, a, res)
    live = (d['tracks'][..., 0] == d['tracks'][..., 0]) & (torch.arange(T, device=score.device)[None, :, None] < d['ntracks'][:, None, None])
    per_frame = live.sum(1).double()                    # boxes per (class, frame): n (n - 1) / 2 pairs meet there
    res["shape"] = {"classes": C, "T": T, "frames": F, "tubelets_in": int(d['ntracks'].sum()), "boxes_in": int(live.sum()),
                    "kept_per_class_mean": round(float(out['ntracks'].float().mean()), 2),
                    "torch_rule_kept_per_class_mean": round(float(kept_t.sum(1).float().mean()), 2),
                    "frame_pairs": int((per_frame * (per_frame - 1) / 2).sum())}
    res["nms_tracks"]["note"] = "different work (one list per frame and class): for scale"
    res["torch_rule_union"]["note"] = "f32 IoU summed as floats: not bit-equal"
    if with_spec:
        import tubenms_spec as spec
        n = max(1, min(a.spec_classes, C))
        tr, nt, sc = d['tracks'][:n].cpu().numpy(), d['ntracks'][:n].cpu().numpy(), score[:n].cpu().numpy()
        t0 = time.perf_counter()
        want = spec.expected(tr, nt, sc, thresh=THRESH)
        secs = time.perf_counter() - t0
        equal = all(np.array_equal(out[k][:n].cpu().numpy().view(np.uint8), want[k].view(np.uint8)) for k in ('tracks', 'src', 'tscore', 'by', 'overlaps'))
        res["numpy_spec"] = {"classes": n, "seconds": round(secs, 2), "equal_to_device": bool(equal),
                             "EXTRAPOLATED_all_classes_ms": round(secs / n * C * 1e3, 0)}
    return res


def merged_set(bo, v=0):
    """bench_tracknms's 2 * T1 slots of video v as two sets of T1, put together by merge_tracks('combine')"""
    tr, sc, nt = bo['tracks'][v], bo['pooled'][v], bo['ntracks'][v]
    C, T = tr.shape[:2]
    h = T // 2
    half = lambda lo: dict(tracks=tr[:, lo:lo + h].contiguous(), ntracks=torch.full_like(nt, h), series=(sc[:, lo:lo + h].contiguous(),),
                           anchors=torch.zeros((C, h, 3), device=tr.device))
    return ops.merge_tracks(half(0), half(h), 'combine')


def planted_iou(tracks, anchors, ntracks):
    """mean IoU of every live tubelet's boxes with its anchor box moved by the pan (-2, -1) px a frame"""
    C, T, F = tracks.shape[:3]
    dev = tracks.device
    fa = (anchors[..., 0].long() - 1).clamp(0, F - 1)                                   # [C,T]
    ab = tracks[torch.arange(C, device=dev)[:, None], torch.arange(T, device=dev)[None, :], fa][..., :4]      # [C,T,4]
    df = (torch.arange(F, device=dev)[None, None, :] - fa[..., None]).float()
    shift = torch.stack([-2 * df, -df, -2 * df, -df], -1)
    want = ab[:, :, None, :] + shift
    b = tracks[..., :4]
    w = (torch.minimum(b[..., 2], want[..., 2]) - torch.maximum(b[..., 0], want[..., 0]) + 1).clamp(min=0)
    h = (torch.minimum(b[..., 3], want[..., 3]) - torch.maximum(b[..., 1], want[..., 1]) + 1).clamp(min=0)
    area = lambda x: (x[..., 2] - x[..., 0] + 1) * (x[..., 3] - x[..., 1] + 1)
    iou = w * h / (area(b) + area(want) - w * h)
    live = (b[..., 0] == b[..., 0]) & (torch.arange(T, device=dev)[None, :, None] < ntracks[:, None, None]) & (iou == iou)
    return round(float(iou[live].mean()), 4) if bool(live.any()) else None


def flow(a):
    from bench_greedy_pixels import C, R, S, T
    from bench_pixtrack import panning_video
    dev = torch.device("cuda", 0)
    F, H, W = 300, 720, 1280
    boxes, scores = bench.synth_video_cuda(torch, 2000, F, 10000, C, dev)
    images = panning_video(dev, F, H, W)

    def route(s, keep=False):
        fr, ab, sc, _ = ops.top_anchors(boxes, scores, 3 * T, sync=False)
        tr, an, nt = ops.track_pixels(images, fr, ab, sc, grid=S, radius=R, step=3, sync=False)
        out = ops.nms_tubelets(tr, nt, sc, anchors=an, thresh=THRESH, sync=s)
        return (out, tr, an, nt) if keep else out
    greedy = lambda s: ops.track_volume_pixels(images, boxes, scores, max_tracks=T, grid=S, radius=R, step=3, sync=s)
    out, tr, an, nt = route(True, keep=True)
    gt, ga, gn = greedy(True)
    res = {"anchor_route": {"tubelets_tracked_per_class": 3 * T, "kept_per_class_mean": round(float(out['ntracks'].float().mean()), 2),
                            "kept_per_class_min_max": [int(out['ntracks'].min()), int(out['ntracks'].max())],
                            "planted_iou_kept": planted_iou(out['tracks'], out['anchors'], out['ntracks']),
                            "planted_iou_before_nms": planted_iou(tr, an, nt)},
           "greedy_loop": {"kept_per_class_mean": round(float(gn.float().mean()), 2), "planted_iou_kept": planted_iou(gt, ga, gn)}}
    time_legs({"anchor_route": route, "greedy_loop": greedy}, a, res)
    return res


def main():
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--boxes", type=int, default=2000)
    ap.add_argument("--spec-classes", type=int, default=2)
    ap.add_argument("--skip-flow", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    gen = torch.Generator(device=dev).manual_seed(2025)
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup, "thresh": THRESH}
    boxes, scores = bench.synth_video_cuda(torch, 7, 300, a.boxes, 200, dev)
    _, bo, _ = make_inputs(gen, boxes, scores, [0, 300])
    d = merged_set(bo)
    res["c2_merged20"] = tubelet_legs(d, d['series'][0], a, 50, True)
    print("c2 merged20 timed", file=sys.stderr, flush=True)
    # (a shift of the whole box: the sizes stay, so no copy degenerates into the zero union nms_tracks reports as an error)
    jit = lambda x: x + torch.randint(-3, 4, x.shape[:-1] + (2,), generator=gen, device=dev).repeat_interleave(2, -1).view(
        x.shape[:-1] + (2, 2)).transpose(-1, -2).reshape(x.shape)
    tr = torch.cat([d['tracks']] + [torch.cat((jit(d['tracks'][..., :4]), d['tracks'][..., 4:]), -1) for _ in range(4)], 1).contiguous()
    sc = torch.cat([d['series'][0] + 1e-3 * i for i in range(5)], 1).contiguous()
    d100 = dict(tracks=tr, ntracks=torch.full_like(d['ntracks'], 100), series=(sc,), anchors=torch.zeros((200, 100, 3), device=dev))
    res["c2_dense100"] = tubelet_legs(d100, sc, a, 10, True)
    print("c2 dense100 timed", file=sys.stderr, flush=True)
    del d100, tr, sc
    fr, ab, asc, _ = ops.top_anchors(boxes, scores, 100)
    tr, an, nt = ops.track_from_anchors(boxes, fr, ab, asc)
    det, _ = ops.anchor_propagate_tracks(tr, nt, an, boxes, scores)
    res["c2_anchors100"] = tubelet_legs(dict(tracks=tr, ntracks=nt, anchors=an, series=(det,)), det, a, 10, False)
    print("c2 anchors100 timed", file=sys.stderr, flush=True)
    del boxes, scores, bo, d, tr, an, nt, det
    boxes, scores, off = bench.synth_vid_batch(torch, dev, 64)
    _, bo, _ = make_inputs(gen, boxes, scores, off)
    fns = {}
    for norm in NORMS:
        fns[norm] = lambda s, norm=norm: ops.nms_tubelets_batch(bo, 'pooled', thresh=THRESH, norm=norm, sync=s)
        fns[norm + "+overlaps"] = lambda s, norm=norm: ops.nms_tubelets_batch(bo, 'pooled', thresh=THRESH, norm=norm, return_overlaps=True, sync=s)
    fns["nms_tracks_batch"] = lambda s: ops.nms_tracks_batch(bo, 'pooled', thresh=THRESH, use_tboxes=False, sync=s)
    out = ops.nms_tubelets_batch(bo, 'pooled', thresh=THRESH)
    vid = {"videos": len(off) - 1, "frames": int(off[-1]), "classes": int(bo['ntracks'].shape[1]), "T": int(bo['tracks'][0].shape[1]),
           "kept_per_class_mean": round(float(out['ntracks'].float().mean()), 2)}
    time_legs(fns, a, vid)
    vid["nms_tracks_batch"]["note"] = "different work (one list per frame and class): for scale"
    res["vid64"] = vid
    print("vid64 timed", file=sys.stderr, flush=True)
    del boxes, scores, bo, out
    if not a.skip_flow:
        res["flow"] = flow(a)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
