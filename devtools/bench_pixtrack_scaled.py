#!/usr/bin/env python3
"""The pixel tracker's scale search (ops.track_pixels_scaled, ops.track_volume_pixels_scaled) on the c2 anchors -- 200 classes
x 10, chosen by ops.top_anchors on the c2 detection volume -- over the 300-frame 720 x 1280 panning video of
devtools/bench_pixtrack.py and over a ZOOMING variant of it, so that the levels are actually taken:
  python devtools/bench_pixtrack_scaled.py [--reps R] [--warmup W] [--frames F] [--boxes B] [--no-greedy]
Settings grid 32 / radius 8, scale_step 5, no penalty.  Legs, per video:
 (a) ops.track_pixels, the fixed-scale call: the comparator, in the same run;
 (b) ops.track_pixels_scaled at scales 0, 1 and 2 (step 3, as in 10m);
 (c) ops.track_volume_pixels against ops.track_volume_pixels_scaled(scales=1), at step 1 and step 3 (panning video only).
HIP-event ms, median [min .. max] of R calls after W warm-up calls; the legs alternate and the whole turn runs twice, so the
spread of each shows.  Per leg also the chain steps taken and the mean confidence; per scaled leg the time per step relative
to the fixed-scale leg's, divided by the levels (2 * scales + 1).  Prints one JSON line."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "devtools"))
import torch

S, R, STEP, T, C, P = 32, 8, 3, 10, 200, 5


def zooming_video(dev, F, H, W, seed=2031, rate=0.004):
    """uint8 [F,H,W,3]: bench_pixtrack.panning_video's texture seen through a window that pans by (2, 1) pixels a frame AND
    magnifies about its centre by ``rate`` a frame (bilinear): an object of 100 pixels gains 0.4 pixels a frame"""
    g = torch.Generator(device=dev).manual_seed(seed)
    hh, ww = H + F + 16, W + 2 * F + 16
    coarse = torch.rand(1, 3, hh // 8 + 2, ww // 8 + 2, generator=g, device=dev)
    tex = torch.nn.functional.interpolate(coarse, scale_factor=8, mode='bilinear', align_corners=False)[:, :, :hh, :ww]
    ys = torch.arange(H, device=dev, dtype=torch.float32) - (H - 1) / 2.0
    xs = torch.arange(W, device=dev, dtype=torch.float32) - (W - 1) / 2.0
    out = torch.empty((F, H, W, 3), dtype=torch.uint8, device=dev)
    for f in range(F):
        z = 1.0 + rate * f
        sy = ys / z + (H - 1) / 2.0 + f                    # source rows and columns in the texture
        sx = xs / z + (W - 1) / 2.0 + 2 * f
        grid = torch.stack([(2 * sx[None, :].expand(H, W) + 1) / ww - 1, (2 * sy[:, None].expand(H, W) + 1) / hh - 1], -1)[None]
        frame = torch.nn.functional.grid_sample(tex, grid, mode='bilinear', padding_mode='border', align_corners=False)[0]
        out[f] = (frame * 255).round().clamp(0, 255).to(torch.uint8).permute(1, 2, 0)
    return out


def shape_of(tracks, live_slots):
    live = tracks[..., 0] == tracks[..., 0]
    wid = (tracks[..., 2] - tracks[..., 0])[live]
    return {"steps": int(live.sum()) - live_slots, "mean_confidence": round(float(tracks[..., 4][live].mean()), 4),
            "longest_tubelet_rows": int(live.sum(-1).max()), "box_width_min_max": [float(wid.min()), float(wid.max())]}


def main():
    import argparse
    import bench
    from bench_pixtrack import panning_video
    from bench_tcn import device_times
    from vdetlib_amd import ops
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--boxes", type=int, default=10000)
    ap.add_argument("--no-greedy", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    F, H, W = a.frames, 720, 1280
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup, "frames": F, "image": [H, W], "grid": S,
           "radius": R, "step": STEP, "scale_step": P, "scale_penalty": 0}
    boxes, scores = bench.synth_video_cuda(torch, 2000, F, a.boxes, C, dev)
    fr, ab, sc, _ = ops.top_anchors(boxes, scores, T)
    anchors = int((fr > 0).sum())
    res["anchors"] = anchors
    for vname, video in (("panning", panning_video), ("zooming", zooming_video)):
        images = video(dev, F, H, W)
        legs = [("a_track_pixels", 1, lambda s, im=images: ops.track_pixels(im, fr, ab, sc, grid=S, radius=R, step=STEP, sync=s))]
        for ns in (0, 1, 2):
            legs.append(("b_track_pixels_scaled_%d" % ns, 2 * ns + 1,
                         lambda s, im=images, ns=ns: ops.track_pixels_scaled(im, fr, ab, sc, grid=S, radius=R, step=STEP, scales=ns,
                                                                             scale_step=P, sync=s)))
        out = res[vname] = {}
        for name, levels, fn in legs:
            out[name] = shape_of(fn(True)[0], anchors)
        for rnd in ("round1", "round2"):
            for name, levels, fn in legs:
                ev, wall = device_times(fn, a.reps, a.warmup)
                out[name][rnd] = {"event_ms": ev, "wall_ms": wall}
        base = out["a_track_pixels"]
        per_step = lambda leg: leg["round1"]["event_ms"]["median"] / max(leg["steps"], 1)
        for name, levels, fn in legs[1:]:
            out[name]["per_step_over_fixed_scale_per_level"] = round(per_step(out[name]) / per_step(base) / levels, 3)
        if vname == "panning" and not a.no_greedy:
            glegs = []
            for step in (1, 3):
                glegs.append(("c_track_volume_pixels_step%d" % step, 1,
                              lambda s, im=images, st=step: ops.track_volume_pixels(im, boxes, scores, max_tracks=T, grid=S, radius=R,
                                                                                    step=st, sync=s)))
                glegs.append(("c_track_volume_pixels_scaled_1_step%d" % step, 3,
                              lambda s, im=images, st=step: ops.track_volume_pixels_scaled(im, boxes, scores, max_tracks=T, grid=S, radius=R,
                                                                                           step=st, scales=1, scale_step=P, sync=s)))
            for name, levels, fn in glegs:
                tr, _, nt = fn(True)
                out[name] = shape_of(tr, int(nt.sum()))
                out[name]["tubelets"] = int(nt.sum())
            for rnd in ("round1", "round2"):
                for name, levels, fn in glegs:
                    ev, wall = device_times(fn, a.reps, a.warmup)
                    out[name][rnd] = {"event_ms": ev, "wall_ms": wall}
        del images
    print(json.dumps(res))


if __name__ == "__main__":
    main()
