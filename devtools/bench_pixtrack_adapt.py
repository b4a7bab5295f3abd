#!/usr/bin/env python3
"""Template update with an anchor guard for the pixel tracker (the ``update`` / ``update_conf`` / ``drift_conf`` keywords of
ops.track_pixels, track_pixels_scaled and track_volume_pixels) on the c2 anchors -- 200 classes x 10, chosen by
ops.top_anchors on the c2 detection volume -- over the 300-frame 720 x 1280 panning and zooming videos of
devtools/bench_pixtrack_scaled.py:
  python devtools/bench_pixtrack_adapt.py [--reps R] [--warmup W] [--frames F] [--boxes B] [--no-greedy]
Settings grid 32 / radius 8 / step 3, scale_step 5, no penalty, update 64 at the default confidences.
Legs:
 (a) per video, ops.track_pixels and ops.track_pixels_scaled(scales=1) as they are -- the fixed-template kernels, the
     comparator -- and with update = 64: point sampling, and box sampling with the integral passed in (against the fixed
     template's box leg);
 (b) ops.track_volume_pixels at step 1 and step 3 (panning video only): the fixed template against update = 64;
 (c) quality: the panning video re-made with seeded moves of 1 .. 3 columns and 0 .. 2 rows a frame and a texture that fades
     linearly into another one over the video, ops.track_pixels at step 1, min_conf 0.8: the mean chain length (rows a
     tubelet, the anchor row included) and the mean distance of a tubelet's box from its planted track, the fixed template
     against update = 64 with the default guard and with the guard off (drift_conf = 0).
HIP-event ms, median [min .. max] of R calls after W warm-up calls; the legs alternate and the whole turn runs twice, so the
spread of each shows.  Per tracker leg also the chain steps taken; per adaptive leg the time per step relative to its
fixed-template leg's.  Prints one JSON line."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "devtools"))
import torch

S, R, STEP, T, C, P, UPDATE = 32, 8, 3, 10, 200, 5, 64


def fading_video(dev, F, H, W, seed=2041):
    """bench_pixtrack_box.jittered_video with TWO textures: frame f shows (1 - t) * A + t * B, t = f / (F - 1), through the
    moving window -> (uint8 [F,H,W,3], offsets int64 [F,2])"""
    g = torch.Generator(device=dev).manual_seed(seed)
    hh, ww = H + 2 * F + 16, W + 3 * F + 16
    tex = []
    for _ in range(2):
        coarse = torch.rand(1, 3, hh // 8 + 2, ww // 8 + 2, generator=g, device=dev)
        t = torch.nn.functional.interpolate(coarse, scale_factor=8, mode='bilinear', align_corners=False)[0, :, :hh, :ww]
        tex.append((t * 255).permute(1, 2, 0).contiguous())
    cpu = torch.Generator().manual_seed(seed)
    moves = torch.stack([torch.randint(1, 4, (F,), generator=cpu), torch.randint(0, 3, (F,), generator=cpu)], 1)
    moves[0] = 0
    off = moves.cumsum(0)
    out = torch.empty((F, H, W, 3), dtype=torch.uint8, device=dev)
    for f in range(F):
        x, y = int(off[f, 0]), int(off[f, 1])
        t = f / float(max(F - 1, 1))
        out[f] = ((1 - t) * tex[0][y:y + H, x:x + W] + t * tex[1][y:y + H, x:x + W]).round().clamp(0, 255).to(torch.uint8)
    return out, off


def main():
    import argparse
    import bench
    from bench_pixtrack import panning_video
    from bench_pixtrack_box import quality, shape_of
    from bench_pixtrack_scaled import zooming_video
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
           "radius": R, "step": STEP, "scale_step": P, "scale_penalty": 0, "update": UPDATE, "update_conf": 0.8, "drift_conf": 0.7}
    boxes, scores = bench.synth_video_cuda(torch, 2000, F, a.boxes, C, dev)
    fr, ab, sc, _ = ops.top_anchors(boxes, scores, T)
    anchors = int((fr > 0).sum())
    res["anchors"] = anchors
    both = lambda fn, reps=a.reps: dict(zip(("event_ms", "wall_ms"), device_times(fn, reps, a.warmup)))
    per_step = lambda leg: leg["round1"]["event_ms"]["median"] / max(leg["steps"], 1)
    for vname, video in (("panning", panning_video), ("zooming", zooming_video)):
        images = video(dev, F, H, W)
        out = res[vname] = {}
        integ = ops.luma_integral(images)
        legs = []
        for tag, call, kw in (("track_pixels", ops.track_pixels, {}),
                              ("track_pixels_scaled_1", ops.track_pixels_scaled, dict(scales=1, scale_step=P))):
            run = lambda s, call=call, kw=kw, **m: call(images, fr, ab, sc, grid=S, radius=R, step=STEP, sync=s, **dict(kw, **m))
            legs.append(("a_%s_fixed_point" % tag, None, run))
            legs.append(("a_%s_update_point" % tag, "a_%s_fixed_point" % tag, lambda s, run=run: run(s, update=UPDATE)))
            legs.append(("a_%s_fixed_box" % tag, None, lambda s, run=run: run(s, sampling='box', integral=integ)))
            legs.append(("a_%s_update_box" % tag, "a_%s_fixed_box" % tag,
                         lambda s, run=run: run(s, sampling='box', integral=integ, update=UPDATE)))
        for name, base, fn in legs:
            out[name] = shape_of(fn(True)[0], anchors)
        for rnd in ("round1", "round2"):
            for name, base, fn in legs:
                out[name][rnd] = both(fn)
        for name, base, fn in legs:
            if base:
                out[name]["per_step_over_fixed"] = round(per_step(out[name]) / per_step(out[base]), 3)
        if vname == "panning" and not a.no_greedy:                 # (b)
            glegs = []
            for step in (1, 3):
                run = lambda s, st=step, **m: ops.track_volume_pixels(images, boxes, scores, max_tracks=T, grid=S, radius=R, step=st, sync=s, **m)
                glegs.append(("b_track_volume_pixels_fixed_step%d" % step, None, run))
                glegs.append(("b_track_volume_pixels_update_step%d" % step, "b_track_volume_pixels_fixed_step%d" % step,
                              lambda s, run=run: run(s, update=UPDATE)))
            for name, base, fn in glegs:
                tr, _, nt = fn(True)
                out[name] = shape_of(tr, int(nt.sum()))
                out[name]["tubelets"] = int(nt.sum())
            for rnd in ("round1", "round2"):
                for name, base, fn in glegs:
                    out[name][rnd] = both(fn)
            for name, base, fn in glegs:
                if base:
                    out[name]["per_step_over_fixed"] = round(per_step(out[name]) / per_step(out[base]), 3)
        del images, integ
    images, off = fading_video(dev, F, H, W)                       # (c)
    q = res["quality_fading_pan"] = {"min_conf": 0.8}
    for name, kw in (("fixed", {}), ("update_default_guard", dict(update=UPDATE)), ("update_guard_off", dict(update=UPDATE, drift_conf=0.0))):
        tracks = ops.track_pixels(images, fr, ab, sc, grid=S, radius=R, step=1, min_conf=0.8, **kw)[0]
        q[name] = quality(tracks, fr, ab, off)
        q[name]["mean_chain_rows"] = round((q[name]["rows"] + anchors) / float(max(anchors, 1)), 2)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
