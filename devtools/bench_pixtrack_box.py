#!/usr/bin/env python3
"""Box-filter sampling for the pixel tracker (ops.luma_integral; sampling='box' of ops.track_pixels, track_pixels_scaled and
track_volume_pixels) on the c2 anchors -- 200 classes x 10, chosen by ops.top_anchors on the c2 detection volume -- over the
300-frame 720 x 1280 panning and zooming videos of devtools/bench_pixtrack_scaled.py:
  python devtools/bench_pixtrack_box.py [--reps R] [--warmup W] [--frames F] [--boxes B] [--no-greedy]
Settings grid 32 / radius 8 / step 3, scale_step 5, no penalty.  Legs:
 (a) ops.luma_integral of the video against luma.to(int64).cumsum(1).cumsum(2) in torch on the same frames (the luma plane is
     made before the clock starts), with the bytes the integral must move (the frames in, the table out) per second;
 (b) per video, ops.track_pixels and ops.track_pixels_scaled(scales=1): point sampling, box sampling with the integral passed
     in, box sampling with the integral built inside the call;
 (c) ops.track_volume_pixels at step 1 and step 3 (panning video only): point against box with the integral passed in;
 (d) quality: the panning video re-made with seeded moves of 1 .. 3 columns and 0 .. 2 rows a frame (whole pixels, not
     multiples of a pitch), ops.track_pixels at step 1, min_conf 0: the mean distance of a tubelet's box from its planted track
     (the anchor box carried along with the pan) and the mean confidence, point against box.
HIP-event ms, median [min .. max] of R calls after W warm-up calls; the legs alternate and the whole turn runs twice, so the
spread of each shows.  Per tracker leg also the chain steps taken; per box leg the time per step relative to the point leg's.
Prints one JSON line."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "devtools"))
import torch

S, R, STEP, T, C, P = 32, 8, 3, 10, 200, 5


def luma_of(images):
    w = torch.tensor([29, 150, 77], device=images.device, dtype=torch.int32)
    return (((images.to(torch.int32) * w).sum(-1) + 128) >> 8).to(torch.uint8)


def jittered_video(dev, F, H, W, seed=2031):
    """bench_pixtrack.panning_video's texture seen through a window that moves by a seeded 1 .. 3 columns and 0 .. 2 rows a
    frame -> (uint8 [F,H,W,3], offsets int64 [F,2]: the window's (column, row) on every frame)"""
    g = torch.Generator(device=dev).manual_seed(seed)
    hh, ww = H + 2 * F + 16, W + 3 * F + 16
    coarse = torch.rand(1, 3, hh // 8 + 2, ww // 8 + 2, generator=g, device=dev)
    tex = torch.nn.functional.interpolate(coarse, scale_factor=8, mode='bilinear', align_corners=False)[0, :, :hh, :ww]
    tex = (tex * 255).round().clamp(0, 255).to(torch.uint8).permute(1, 2, 0).contiguous()
    cpu = torch.Generator().manual_seed(seed)
    moves = torch.stack([torch.randint(1, 4, (F,), generator=cpu), torch.randint(0, 3, (F,), generator=cpu)], 1)
    moves[0] = 0
    off = moves.cumsum(0)
    out = torch.empty((F, H, W, 3), dtype=torch.uint8, device=dev)
    for f in range(F):
        x, y = int(off[f, 0]), int(off[f, 1])
        out[f] = tex[y:y + H, x:x + W]
    return out, off


def shape_of(tracks, live_slots):
    live = tracks[..., 0] == tracks[..., 0]
    return {"steps": int(live.sum()) - live_slots, "mean_confidence": round(float(tracks[..., 4][live].mean()), 4),
            "longest_tubelet_rows": int(live.sum(-1).max())}


def quality(tracks, fr, ab, off):
    """mean distance (pixels) of the rows' (x1, y1) from the planted track, over the rows off the anchor frame; mean confidence"""
    C_, T_, F = tracks.shape[:3]
    off = off.to(tracks.device).to(torch.float32)
    af = (fr.clamp(min=1) - 1).long()                                     # [C,T]
    shift = off[af][:, :, None, :] - off[None, None, :, :]                # content moves against the window: [C,T,F,2]
    planted = ab[:, :, None, :2].floor() + shift
    live = tracks[..., 0] == tracks[..., 0]
    live &= torch.arange(F, device=tracks.device)[None, None, :] != af[:, :, None]
    d = ((tracks[..., :2] - planted) ** 2).sum(-1).sqrt()
    return {"rows": int(live.sum()), "mean_distance_px": round(float(d[live].mean()), 3),
            "mean_confidence": round(float(tracks[..., 4][live].mean()), 4)}


def main():
    import argparse
    import bench
    from bench_pixtrack import panning_video
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
           "radius": R, "step": STEP, "scale_step": P, "scale_penalty": 0}
    boxes, scores = bench.synth_video_cuda(torch, 2000, F, a.boxes, C, dev)
    fr, ab, sc, _ = ops.top_anchors(boxes, scores, T)
    anchors = int((fr > 0).sum())
    res["anchors"] = anchors
    both = lambda fn, reps=a.reps: dict(zip(("event_ms", "wall_ms"), device_times(fn, reps, a.warmup)))
    for vname, video in (("panning", panning_video), ("zooming", zooming_video)):
        images = video(dev, F, H, W)
        out = res[vname] = {}
        if vname == "panning":                  # (a)
            luma = luma_of(images)
            want = luma.to(torch.int64).cumsum(1).cumsum(2)
            got = ops.luma_integral(images).to(torch.int64)
            assert torch.equal(got[:, 1:, 1:], want) and not bool(got[:, 0].any()) and not bool(got[:, :, 0].any())
            del want, got
            ilegs = [("a_luma_integral", lambda s: ops.luma_integral(images, sync=s)),
                     ("a_torch_int64_cumsum", lambda s: luma.to(torch.int64).cumsum(1).cumsum(2))]
            ia = res["integral"] = {name: {} for name, _ in ilegs}
            for rnd in ("round1", "round2"):
                for name, fn in ilegs:
                    ia[name][rnd] = both(fn)
            moved = images.numel() + 4 * F * (H + 1) * (W + 1)
            ia["bytes_in_plus_out"] = moved
            ia["a_luma_integral"]["gb_per_s_of_in_plus_out"] = round(moved / ia["a_luma_integral"]["round1"]["event_ms"]["median"] / 1e6, 1)
            ia["integral_over_torch"] = round(ia["a_luma_integral"]["round1"]["event_ms"]["median"] /
                                              ia["a_torch_int64_cumsum"]["round1"]["event_ms"]["median"], 4)
            del luma
        integ = ops.luma_integral(images)
        legs = []
        for tag, call, kw in (("track_pixels", ops.track_pixels, {}),
                              ("track_pixels_scaled_1", ops.track_pixels_scaled, dict(scales=1, scale_step=P))):
            run = lambda s, call=call, kw=kw, **m: call(images, fr, ab, sc, grid=S, radius=R, step=STEP, sync=s, **dict(kw, **m))
            legs.append(("b_%s_point" % tag, None, run))
            legs.append(("b_%s_box_integral_passed" % tag, "b_%s_point" % tag, lambda s, run=run: run(s, sampling='box', integral=integ)))
            legs.append(("b_%s_box_integral_built" % tag, "b_%s_point" % tag, lambda s, run=run: run(s, sampling='box')))
        for name, base, fn in legs:
            out[name] = shape_of(fn(True)[0], anchors)
        for rnd in ("round1", "round2"):
            for name, base, fn in legs:
                out[name][rnd] = both(fn)
        per_step = lambda leg: leg["round1"]["event_ms"]["median"] / max(leg["steps"], 1)
        for name, base, fn in legs:
            if base:
                out[name]["per_step_over_point"] = round(per_step(out[name]) / per_step(out[base]), 3)
        if vname == "panning" and not a.no_greedy:                 # (c)
            glegs = []
            for step in (1, 3):
                run = lambda s, st=step, **m: ops.track_volume_pixels(images, boxes, scores, max_tracks=T, grid=S, radius=R, step=st, sync=s, **m)
                glegs.append(("c_track_volume_pixels_point_step%d" % step, None, run))
                glegs.append(("c_track_volume_pixels_box_step%d" % step, "c_track_volume_pixels_point_step%d" % step,
                              lambda s, run=run: run(s, sampling='box', integral=integ)))
            for name, base, fn in glegs:
                tr, _, nt = fn(True)
                out[name] = shape_of(tr, int(nt.sum()))
                out[name]["tubelets"] = int(nt.sum())
            for rnd in ("round1", "round2"):
                for name, base, fn in glegs:
                    out[name][rnd] = both(fn)
            for name, base, fn in glegs:
                if base:
                    out[name]["per_step_over_point"] = round(per_step(out[name]) / per_step(out[base]), 3)
        del images, integ
    images, off = jittered_video(dev, F, H, W)                     # (d)
    q = res["quality_jittered_pan"] = {}
    for name, kw in (("point", {}), ("box", dict(sampling='box'))):
        tracks = ops.track_pixels(images, fr, ab, sc, grid=S, radius=R, step=1, min_conf=0.0, **kw)[0]
        q[name] = quality(tracks, fr, ab, off)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
