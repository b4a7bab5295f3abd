#!/usr/bin/env python3
"""The device pixel tracker (ops.track_pixels) on the c2 anchors -- 200 classes x 10, chosen by ops.top_anchors on the c2
detection volume -- over a 300-frame 720 x 1280 video whose pixels are synthetic: a seeded smooth texture that pans:
  python devtools/bench_pixtrack.py [--reps R] [--warmup W] [--frames F] [--host-chains N]
Settings grid 32 / radius 8, step 3.  Comparators, never the code under test:
 (b) ops.track_from_anchors on the same anchors: the IoU link does different work (it scans proposals, not pixels) and is
     there for scale only;
 (c) a torch formulation of ONE step for all chains (gather, unfold, absolute difference, sum, argmin) timed on one frame
     pair and multiplied by the steps the device took per chain: EXTRAPOLATED;
 (d) the numpy spec (tests/pixtrack_spec.py) on a handful of chains, scaled to all of them: EXTRAPOLATED.
HIP-event ms, median [min .. max] of R calls after W warm-up calls; legs (a) and (b) alternate and the whole turn runs twice,
so the spread of each shows.  Prints one JSON line."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

S, R, STEP, T = 32, 8, 3, 10


def panning_video(dev, F, H, W, seed=2031):
    """uint8 [F,H,W,3]: a smooth seeded texture (noise on a 1/8 lattice, bilinear) seen through a window that pans by
    (2, 1) pixels a frame"""
    g = torch.Generator(device=dev).manual_seed(seed)
    hh, ww = H + F + 16, W + 2 * F + 16
    coarse = torch.rand(1, 3, hh // 8 + 2, ww // 8 + 2, generator=g, device=dev)
    tex = torch.nn.functional.interpolate(coarse, scale_factor=8, mode='bilinear', align_corners=False)[0, :, :hh, :ww]
    tex = (tex * 255).round().clamp(0, 255).to(torch.uint8).permute(1, 2, 0).contiguous()
    out = torch.empty((F, H, W, 3), dtype=torch.uint8, device=dev)
    for f in range(F):
        out[f] = tex[f:f + H, 2 * f:2 * f + W]
    return out


def torch_step(images, f, g, boxes0, chunk=250):
    """one step f -> g of every chain in torch: boxes0 int64 [N,4] 0-based.  Returns (SAD, dy, dx) of the spec's winner."""
    dev = images.device
    H, W = images.shape[1], images.shape[2]
    w = torch.tensor([29, 150, 77], device=dev, dtype=torch.int32)
    lf = ((images[f].to(torch.int32) * w).sum(-1) + 128) >> 8
    lg = lf if g == f else ((images[g].to(torch.int32) * w).sum(-1) + 128) >> 8
    d = torch.arange(-R, R + 1, device=dev)
    tie = (((d[:, None] ** 2 + d[None, :] ** 2) << 16) | ((d[:, None] + R) << 8) | (d[None, :] + R)).reshape(-1)
    outs = []
    for a in range(0, boxes0.shape[0], chunk):
        b = boxes0[a:a + chunk]
        bw, bh = b[:, 2] - b[:, 0] + 1, b[:, 3] - b[:, 1] + 1
        k = torch.arange(-R, S + R, device=dev)
        cols = (b[:, :1] + torch.div((2 * k[None] + 1) * bw[:, None], 2 * S, rounding_mode='floor')).clamp(0, W - 1)
        rows = (b[:, 1:2] + torch.div((2 * k[None] + 1) * bh[:, None], 2 * S, rounding_mode='floor')).clamp(0, H - 1)
        tm = lf[rows[:, R:R + S, None], cols[:, None, R:R + S]].to(torch.int16)               # [n,S,S]
        rg = lg[rows[:, :, None], cols[:, None, :]].to(torch.int16)                            # [n,P,P]
        win = rg.unfold(1, S, 1).unfold(2, S, 1)                                               # [n,2R+1,2R+1,S,S]
        sad = (win - tm[:, None, None]).abs().sum((3, 4), dtype=torch.int64).reshape(b.shape[0], -1)
        best = ((sad << 32) | tie[None]).argmin(1)
        outs.append(torch.stack([sad.gather(1, best[:, None])[:, 0], best // (2 * R + 1) - R, best % (2 * R + 1) - R], 1))
    return torch.cat(outs)


def main():
    import argparse
    import bench
    from bench_tcn import device_times
    from vdetlib_amd import ops
    import pixtrack_spec as px
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--boxes", type=int, default=10000)
    ap.add_argument("--host-chains", type=int, default=4)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    F, H, W, C = a.frames, 720, 1280, 200
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup, "frames": F, "image": [H, W],
           "grid": S, "radius": R, "step": STEP}
    boxes, scores = bench.synth_video_cuda(torch, 2000, F, a.boxes, C, dev)
    fr, ab, sc, _ = ops.top_anchors(boxes, scores, T)
    del scores
    images = panning_video(dev, F, H, W)
    new = lambda s: ops.track_pixels(images, fr, ab, sc, grid=S, radius=R, step=STEP, sync=s)
    old = lambda s: ops.track_from_anchors(boxes, fr, ab, sc, sync=s)
    tracks = new(True)[0]
    live = tracks[..., 0] == tracks[..., 0]
    anchors = int((fr > 0).sum())
    steps = int(live.sum()) - anchors
    res["a_track_pixels"] = {"anchors": anchors, "chains": 2 * anchors, "steps": steps, "mean_confidence": round(float(tracks[..., 4][live].mean()), 4)}
    res["b_track_from_anchors"] = {"note": "different work (IoU link over %d proposals a frame, every frame): for scale" % a.boxes}
    for rnd in ("round1", "round2"):
        for name, fn in (("a_track_pixels", new), ("b_track_from_anchors", old)):
            ev, wall = device_times(fn, a.reps, a.warmup)
            res[name][rnd] = {"event_ms": ev, "wall_ms": wall}
    med = res["a_track_pixels"]["round1"]["event_ms"]["median"]
    idx = torch.arange(F, device=dev)[None, None, :]
    af = (fr.long() - 1)[..., None]
    longest = int(max((live & (idx > af)).sum(-1).max(), (live & (idx < af)).sum(-1).max()))
    res["a_track_pixels"]["longest_chain_steps"] = longest
    res["a_track_pixels"]["us_per_step_of_the_longest_chain"] = round(med * 1e3 / max(longest, 1), 3)     # (an upper bound on a dependent step)
    # (c) torch, one frame pair, all chains: EXTRAPOLATED to the steps the device took
    b0 = ab.reshape(-1, 4).to(torch.int64) - 1                       # (the c2 anchors are integer-valued and inside the image)
    f0 = F // 2
    mine = torch_step(images, f0, min(f0 + STEP, F - 1), b0)
    ev, wall = device_times(lambda s: (torch_step(images, f0, min(f0 + STEP, F - 1), b0), torch.cuda.synchronize() if s else None),
                            max(a.reps // 4, 3), 1)
    res["c_torch_one_step_all_chains"] = {"event_ms": ev, "chains_in_the_step": int(b0.shape[0]),
                                          "EXTRAPOLATED_video_ms": round(ev["median"] * steps / max(int(b0.shape[0]), 1), 1)}
    # (d) the numpy spec on a handful of chains: EXTRAPOLATED (the luma planes are made on the device: same integers)
    n = max(1, min(a.host_chains, T))
    w3 = torch.tensor([29, 150, 77], device=dev, dtype=torch.int32)
    lum = torch.stack([(((images[f].to(torch.int32) * w3).sum(-1) + 128) >> 8).to(torch.uint8) for f in range(F)]).cpu().numpy()
    frh, abh, got = fr[0, :n].cpu().numpy(), ab[0, :n].cpu().numpy(), tracks[0, :n].cpu().numpy()
    t0 = time.perf_counter()
    want = np.stack([px.track_slot(lum, int(frh[q]), px.anchor_state(frh[q], abh[q], F, H, W)[1], S, R, 0.5, 0, STEP) for q in range(n)])
    dt = time.perf_counter() - t0
    hsteps = int(np.isfinite(want[..., 0]).sum()) - n
    res["d_host_spec"] = {"slots": n, "steps": hsteps, "seconds": round(dt, 2),
                          "equal_to_device": bool(np.array_equal(want, got, equal_nan=True)),
                          "EXTRAPOLATED_video_s": round(dt * steps / max(hsteps, 1), 1)}
    # the torch step agrees with the spec's winner on the handful
    f1 = min(f0 + STEP, F - 1)
    agree = True
    for q in range(n):
        box = tuple(int(v) for v in b0[q].tolist())
        sad, dy, dx = px.best_shift(px.sample(lum[f0], box, S, 0, S), px.sample(lum[f1], box, S, -R, S + R), R)
        agree = agree and [sad, dy, dx] == mine[q].tolist()
    res["c_torch_one_step_all_chains"]["equal_to_spec_on_the_handful"] = agree
    print(json.dumps(res))


if __name__ == "__main__":
    main()
