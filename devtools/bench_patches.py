#!/usr/bin/env python3
"""R-CNN windows on the device (ops.rcnn_patches / ops.tubelet_patches) at three shapes:
  python devtools/bench_patches.py [--reps R] [--warmup W] [--boxes N]
 a  one 720 x 1280 frame, --boxes (default 2 000) boxes of the c2 generator, crop 224, padding 16, float32 (1.2 GB of output);
 b  the same in bfloat16;
 c  ops.tubelet_patches over 8 frames of c2 anchor-route tubelets (200 classes x 10), cap = the present count, float32.
Comparators, timed in the same run and never the code under test:
 fill         ``fill_`` of a tensor of the output's size and dtype: the write floor the call is sized by (a, b, c);
 grid_sample  torch.nn.functional.affine_grid + grid_sample + mean subtraction of the same windows in f32 (a).  NOT bit-equal
              and not the same semantics at the rim: f32 arithmetic, and outside the placed rectangle it samples whatever the
              image holds there instead of writing zeros;
 host         tests/patch_spec.py, the per-window host form, timed on 20 boxes and EXTRAPOLATED linearly to the call's count.
Per leg: HIP-event time of the enqueued work, median [min .. max] of R calls after W warm-up calls; the legs are timed
alternately, twice, so the spread of each shows.  Prints one JSON line."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np
import torch

import bench
import patch_spec
from vdetlib_amd import ops

S, PAD = 224, 16
MEAN = (103.939, 116.779, 123.68)
H, W = 720, 1280


def stats(xs):
    xs = sorted(xs)
    return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1]}


def event_times(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return stats(ms)


def rounds(legs, a):
    res = {}
    for rnd in ("round1", "round2"):
        for name, fn in legs:
            res.setdefault(name, {})[rnd] = event_times(fn, a.reps, a.warmup)
    return res


def rates(res, name, nbytes):
    for rnd, r in res[name].items():
        r["out_TB_s"] = nbytes / (r["median"] * 1e-3) / 1e12
        r["ratio_to_fill"] = res["fill"][rnd]["median"] / r["median"]


def affine_thetas(boxes):
    """Per box the map from the patch's normalised coordinates to the image's (align_corners=False), from the spec's geometry."""
    th = np.zeros((len(boxes), 2, 3), np.float32)
    for i, b in enumerate(boxes):
        g = patch_spec.geometry(b, H, W, 'warp', S, PAD)
        if not g['ok']:
            th[i] = [[0, 0, 5], [0, 0, 5]]       # samples outside: zeros
            continue
        # patch pixel x -> source pixel (x - pad_w + .5) * (src_w / crop_w) - .5 + x1; normalised: n = (2*p + 1)/size - 1
        ax, ay = g['src_w'] / g['crop_w'], g['src_h'] / g['crop_h']
        cx = (-g['pad_w'] + 0.5) * ax - 0.5 + g['x1']
        cy = (-g['pad_h'] + 0.5) * ay - 0.5 + g['y1']
        # p = ax * (S*(n+1) - 1)/2 + c  ->  n_src = (2p + 1)/W - 1
        th[i, 0] = [ax * S / W, 0, (ax * (S - 1) + 2 * cx + 1) / W - 1]
        th[i, 1] = [0, ay * S / H, (ay * (S - 1) + 2 * cy + 1) / H - 1]
    return th


def main():
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--boxes", type=int, default=2000)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup, "crop_size": S, "padding": PAD}
    g = torch.Generator(device=dev).manual_seed(2027)
    N = a.boxes
    frame = torch.randint(0, 256, (1, H, W, 3), generator=g, device=dev, dtype=torch.uint8)
    boxes = bench.synth_video_cuda(torch, 7, 1, N, 1, dev)[0][0].contiguous()

    # the host form, on 20 boxes (extrapolated below)
    hb, hf = boxes[:20].cpu().numpy(), frame.cpu().numpy()
    t0 = time.perf_counter()
    hp, hok = patch_spec.rcnn_patches(hf, hb, None, 'warp', S, PAD, np.asarray(MEAN))
    host_ms = (time.perf_counter() - t0) * 1e3
    first = ops.rcnn_patches(frame, boxes[:20], crop_size=S, padding=PAD)
    res["equal_to_spec_on_20"] = bool(torch.equal(first['patches'].cpu(), torch.from_numpy(hp)) and
                                      torch.equal(first['ok'].cpu(), torch.from_numpy(hok)))

    # a / b: one frame, N boxes
    mean_t = torch.tensor(MEAN, dtype=torch.float64, device=dev)
    for key, dt in (("a_f32", torch.float32), ("b_bf16", torch.bfloat16)):
        buf = torch.empty((N, 3, S, S), dtype=dt, device=dev)
        nbytes = buf.numel() * buf.element_size()
        legs = [("rcnn_patches", lambda dt=dt: ops.rcnn_patches(frame, boxes, crop_size=S, padding=PAD, mean=mean_t, dtype=dt, sync=False)),
                ("fill", lambda buf=buf: buf.fill_(1.0))]
        if dt == torch.float32:
            theta = torch.from_numpy(affine_thetas(boxes.cpu().numpy().astype(np.float64))).to(dev)
            src = frame.permute(0, 3, 1, 2).float().expand(N, -1, -1, -1)
            m32 = mean_t.float().view(1, 3, 1, 1)

            def gs():
                grid = torch.nn.functional.affine_grid(theta, (N, 3, S, S), align_corners=False)
                return torch.nn.functional.grid_sample(src, grid, mode='bilinear', padding_mode='zeros', align_corners=False) - m32
            legs.append(("grid_sample_not_bit_equal", gs))
            out = ops.rcnn_patches(frame, boxes, crop_size=S, padding=PAD, mean=mean_t)
            ok = out['ok'].bool()
            diff = (gs() - out['patches']).abs()
            inside = out['patches'] != 0
            res["grid_sample_mean_abs_diff_inside"] = float(diff[inside].mean())
            res["windows_ok"] = int(ok.sum())
            del out, diff, inside
        r = rounds(legs, a)
        rates(r, "rcnn_patches", nbytes)
        if dt == torch.float32:
            rates(r, "grid_sample_not_bit_equal", nbytes)
            r["host_spec_ms_EXTRAPOLATED_from_20_boxes"] = host_ms / 20 * N
        r["output_bytes"] = nbytes
        r["windows"] = N
        res[key] = r
        del buf, legs
        print(key, "timed", file=sys.stderr, flush=True)

    # c: tubelet_patches over 8 frames of c2 anchor-route tubelets
    F, B, C, T = 8, 10000, 200, 10
    base, _ = bench.synth_video_cuda(torch, 7, 1, B, 1, dev)
    vb = base + 3.0 * torch.arange(F, device=dev, dtype=torch.float32)[:, None, None] + \
        torch.randint(-1, 2, (F, B, 4), generator=g, device=dev).float()
    vb[..., 2:] = torch.maximum(vb[..., 2:], vb[..., :2] + 4)
    vb = vb.contiguous()
    vs = torch.rand(F, B, C, generator=g, device=dev)
    fr, ab, sc, _ = ops.top_anchors(vb, vs, T)
    tr, an, nt = ops.track_from_anchors(vb, fr, ab, sc)
    frames = torch.randint(0, 256, (F, H, W, 3), generator=g, device=dev, dtype=torch.uint8)
    live = torch.arange(T, device=dev)[None, :] < nt[:, None]
    n = int(((tr[..., 0] == tr[..., 0]) & live[..., None]).sum())        # the present boxes of the 8 frames
    buf = torch.empty((n, 3, S, S), dtype=torch.float32, device=dev)
    nbytes = buf.numel() * 4
    r = rounds([("tubelet_patches", lambda: ops.tubelet_patches(frames, tr, nt, (0, F), n, crop_size=S, padding=PAD, mean=mean_t, sync=False)),
                ("fill", lambda: buf.fill_(1.0))], a)
    rates(r, "tubelet_patches", nbytes)
    r["output_bytes"] = nbytes
    r["windows"] = n
    res["c_tubelets_8_frames"] = r
    print(json.dumps(res))


if __name__ == "__main__":
    main()
