#!/usr/bin/env python3
"""RoI pooling on the device (ops.roi_pool / ops.tubelet_rois) at two shapes, float32 and bfloat16, 'max' and 'align':
  python devtools/bench_roipool.py [--reps R] [--warmup W] [--boxes N]
 a  one 720 x 1280 frame at stride 16 -- features [1,512,45,80] -- and --boxes (default 2 000) boxes of the c2 generator, 7 x 7;
 c  ops.tubelet_rois over 8 frames of c2 anchor-route tubelets (200 classes x 10: the 15 890 boxes of bench_patches.py), features
    [8,512,45,80], cap = the present count.
Comparators, timed in the same run and never the code under test:
 fill       ``fill_`` of a tensor of the output's size and dtype: the write floor;
 windows    the BYTES the R-CNN windows route writes for the same boxes (3 x 224 x 224 float32 per box; its time is
            devtools/bench_patches.py's), next to the bytes pooled here;
 torch_loop a per-RoI ``adaptive_max_pool2d`` of the rounded cell box on 32 RoIs, EXTRAPOLATED linearly to the call's count (a).
            Not the same rule (its bin edges are integer arithmetic) and not bit-equal.
Per leg: HIP-event time of the enqueued work, median [min .. max] of R calls after W warm-up calls; the legs are timed
alternately, twice, so the spread of each shows.  No ratio is a pass condition.  Prints one JSON line."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import torch

import bench
import roipool_spec
from bench_patches import rounds
from vdetlib_amd import ops

H, W, STRIDE, K, POOLED = 720, 1280, 16, 512, (7, 7)
MODES = (("max", dict(mode='max')), ("align", dict(mode='align', sampling=2)))


def rates(res, name, nbytes):
    for rnd, r in res[name].items():
        r["out_TB_s"] = nbytes / (r["median"] * 1e-3) / 1e12
        r["ratio_to_fill"] = res["fill"][rnd]["median"] / r["median"]


def main():
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--boxes", type=int, default=2000)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    Hf, Wf = H // STRIDE, W // STRIDE
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup, "pooled": POOLED, "features": [K, Hf, Wf]}
    g = torch.Generator(device=dev).manual_seed(2028)
    N = a.boxes
    boxes = bench.synth_video_cuda(torch, 7, 1, N, 1, dev)[0][0].contiguous()
    feat32 = torch.randn((1, K, Hf, Wf), generator=g, device=dev)

    # the device against the spec on 20 boxes and 8 channels
    small = feat32[:, :8].contiguous()
    res["equal_to_spec_on_20"] = {}
    for name, kw in MODES:
        got = ops.roi_pool(small, boxes[:20], spatial_scale=1. / STRIDE, pooled=POOLED, **kw)
        wp, wok = roipool_spec.roi_pool(small.cpu().numpy(), boxes[:20].cpu().numpy(), None, 1. / STRIDE, POOLED, 1.0, **kw)
        res["equal_to_spec_on_20"][name] = bool(torch.equal(got['pooled'].cpu(), torch.from_numpy(wp)) and
                                                torch.equal(got['ok'].cpu(), torch.from_numpy(wok)))

    # a: one frame, N boxes
    for dname, dt in (("f32", torch.float32), ("bf16", torch.bfloat16)):
        feat = feat32.to(dt)
        buf = torch.empty((N, K) + POOLED, dtype=dt, device=dev)
        nbytes = buf.numel() * buf.element_size()
        legs = [(name, lambda kw=kw: ops.roi_pool(feat, boxes, spatial_scale=1. / STRIDE, pooled=POOLED, sync=False, **kw)) for name, kw in MODES]
        legs.append(("fill", lambda buf=buf: buf.fill_(1.0)))
        if dt == torch.float32:
            cells = torch.round(boxes[:32] / STRIDE).long().cpu().tolist()

            def torch_loop():
                for x1, y1, x2, y2 in cells:
                    ys, xs = min(max(y1, 0), Hf - 1), min(max(x1, 0), Wf - 1)
                    crop = feat[0, :, ys:max(min(y2, Hf - 1), ys) + 1, xs:max(min(x2, Wf - 1), xs) + 1]
                    torch.nn.functional.adaptive_max_pool2d(crop, POOLED)
            legs.append(("torch_loop_32_rois", torch_loop))
        r = rounds(legs, a)
        for name, _ in MODES:
            rates(r, name, nbytes)
        if dt == torch.float32:
            r["torch_loop_ms_EXTRAPOLATED_from_32_rois"] = {rnd: v["median"] / 32 * N for rnd, v in r["torch_loop_32_rois"].items()}
        r["output_bytes"] = nbytes
        r["windows_route_bytes_f32"] = N * 3 * 224 * 224 * 4
        r["rois"] = N
        res["a_" + dname] = r
        del buf, legs
        print("a", dname, "timed", file=sys.stderr, flush=True)

    # c: tubelet_rois over 8 frames of c2 anchor-route tubelets
    F, B, C, T = 8, 10000, 200, 10
    gp = torch.Generator(device=dev).manual_seed(2027)       # bench_patches.py's draws, in its order: the same tubelets
    torch.randint(0, 256, (1, H, W, 3), generator=gp, device=dev, dtype=torch.uint8)
    base, _ = bench.synth_video_cuda(torch, 7, 1, B, 1, dev)
    vb = base + 3.0 * torch.arange(F, device=dev, dtype=torch.float32)[:, None, None] + \
        torch.randint(-1, 2, (F, B, 4), generator=gp, device=dev).float()
    vb[..., 2:] = torch.maximum(vb[..., 2:], vb[..., :2] + 4)
    vb = vb.contiguous()
    vs = torch.rand(F, B, C, generator=gp, device=dev)
    fr, ab, sc, _ = ops.top_anchors(vb, vs, T)
    tr, an, nt = ops.track_from_anchors(vb, fr, ab, sc)
    live = torch.arange(T, device=dev)[None, :] < nt[:, None]
    n = int(((tr[..., 0] == tr[..., 0]) & live[..., None]).sum())        # the present boxes of the 8 frames
    feats32 = torch.randn((F, K, Hf, Wf), generator=g, device=dev)
    for dname, dt in (("f32", torch.float32), ("bf16", torch.bfloat16)):
        feats = feats32.to(dt)
        buf = torch.empty((n, K) + POOLED, dtype=dt, device=dev)
        nbytes = buf.numel() * buf.element_size()
        legs = [(name, lambda kw=kw: ops.tubelet_rois(feats, tr, nt, (0, F), n, spatial_scale=1. / STRIDE, pooled=POOLED, sync=False, **kw))
                for name, kw in MODES]
        legs.append(("fill", lambda buf=buf: buf.fill_(1.0)))
        r = rounds(legs, a)
        for name, _ in MODES:
            rates(r, name, nbytes)
        r["output_bytes"] = nbytes
        r["windows_route_bytes_f32"] = n * 3 * 224 * 224 * 4
        r["rois"] = n
        res["c_tubelets_8_frames_" + dname] = r
        del buf, legs, feats
        print("c", dname, "timed", file=sys.stderr, flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
