#!/usr/bin/env python3
"""The RPN proposal layer on the device (ops.rpn_proposals):
  python devtools/bench_proposals.py [--reps R] [--warmup W]
Four shapes of an RPN head's output, 8 frames each, 9 anchors, stride 16, nms 0.7, post_nms_top_n 300, min_size 16, identical
inputs for both legs:
  600x1000     38 x 63 cells (21 546 anchors a frame), pre_nms_top_n 6000
  720x1280     45 x 80 cells (32 400 anchors a frame), pre_nms_top_n 6000
  ... and both with pre_nms_top_n 12000
Legs:
  device   ops.rpn_proposals
  torch    permute to (h,w,a) order + an elementwise float32 decode (torch.exp) + the size filter + torch.topk + gathers +
           ops.nms_volume_ordered over the selected boxes + the gather of the first 300.  A comparator, never the code under
           test: NOT bit-equal to the rule (float32 arithmetic, another exponential, topk's own order among equal scores)
Both legs run on a context set asynchronous (no host wait inside the calls).  Per leg: HIP-event time of the enqueued work,
median [min .. max] of R calls after W warm-up calls; the legs are timed alternately, twice, so the spread of each shows.
``stages_ms`` is the library's own per-stage event timing of one device call (other: decode pass, frame flags and gather;
merge_sort: select and sort; iou_bits / adj_build / walk: the NMS).  No ratio is a pass condition.  Prints one JSON line."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import torch

from bench_patches import rounds
from vdetlib_amd import _lib, ops

F, A, STRIDE, POST, NMS, MIN_SIZE = 8, 9, 16, 300, 0.7, 16.0


def torch_proposals(scores, deltas, anchors32, im_size, pre):
    """the comparator: float32 torch, the existing ordered NMS"""
    Fn, _, Hf, Wf = scores.shape
    H, W = im_size
    dev = scores.device
    s = scores.permute(0, 2, 3, 1).reshape(Fn, -1)
    d = deltas.view(Fn, A, 4, Hf, Wf).permute(0, 3, 4, 1, 2).reshape(Fn, -1, 4)
    sx = torch.arange(Wf, device=dev, dtype=torch.float32) * STRIDE
    sy = torch.arange(Hf, device=dev, dtype=torch.float32) * STRIDE
    shift = torch.stack([sx[None, :].expand(Hf, Wf), sy[:, None].expand(Hf, Wf)] * 2, -1)       # [Hf,Wf,4]
    an = (shift[:, :, None, :] + anchors32[None, None]).reshape(-1, 4)
    w, h = an[:, 2] - an[:, 0] + 1.0, an[:, 3] - an[:, 1] + 1.0
    cx, cy = an[:, 0] + 0.5 * w, an[:, 1] + 0.5 * h
    pcx, pcy = d[..., 0] * w + cx, d[..., 1] * h + cy
    pw, ph = torch.exp(d[..., 2]) * w, torch.exp(d[..., 3]) * h
    boxes = torch.stack([(pcx - 0.5 * pw).clamp(0, W - 1), (pcy - 0.5 * ph).clamp(0, H - 1),
                         (pcx + 0.5 * pw).clamp(0, W - 1), (pcy + 0.5 * ph).clamp(0, H - 1)], -1)
    ok = (boxes[..., 2] - boxes[..., 0] + 1 >= MIN_SIZE) & (boxes[..., 3] - boxes[..., 1] + 1 >= MIN_SIZE)
    top, idx = torch.topk(torch.where(ok, s, torch.full_like(s, -float('inf'))), pre, dim=1)
    cand = torch.gather(boxes, 1, idx[..., None].expand(-1, -1, 4)).contiguous()
    order = torch.arange(pre, device=dev, dtype=torch.int16)[None, None].expand(Fn, 1, pre).contiguous()
    ncand = (top > -float('inf')).sum(1, dtype=torch.int32)[:, None].contiguous()
    keep, cnt = ops.nms_volume_ordered(cand, order, ncand, NMS, cap=pre, pad=False)
    k = keep[:, 0, :POST].long().clamp(min=0)
    return torch.gather(cand, 1, k[..., None].expand(-1, -1, 4)), torch.gather(top, 1, k), cnt.clamp(max=POST)


def main():
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    ctx = _lib.get_context(0)
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup, "frames": F, "anchors": A}
    gen = torch.Generator(device=dev).manual_seed(2030)
    anchors = ops.generate_anchors()
    anchors32 = torch.from_numpy(anchors).float().to(dev)
    for (H, W) in ((600, 1000), (720, 1280)):
        Hf, Wf = -(-H // STRIDE), -(-W // STRIDE)
        cls = torch.randn(F, 2 * A, Hf, Wf, generator=gen, device=dev)
        scores = cls[:, A:]                                   # the strided foreground half, as a net hands it over
        deltas = torch.randn(F, 4 * A, Hf, Wf, generator=gen, device=dev) * 0.2
        for pre in (6000, 12000):
            kw = dict(stride=STRIDE, pre_nms_top_n=pre, post_nms_top_n=POST, nms_thresh=NMS, min_size=MIN_SIZE)
            first = ops.rpn_proposals(scores, deltas, anchors, (H, W), return_candidates=True, **kw)     # (sizes the NMS's pool)
            tr, ts, tc = torch_proposals(scores, deltas, anchors32, (H, W), pre)
            ctx.set_timing(True)
            ops.rpn_proposals(scores, deltas, anchors, (H, W), **kw)
            stages = {k: v for k, v in ctx.last_timing().items() if v[1]}
            ctx.set_timing(False)
            ctx.set_async(True)
            try:
                legs = [("device", lambda: ops.rpn_proposals(scores, deltas, anchors, (H, W), sync=False, **kw)),
                        ("torch", lambda: torch_proposals(scores, deltas, anchors32, (H, W), pre))]
                r = rounds(legs, a)
                ctx.sync()
            finally:
                ctx.set_async(False)
            r.update(shape=[F, A, Hf, Wf], anchors_per_frame=A * Hf * Wf, pre_nms_top_n=pre, stages_ms=stages,
                     candidates=first['cand_cnt'].tolist(), proposals=first['count'].tolist(),
                     torch_proposals=tc.view(-1).tolist())
            res["%dx%d_pre%d" % (H, W, pre)] = r
            print(H, W, pre, "timed", file=sys.stderr, flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
