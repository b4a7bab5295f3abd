#!/usr/bin/env python3
"""The Fast R-CNN box decode on the device (ops.decode_boxes / det_nms_volume_deltas / tubelet_dets / dets_as_tracks):
  python devtools/bench_decode.py [--reps R] [--warmup W]
Two shapes of a head's output, identical inputs for every leg:
  c2   F = 8 frames, B = 10 000 proposals, K = 201 columns, topk 100
  vid  F = 30 frames, B = 300 proposals, K = 31 columns, topk 100
Legs:
  fused          det_nms_volume_deltas: selection on the scores, decode of the selected boxes at the gather
  decode_nms     decode_boxes + det_nms_volume: the full [F,B,K,4] tensor written and read back
  torch_nms      an elementwise float64 torch decode (the host functions' arithmetic, torch.exp) + det_nms_volume.  Not the
                 same bits as the rule (another exponential); a comparator, never the code under test
  nms_alone      det_nms_volume on boxes decoded beforehand: the floor
  decode_alone   decode_boxes, with the TB/s of its reads and writes
Also tubelet_dets on 15 890 rows (200 classes x 10 tubelets x 8 frames, K = 201) and dets_as_tracks of the c2 result, each
next to a ``fill_`` of its outputs.
Per leg: HIP-event time of the enqueued work, median [min .. max] of R calls after W warm-up calls; the legs are timed
alternately, twice, so the spread of each shows.  No ratio is a pass condition.  Prints one JSON line."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import torch

from bench_patches import rounds
from vdetlib_amd import ops

IM = (720, 1280)


def head_output(gen, F, B, K, dev):
    H, W = IM
    x1 = torch.rand(F, B, generator=gen, device=dev) * (W - 60)
    y1 = torch.rand(F, B, generator=gen, device=dev) * (H - 60)
    w = 20 + torch.rand(F, B, generator=gen, device=dev) * 300
    h = 20 + torch.rand(F, B, generator=gen, device=dev) * 300
    rois = torch.stack([x1, y1, torch.minimum(x1 + w, torch.tensor(W - 1.0, device=dev)),
                        torch.minimum(y1 + h, torch.tensor(H - 1.0, device=dev))], -1).contiguous()
    scores = torch.rand(F, B, K, generator=gen, device=dev)
    deltas = torch.randn(F, B, 4 * K, generator=gen, device=dev) * 0.2
    return rois, scores, deltas


def torch_decode(rois, deltas, K):
    r, d = rois.double(), deltas.double().view(rois.shape[0], rois.shape[1], K, 4)
    w = (r[..., 2] - r[..., 0] + 1e-14)[..., None]
    h = (r[..., 3] - r[..., 1] + 1e-14)[..., None]
    cx, cy = r[..., 0, None] + 0.5 * w, r[..., 1, None] + 0.5 * h
    pcx, pcy = d[..., 0] * w + cx, d[..., 1] * h + cy
    pw, ph = torch.exp(d[..., 2]) * w, torch.exp(d[..., 3]) * h
    out = torch.stack([(pcx - 0.5 * pw).clamp(0, IM[1] - 1), (pcy - 0.5 * ph).clamp(0, IM[0] - 1),
                       (pcx + 0.5 * pw).clamp(0, IM[1] - 1), (pcy + 0.5 * ph).clamp(0, IM[0] - 1)], -1)
    return out.float()


def main():
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup, "im_size": IM}
    gen = torch.Generator(device=dev).manual_seed(2029)
    last = None
    for name, F, B, K, topk in (("c2", 8, 10000, 201, 100), ("vid", 30, 300, 31, 100)):
        rois, scores, deltas = head_output(gen, F, B, K, dev)
        boxes = ops.decode_boxes(rois, deltas, IM)
        kw = dict(score_thresh=0.05, topk=topk, nms_thresh=0.3, sync=False)
        fused = ops.det_nms_volume_deltas(rois, scores, deltas, IM, **dict(kw, sync=True))
        plain = ops.det_nms_volume(boxes, scores, **dict(kw, sync=True))
        equal = all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(fused, plain))
        td = torch_decode(rois, deltas, K)
        legs = [("fused", lambda: ops.det_nms_volume_deltas(rois, scores, deltas, IM, **kw)),
                ("decode_nms", lambda: ops.det_nms_volume(ops.decode_boxes(rois, deltas, IM, sync=False), scores, **kw)),
                ("torch_nms", lambda: ops.det_nms_volume(torch_decode(rois, deltas, K), scores, **kw)),
                ("nms_alone", lambda: ops.det_nms_volume(boxes, scores, **kw)),
                ("decode_alone", lambda: ops.decode_boxes(rois, deltas, IM, sync=False))]
        r = rounds(legs, a)
        nbytes = deltas.numel() * 4 + boxes.numel() * 4 + rois.numel() * 4
        for rnd, v in r["decode_alone"].items():
            v["TB_s"] = nbytes / (v["median"] * 1e-3) / 1e12
        r.update(shape=[F, B, K], topk=topk, fused_equals_decode_then_nms=bool(equal), decode_bytes=nbytes,
                 gather_bytes_at_most=F * K * topk * 32,
                 torch_decode_elements_differing_from_rule=int((td != boxes).sum()), elements=boxes.numel())
        res[name] = r
        if name == "c2":
            last = fused
        del boxes, td, legs, plain
        print(name, "timed", file=sys.stderr, flush=True)

    # dets_as_tracks of the c2 result
    dets, sel, _, keep, kcnt = last
    out = ops.dets_as_tracks(dets, sel, keep, kcnt)
    bufs = [torch.empty_like(out[k]) for k in ("tracks", "score", "src", "cnt", "ntracks")]

    def fill(bufs=bufs):
        for b in bufs:
            b.fill_(1)
    r = rounds([("dets_as_tracks", lambda: ops.dets_as_tracks(dets, sel, keep, kcnt, sync=False)), ("fill", fill)], a)
    r["output_bytes"] = sum(b.numel() * b.element_size() for b in bufs)
    res["dets_as_tracks_c2"] = r

    # tubelet_dets on 15 890 rows
    C, T, F, K, N = 200, 10, 8, 201, 15890
    pick = torch.randperm(C * T * F, generator=gen, device=dev)[:N].sort().values
    slot = torch.stack([pick // (T * F), (pick // F) % T, pick % F], 1).int().contiguous()
    tr = torch.cat([head_output(gen, C, T * F, 1, dev)[0].view(C, T, F, 4), torch.rand(C, T, F, 1, generator=gen, device=dev)], -1).contiguous()
    sc = torch.rand(N, K, generator=gen, device=dev)
    dl = torch.randn(N, 4 * K, generator=gen, device=dev) * 0.2
    cnt = torch.tensor([N], dtype=torch.int32, device=dev)
    o = ops.tubelet_dets(sc, dl, tr, slot, cnt, IM)
    bufs2 = [torch.empty_like(o['det']), torch.empty_like(o['tboxes'])]

    def fill2(bufs=bufs2):
        for b in bufs:
            b.fill_(1.0)
    r = rounds([("tubelet_dets", lambda: ops.tubelet_dets(sc, dl, tr, slot, cnt, IM, out=o, sync=False)), ("fill", fill2)], a)
    r["rows"] = N
    r["output_bytes"] = sum(b.numel() * b.element_size() for b in bufs2)
    res["tubelet_dets"] = r
    print(json.dumps(res))


if __name__ == "__main__":
    main()
