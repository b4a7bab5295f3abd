#!/usr/bin/env python3
"""The device TCN with WIDE inputs (ops.tcn_tracks(wide=...), csrc/tcn_kernels.hpp: tcn_wide_layer_kernel) on the tubelets of
one c2 video (300 frames x 10 000 boxes x 200 classes, 10 tracks per class) and of the 64-video VID-shaped batch:
  python devtools/bench_tcn_wide.py [--reps R] [--warmup W] [--host-tubelets N]
Legs, HIP-event ms, median [min .. max] of R calls after W warm-up calls; the legs are run in turn and the whole turn twice
(``pass1`` / ``pass2``), so a drift of the machine shows as a difference between the passes:
  wide_as          all_scores (200) + det_scores, net (64, 64), K = 5
  wide_as_feats    all_scores + det_scores + feats (1024), f32 rows; ``_bf16``: the same rows stored as bfloat16
  narrow           the four one-channel inputs on the same tubelets (the call without wide=)
  read_floor       torch.sum(rows, -1) over the same row tensors: every row read once
  conv1d           torch.nn.functional.conv1d of layer 0 on a channel-major copy of ALL slots as hole-free series (the vendor
                   route; not bit-equal), ``permute``: making that copy
  vid64_wide_as    tcn_tracks_batch over the 64-video batch with all_scores
and, timed once on the host: TCNNet.forward_series fed host-transposed series of the first N tubelets, EXTRAPOLATED to all.
Beside the times: the un-fused multiply-adds of layer 0 (boxes x cout0 x Cin x K) and the rate they give.  One JSON line."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import bench
from vdetlib_amd import ops
from vdetlib_amd.vdet.tcn import TCNNet


def stats(ts):
    ts = np.asarray(ts, dtype=np.float64)
    return {"median": round(float(np.median(ts)), 4), "min": round(float(ts.min()), 4), "max": round(float(ts.max()), 4)}


def event_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return stats(out)


def main():
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-tubelets", type=int, default=16)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup}
    hidden, K = (64, 64), 5
    F, B, C = 300, 10000, 200
    boxes, scores = bench.synth_video_cuda(torch, 2000, F, B, C, dev)
    tr, an, nt = ops.track_volume(boxes, scores, nms_thres=0.3, thres=0.0, max_tracks=10, link_thres=0.5)
    det, pooled, ob = ops.rescore_tracks(tr, nt, boxes, scores, overlap_thres=0.7, window=3)
    del boxes, scores
    T = tr.shape[1]
    has = ~torch.isnan(tr[..., 0]) & (torch.arange(T, device=dev)[None, :, None] < nt[:, None, None])
    nbox, ntub = int(has.sum()), int(nt.sum())
    g = torch.Generator(device=dev).manual_seed(3)
    rows_as = torch.randn((C, T, F, 200), generator=g, device=dev)
    rows_ft = torch.randn((C, T, F, 1024), generator=g, device=dev)
    rows_as16, rows_ft16 = rows_as.bfloat16(), rows_ft.bfloat16()
    D = ('det_scores', 1)
    net_as = TCNNet.random([('all_scores', 200), D], hidden=hidden, kernel=K, seed=1)
    net_af = TCNNet.random([('all_scores', 200), D, ('feats', 1024)], hidden=hidden, kernel=K, seed=1)
    net_nr = TCNNet.random([(n, 1) for n in ('det_scores', 'track_scores', 'anchors', 'abs_anchors')], hidden=hidden, kernel=K, seed=1)
    w0 = torch.from_numpy(net_af.layers[0][0]).to(dev)
    b0 = torch.from_numpy(net_af.layers[0][1]).to(dev)
    xcm = [None]

    def permute():
        xcm[0] = torch.cat([rows_as.view(C * T, F, 200), det.float().view(C * T, F, 1), rows_ft.view(C * T, F, 1024)], 2) \
            .permute(0, 2, 1).contiguous()

    vb, vs, off = bench.synth_vid_batch(torch, dev, 64)
    bo = ops.video_batch(vb, vs, off, nms_thres=0.3, thres=0.5, max_tracks=4, link_thres=0.5, cap=300, overlap_thres=0.7, window=3)
    Cv, Tv, Ft = bo['tracks'][0].shape[0], bo['tracks'][0].shape[1], int(off[-1])
    rows_v = torch.randn((Cv * Tv * Ft, 200), generator=g, device=dev)
    hasv = [~torch.isnan(t[..., 0]) & (torch.arange(Tv, device=dev)[None, :, None] < n[:, None, None])
            for t, n in zip(bo['tracks'], bo['ntracks'])]
    nbox_v = int(sum(int(h.sum()) for h in hasv))
    permute()
    legs = [
        ("wide_as", lambda: ops.tcn_tracks(net_as, tr, nt, an, det, sync=False, wide={'all_scores': rows_as})),
        ("wide_as_feats", lambda: ops.tcn_tracks(net_af, tr, nt, an, det, sync=False, wide={'all_scores': rows_as, 'feats': rows_ft})),
        ("wide_as_feats_bf16", lambda: ops.tcn_tracks(net_af, tr, nt, an, det, sync=False,
                                                      wide={'all_scores': rows_as16, 'feats': rows_ft16})),
        ("narrow", lambda: ops.tcn_tracks(net_nr, tr, nt, an, det, sync=False)),
        ("read_floor_as", lambda: torch.sum(rows_as, -1)),
        ("read_floor_as_feats", lambda: (torch.sum(rows_as, -1), torch.sum(rows_ft, -1))),
        ("read_floor_as_feats_bf16", lambda: (torch.sum(rows_as16, -1), torch.sum(rows_ft16, -1))),
        ("permute", permute),
        ("conv1d", lambda: torch.nn.functional.conv1d(xcm[0], w0, b0, padding=K // 2)),
        ("vid64_wide_as", lambda: ops.tcn_tracks_batch(net_as, bo, sync=False, wide={'all_scores': rows_v})),
        ("vid64_read_floor", lambda: torch.sum(rows_v, -1)),
    ]
    for p in ("pass1", "pass2"):
        res[p] = {name: event_ms(fn, a.reps, a.warmup) for name, fn in legs}
    # the arithmetic of layer 0: un-fused multiply-adds (one multiply and one add each), and the bytes of the rows
    cout0 = hidden[0]
    for name, cin, nb, rb in (("wide_as", 201, nbox, 200 * 4), ("wide_as_feats", 1225, nbox, 1224 * 4),
                              ("wide_as_feats_bf16", 1225, nbox, 1224 * 2), ("vid64_wide_as", 201, nbox_v, 200 * 4)):
        macs = nb * cout0 * cin * K
        ms = min(res["pass1"][name]["median"], res["pass2"][name]["median"])
        res[name + "_arith"] = {"boxes": nb, "layer0_macs": macs, "tera_macs_per_s": round(macs / ms / 1e9, 3),
                                "row_bytes_read": nb * rb, "row_GB_per_s": round(nb * rb / ms / 1e6, 1)}
    res["c2"] = {"tubelets": ntub, "boxes": nbox, "slots": C * T * F}
    res["vid64"] = {"tubelets": int(bo['ntracks'].sum()), "boxes": nbox_v, "slots": Cv * Tv * Ft}
    # the host route: host-transposed series of a few tubelets through forward_series, extrapolated by boxes
    n_host = max(1, min(a.host_tubelets, ntub))
    hh = has.cpu().numpy()
    picks = [(c, t) for c in range(C) for t in range(int(nt[c]))][:n_host]
    t0 = time.perf_counter()
    series, hb = [], 0
    for c, t in picks:
        fr = np.nonzero(hh[c, t])[0]
        x = np.concatenate([rows_as[c, t].cpu().numpy()[fr].T, det[c, t].cpu().numpy()[fr][None].astype(np.float32),
                            rows_ft[c, t].cpu().numpy()[fr].T], 0)
        series.append(np.ascontiguousarray(x))
        hb += len(fr)
    t_build = time.perf_counter() - t0
    t0 = time.perf_counter()
    net_af.forward_series(series)
    t_fwd = time.perf_counter() - t0
    res["host_forward_series"] = {"tubelets_timed": n_host, "boxes_timed": hb, "build_s": round(t_build, 3), "forward_s": round(t_fwd, 3),
                                  "extrapolated_s_all_boxes": round((t_build + t_fwd) * nbox / max(hb, 1), 2)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
