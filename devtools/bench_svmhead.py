#!/usr/bin/env python3
"""The SVM head of the CNN scorers on the device (ops.svm_head) at three shapes:
  python devtools/bench_svmhead.py [--reps R] [--warmup W] [--scale-down D]
 a  15 890 boxes x 33 windows x 1024 float32 features, 200 classes, f64 model: one c2 tubelet_patches chunk of 8 frames;
 b  the same features in bfloat16;
 c  582 000 boxes x 1 window x 1024 float32 (rcnn_scoring over the tubelets of a whole c2 video).
(--scale-down D divides the box counts by D, for a quick look.)
Comparators, timed in the same run and never the code under test:
 read_floor  ``torch.sum(features, 1)`` on the same tensor: one read of the features, the floor the call is sized by;
 torch_full  the torch formulation ``(features.double()*scale) @ W + B``, a gather of the class column, ``view(N,G).max(1)``:
             the full 200-column product through the vendor GEMM;
 host        the present route -- download, image_det.svm_scores (all 200 columns on a private context), numpy max -- timed on
             a slice of 4 096 windows and EXTRAPOLATED linearly to the call's count.
Per leg: HIP-event time of the enqueued work, median [min .. max] of R calls after W warm-up calls; the legs are timed
alternately, twice, so the spread of each shows.  Prints one JSON line."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from vdetlib_amd import ops
from vdetlib_amd.vdet.image_det import svm_scores

K, M = 1024, 200


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


def main():
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--scale-down", type=int, default=1)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup, "K": K, "classes": M}
    gen = torch.Generator(device=dev).manual_seed(2028)
    rng = np.random.RandomState(2028)
    model_np = {'W': rng.uniform(-1, 1, (K, M)), 'B': rng.uniform(-0.5, 0.5, (1, M)), 'feat_norm_mean': np.float64(19.6)}
    model = {'W': torch.from_numpy(model_np['W']).to(dev), 'B': torch.from_numpy(model_np['B'].reshape(-1)).to(dev),
             'feat_norm_mean': model_np['feat_norm_mean']}
    scale = float(20. / model_np['feat_norm_mean'])
    for key, N, G, dt in (("a_f32_33_windows", 15890, 33, torch.float32), ("b_bf16_33_windows", 15890, 33, torch.bfloat16),
                          ("c_f32_1_window", 582000, 1, torch.float32)):
        N = max(1, N // a.scale_down)
        C, T = M, 10
        F = (N + C * T - 1) // (C * T)
        feat = torch.randn((N * G, K), generator=gen, device=dev, dtype=torch.float32).to(dt)
        flat = torch.randperm(C * T * F, generator=gen, device=dev)[:N].sort().values
        slot = torch.stack([flat // (T * F), (flat // F) % T, flat % F], 1).to(torch.int32)
        slot = slot[torch.argsort(slot[:, 2], stable=True)].contiguous()            # frames outer, as the patch calls give them
        cols = torch.randperm(M, generator=gen, device=dev).to(torch.int32)
        sboxes = torch.rand((N, G, 4), generator=gen, device=dev, dtype=torch.float64)
        out = ops.svm_head(feat, model, group=G, slot=slot, shape=(C, T, F), cols=cols, sboxes=sboxes)
        colw = cols.long()[slot[:, 0].long()].repeat_interleave(G)

        def torch_full():
            s = (feat.double() * scale) @ model['W'] + model['B']
            s = s.gather(1, colw[:, None]).view(N, G)
            return s.max(1)
        ref = torch_full()
        r = {"windows": N * G, "boxes": N, "feature_bytes": feat.numel() * feat.element_size(),
             "max_abs_diff_to_torch_full": float((ref.values - out['score']).abs().max()),
             "winners_equal_to_torch_full": bool(torch.equal(ref.indices, out['arg_flat'].long()))}
        del ref
        # the present route on a slice (extrapolated)
        n_host = min(4096 // G * G, N * G)
        t0 = time.perf_counter()
        h = feat[:n_host].float().cpu().numpy()
        s = svm_scores(h, model_np)
        hc = colw[:n_host].cpu().numpy()
        s[np.arange(n_host), hc].reshape(-1, G).max(1)
        r["host_route_ms_EXTRAPOLATED_from_%d_windows" % n_host] = (time.perf_counter() - t0) * 1e3 / n_host * (N * G)
        hold = dict(out)
        legs = [("svm_head", lambda: ops.svm_head(feat, model, group=G, slot=slot, cols=cols, sboxes=sboxes, out=hold, sync=False)),
                ("read_floor", lambda: torch.sum(feat, 1)),
                ("torch_full", torch_full)]
        r.update(rounds(legs, a))
        for rnd in ("round1", "round2"):
            for name in ("svm_head", "read_floor", "torch_full"):
                r[name][rnd]["feature_TB_s"] = r["feature_bytes"] / (r[name][rnd]["median"] * 1e-3) / 1e12
            r["svm_head"][rnd]["ratio_to_read_floor"] = r["svm_head"][rnd]["median"] / r["read_floor"][rnd]["median"]
            r["svm_head"][rnd]["speedup_over_torch_full"] = r["torch_full"][rnd]["median"] / r["svm_head"][rnd]["median"]
        res[key] = r
        del feat, slot, sboxes, out, hold, legs, colw
        torch.cuda.empty_cache()
        print(key, "timed", file=sys.stderr, flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
