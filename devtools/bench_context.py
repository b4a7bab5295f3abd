#!/usr/bin/env python3
"""Multi-context suppression (ops.context_classes, ops.suppress_context) on the c2 detection volume
(300 frames x 10 000 boxes x 200 classes, bench.py's generator: BASELINE.md section 3) and on the 64-video VID-shape batch:
  python devtools/bench_context.py [--reps R] [--warmup W] [--frames F] [--boxes B] [--classes C] [--videos V] [--skip-torch]
Legs, per volume:
  context_classes            as the data sends it (vdet_query 13 tells how many full reads that was)
  context_classes_full_read  a context created under VDET_CTX_RECORDS=0: the four-read form
  torch_sum                  torch.sum(scores): the floor of ONE read
  suppress_context           out of place, and in place
  torch_clone                scores.clone(): the floor of one read + one write
  torch_formulation          torch.topk(scores.flatten(), k) for the threshold, (scores >= t).sum((0, 1)) for the hits,
                             scores - table[:, None, :] for the suppression; on the batch a loop over the videos.  Its results
                             are checked against the device's (the subtraction differs from the rule only on NaN, absent here).
The c2 volume is measured with uniform scores (the generator's default: the top bin of the first digit holds an eighth of them)
and with normal ones (kind="randn").  HIP-event ms, median [min .. max] of R calls after W warm-up calls; the legs alternate and
the whole turn runs twice, so the spread of each shows.  Prints one JSON line."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "devtools"))
import torch

RATIO, PENALTY = 0.0003, 0.4


def torch_one(s, ratio):
    """one video in torch -> (thresh, hits [C], suppressed scores)"""
    n = s.numel()                                    # (no NaN in the generators' scores: every score is a candidate)
    k = min(n, max(1, int(ratio * n)))
    t = torch.topk(s.flatten(), k, sorted=False).values.min()
    hits = (s >= t).sum((0, 1))
    table = torch.where(hits >= 1, 0.0, PENALTY).to(torch.float32)
    return t, hits, s - table[None, None, :]


def measure(name, scores, off, a, res, ops, _lib, dev):
    from bench_tcn import device_times
    from context_cases import records_off_context
    cf = records_off_context(dev.index)
    cd = _lib.get_context(dev.index)
    kw = dict(ratio=RATIO, frame_off=off)
    t, n, hits, high = ops.context_classes(scores, **kw)
    reads = cd.query(13)
    tf = ops.context_classes(scores, ctx=cf, **kw)
    assert cf.query(13) == 4
    for x, y in zip((t, n, hits, high), tf):
        assert torch.equal(x, y), "the paths disagree"
    r = res[name] = {"shape": list(scores.shape), "gbytes": round(scores.numel() * 4 / 1e9, 3), "videos": 1 if off is None else len(off) - 1,
                     "full_reads_as_the_data_sends_it": reads, "n": n.reshape(-1)[:4].tolist(),
                     "high_classes": high.reshape(-1, high.shape[-1]).sum(1)[:4].tolist()}
    vids = [(0, scores.shape[0])] if off is None else list(zip(off[:-1].tolist(), off[1:].tolist()))

    def torch_all(sync):
        return [torch_one(scores[x:y], RATIO) for x, y in vids]

    if not a.skip_torch:
        out = ops.suppress_context(scores, high, PENALTY, frame_off=off)
        for v, ((x, y), (tt, th, ts)) in enumerate(zip(vids, torch_all(True))):
            assert float(tt) == float(t.reshape(-1)[v]) and torch.equal(th.to(torch.int32), hits.reshape(-1, hits.shape[-1])[v])
            assert torch.equal(ts, out[x:y]), "torch's suppression differs"
        del out, tt, th, ts
    buf = torch.empty_like(scores)
    legs = [("context_classes", lambda s: ops.context_classes(scores, sync=s, **kw), a.reps),
            ("context_classes_full_read", lambda s: ops.context_classes(scores, sync=s, ctx=cf, **kw), a.reps),
            ("torch_sum", lambda s: torch.sum(scores), a.reps),
            ("suppress_context", lambda s: ops.suppress_context(scores, high, PENALTY, frame_off=off, out=buf, sync=s), a.reps),
            ("suppress_context_in_place", lambda s: ops.suppress_context(buf, high, 0.0, frame_off=off, out=buf, sync=s), a.reps),
            ("torch_clone", lambda s: scores.clone(), a.reps)]
    if not a.skip_torch:
        legs.append(("torch_formulation", torch_all, max(a.reps // 10, 2)))
    for leg, _, _ in legs:
        r[leg] = {}
    for rnd in ("round1", "round2"):
        for leg, fn, reps in legs:
            r[leg][rnd] = dict(zip(("event_ms", "wall_ms"), device_times(fn, reps, min(a.warmup, reps))))
    med = lambda leg: r[leg]["round1"]["event_ms"]["median"]
    for leg in ("context_classes", "context_classes_full_read"):
        r[leg]["over_torch_sum"] = round(med(leg) / med("torch_sum"), 2)
    for leg in ("suppress_context", "suppress_context_in_place"):
        r[leg]["over_torch_clone"] = round(med(leg) / med("torch_clone"), 2)
    r["torch_sum"]["gb_per_s"] = round(scores.numel() * 4 / med("torch_sum") / 1e6, 1)
    if not a.skip_torch:
        r["torch_formulation"]["over_both_calls"] = round(med("torch_formulation") / (med("context_classes") + med("suppress_context")), 1)
    cf.close()
    del buf


def main():
    import argparse
    import bench
    from vdetlib_amd import _lib, ops
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--boxes", type=int, default=10000)
    ap.add_argument("--classes", type=int, default=200)
    ap.add_argument("--videos", type=int, default=64)
    ap.add_argument("--skip-torch", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup, "ratio": RATIO, "penalty": PENALTY}
    for kind in ("rand", "randn"):
        scores = bench.synth_video_cuda(torch, 2000, a.frames, a.boxes, a.classes, dev, kind=kind)[1]
        measure("c2_" + ("uniform" if kind == "rand" else "normal"), scores, None, a, res, ops, _lib, dev)
        del scores
        torch.cuda.empty_cache()
    _, scores, off = bench.synth_vid_batch(torch, dev, a.videos, 300, 30)[:3]
    measure("vid_batch", scores, off, a, res, ops, _lib, dev)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
