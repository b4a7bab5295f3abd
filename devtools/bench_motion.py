#!/usr/bin/env python3
"""Motion-guided propagation (ops.motion_field, ops.propagate_detections) on the 300-frame 720 x 1280
panning video of devtools/bench_pixtrack.py and the c2 detection volume (10 000 boxes x 200 classes a frame):
  python devtools/bench_motion.py [--reps R] [--warmup W] [--frames F] [--boxes B] [--classes C]
Legs:
 (a) ops.motion_field at block 16 / radius 8 and at block 8 / radius 4, against ops.luma_integral of the same video, which reads
     the same images once (the matching kernel reads every frame as a tile and as two regions: at least twice);
 (b) ONE frame pair of block 16 / radius 8 as a torch formulation -- replicate padding, one shifted |difference| and one
     ``unfold`` block sum per candidate, the packed key min-reduced -- whose winners are checked against tests/motion_spec.py;
     its time for the whole video is EXTRAPOLATED: one pair times 2 * (F - 1);
 (c) ops.propagate_detections from the c2 keep lists (ops.nms_volume at 0.3), top 100, reach 3, against torch.full of its three
     output tensors: the floor of writing them once;
 (d) ops.nms_tracks of the result with the same still-image source.
HIP-event ms, median [min .. max] of R calls after W warm-up calls; the legs of a group alternate and the whole turn runs twice,
so the spread of each shows.  Prints one JSON line."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "devtools"))
import torch

TOP, REACH, THRESH = 100, 3, 0.3


def luma_of(images):
    w = torch.tensor([29, 150, 77], device=images.device, dtype=torch.int32)
    return (((images.to(torch.int32) * w).sum(-1) + 128) >> 8).to(torch.uint8)


def torch_pair(lf, lg, P, R):
    """the field of ONE frame pair in torch: luma planes uint8 [H,W] -> (field int64 [Hb,Wb,2], cost int64 [Hb,Wb])"""
    H, W = lf.shape
    Hb, Wb = -(-H // P), -(-W // P)
    pad = torch.nn.functional.pad
    tm = pad(lf[None, None].float(), (0, Wb * P - W, 0, Hb * P - H), mode='replicate')
    rg = pad(lg[None, None].float(), (R, Wb * P - W + R, R, Hb * P - H + R), mode='replicate')
    best = None
    for cy in range(2 * R + 1):
        for cx in range(2 * R + 1):
            diff = (tm - rg[:, :, cy:cy + Hb * P, cx:cx + Wb * P]).abs()
            sad = torch.nn.functional.unfold(diff, P, stride=P).sum(1).to(torch.int64).view(Hb, Wb)      # exact: <= 255 * 32 * 32
            key = (sad << 32) | (((cy - R) ** 2 + (cx - R) ** 2) << 16) | (cy << 8) | cx
            best = key if best is None else torch.minimum(best, key)
    return torch.stack([(best & 0xFF) - R, ((best >> 8) & 0xFF) - R], -1), best >> 32


def main():
    import argparse
    import bench
    import motion_spec as ms
    from bench_pixtrack import panning_video
    from bench_tcn import device_times
    from vdetlib_amd import ops
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--boxes", type=int, default=10000)
    ap.add_argument("--classes", type=int, default=200)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    F, H, W, C = a.frames, 720, 1280, a.classes
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup, "frames": F, "image": [H, W],
           "boxes": a.boxes, "classes": C, "top": TOP, "reach": REACH}
    both = lambda fn, reps=a.reps: dict(zip(("event_ms", "wall_ms"), device_times(fn, reps, a.warmup)))
    med = lambda leg: leg["round1"]["event_ms"]["median"]
    images = panning_video(dev, F, H, W)

    # (a) + (b)
    luma = luma_of(images[:2])
    tf, tc = torch_pair(luma[0], luma[1], 16, 8)
    wf, wc = ms.match_pair(luma[0].cpu().numpy(), luma[1].cpu().numpy(), 16, 8)
    assert (tf.cpu().numpy() == wf).all() and (tc.cpu().numpy() == wc).all(), "the torch formulation is not the spec's field"
    m = ops.motion_field(images, 16, 8)
    assert (m['field'][0, 0].cpu().numpy() == wf).all() and (m['cost'][0, 0].cpu().numpy() == wc).all()
    res["pan_found"] = {"block16_interior_vectors_equal_to_the_pan": float((m['field'][0, :-1, 1:-1, 1:-1] ==
                                                                          torch.tensor([-2, -1], device=dev, dtype=torch.int16)).all(-1).double().mean())}
    legs = [("a_motion_field_p16_r8", lambda s: ops.motion_field(images, 16, 8, sync=s)),
            ("a_motion_field_p8_r4", lambda s: ops.motion_field(images, 8, 4, sync=s)),
            ("a_luma_integral", lambda s: ops.luma_integral(images, sync=s)),
            ("b_torch_unfold_one_pair_p16_r8", lambda s: torch_pair(luma[0], luma[1], 16, 8))]
    fa = res["field"] = {name: {} for name, _ in legs}
    for rnd in ("round1", "round2"):
        for name, fn in legs:
            fa[name][rnd] = both(fn)
    for name in ("a_motion_field_p16_r8", "a_motion_field_p8_r4"):
        fa[name]["over_luma_integral"] = round(med(fa[name]) / med(fa["a_luma_integral"]), 2)
        fa[name]["gb_per_s_of_the_images_once"] = round(images.numel() / med(fa[name]) / 1e6, 1)
    pairs = 2 * (F - 1)
    fa["b_torch_unfold_one_pair_p16_r8"]["EXTRAPOLATED_video_ms"] = round(med(fa["b_torch_unfold_one_pair_p16_r8"]) * pairs, 1)
    fa["b_torch_unfold_one_pair_p16_r8"]["EXTRAPOLATED_over_motion_field"] = round(
        med(fa["b_torch_unfold_one_pair_p16_r8"]) * pairs / med(fa["a_motion_field_p16_r8"]), 1)
    del images

    # (c) + (d)
    boxes, scores = bench.synth_video_cuda(torch, 2000, F, a.boxes, C, dev)
    idx, cnt = ops.nms_volume(boxes, scores, THRESH)
    still = (boxes, scores, idx, cnt)
    p = ops.propagate_detections(m, still, top=TOP, reach=REACH)
    T = p['tracks'].shape[1]
    live = p['score'] == p['score']
    res["propagation"] = pa = {"slots_per_class": T, "rows": int(live.numel()), "rows_written_with_a_box": int(live.sum()),
                               "sources": int(cnt.clamp(max=TOP).sum())}
    shape = tuple(p['score'].shape)
    del live

    def fill(s):
        torch.full(shape + (5,), float('nan'), dtype=torch.float32, device=dev)
        torch.full(shape, float('nan'), dtype=torch.float32, device=dev)
        torch.full(shape, -2 ** 31, dtype=torch.int32, device=dev)

    plegs = [("c_propagate_detections", lambda s: ops.propagate_detections(m, still, top=TOP, reach=REACH, sync=s)),
             ("c_torch_full_of_the_outputs", fill)]
    for name, _ in plegs:
        pa[name] = {}
    for rnd in ("round1", "round2"):
        for name, fn in plegs:
            pa[name][rnd] = both(fn)
    out_bytes = shape[0] * shape[1] * shape[2] * 28          # five f32 of a row, its f32 score and its int32 source
    pa["output_bytes"] = out_bytes
    pa["c_propagate_detections"]["over_torch_full"] = round(med(pa["c_propagate_detections"]) / med(pa["c_torch_full_of_the_outputs"]), 2)
    pa["c_propagate_detections"]["gb_per_s_of_the_outputs"] = round(out_bytes / med(pa["c_propagate_detections"]) / 1e6, 1)
    na = res["nms_tracks"] = {"d_nms_tracks": {}}
    out = ops.nms_tracks(p['tracks'], p['ntracks'], p['score'], still=still, thresh=THRESH)
    na["rows_per_list"] = int(out['tracks'].shape[1])
    na["kept_per_list_mean"] = round(float(out['cnt'].float().mean()), 2)
    plain = ops.nms_tracks(p['tracks'][:, :0], torch.zeros_like(p['ntracks']), p['score'][:, :0], still=still, thresh=THRESH,
                           top_still=na["rows_per_list"] - T)
    na["kept_per_list_mean_without_propagation"] = round(float(plain['cnt'].float().mean()), 2)
    del out, plain
    for rnd in ("round1", "round2"):
        na["d_nms_tracks"][rnd] = both(lambda s: ops.nms_tracks(p['tracks'], p['ntracks'], p['score'], still=still, thresh=THRESH, sync=s),
                                       reps=max(a.reps // 4, 3))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
