#!/usr/bin/env python3
"""Greedy tubelet generation with the pixel tracker on the device (ops.track_volume_pixels) at the c2 shape -- 300 frames x
10 000 proposals x 200 classes, max_tracks 10 -- on the 300-frame 720 x 1280 synthetic video of devtools/bench_pixtrack.py:
  python devtools/bench_greedy_pixels.py [--reps R] [--warmup W] [--frames F] [--boxes B] [--host-classes N] [--host-tracks K]
Settings grid 32 / radius 8, step 1 and step 3.  Comparators on the same inputs, never the code under
test:
 (b) ops.track_volume: the IoU link does DIFFERENT work (it scans proposals, not pixels): for scale only;
 (c) ops.top_anchors + ops.track_pixels: the same chains' arithmetic in one launch, but NO suppression (its tubelets repeat
     each other's objects);
 (d) the dict-level host loop, vdet.track.greedily_track_from_raw_dets with pixel_tracker (one track_pixels launch with
     C = T = 1, a download and one track_det_nms_batch call with a host wait per track): timed on N classes x K tracks,
     step 3, and scaled to 200 classes x 10 tracks: EXTRAPOLATED.
HIP-event ms, median [min .. max] of R calls after W warm-up calls; the device legs alternate and the whole turn runs twice,
so the spread of each shows.  Prints one JSON line."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "devtools"))
import numpy as np
import torch

S, R, T, C = 32, 8, 10, 200


class Opts(object):
    def __init__(self, **kw):
        self.__dict__.update(kw)


def shape_of(tracks, ntracks):
    live = tracks[..., 0] == tracks[..., 0]
    n = int(ntracks.sum())
    return {"tubelets": n, "steps": int(live.sum()) - n, "mean_confidence": round(float(tracks[..., 4][live].mean()), 4),
            "longest_tubelet_rows": int(live.sum(-1).max())}


def main():
    import argparse
    import bench
    from bench_pixtrack import panning_video
    from bench_tcn import device_times
    from vdetlib_amd import ops
    from vdetlib_amd.vdet import track
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--boxes", type=int, default=10000)
    ap.add_argument("--host-classes", type=int, default=2)
    ap.add_argument("--host-tracks", type=int, default=4)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    F, H, W = a.frames, 720, 1280
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup, "frames": F, "boxes": a.boxes, "classes": C,
           "max_tracks": T, "image": [H, W], "grid": S, "radius": R}
    boxes, scores = bench.synth_video_cuda(torch, 2000, F, a.boxes, C, dev)
    images = panning_video(dev, F, H, W)
    greedy = lambda step: (lambda s: ops.track_volume_pixels(images, boxes, scores, max_tracks=T, grid=S, radius=R, step=step, sync=s))
    link = lambda s: ops.track_volume(boxes, scores, max_tracks=T, sync=s)

    def route(step):
        def fn(s):
            fr, ab, sc, _ = ops.top_anchors(boxes, scores, T, sync=False)
            return ops.track_pixels(images, fr, ab, sc, grid=S, radius=R, step=step, sync=s)
        return fn

    legs = (("a_track_volume_pixels_step1", greedy(1)), ("a_track_volume_pixels_step3", greedy(3)), ("b_track_volume", link),
            ("c_top_anchors_track_pixels_step1", route(1)), ("c_top_anchors_track_pixels_step3", route(3)))
    for name, fn in legs:
        tr, _, nt = fn(True)
        res[name] = shape_of(tr, nt)
    res["b_track_volume"]["note"] = "different work (IoU link over %d proposals a frame): for scale" % a.boxes
    for name in ("c_top_anchors_track_pixels_step1", "c_top_anchors_track_pixels_step3"):
        res[name]["note"] = "no suppression: the tubelets repeat each other's objects"
    for rnd in ("round1", "round2"):
        for name, fn in legs:
            ev, wall = device_times(fn, a.reps, a.warmup)
            res[name][rnd] = {"event_ms": ev, "wall_ms": wall}
    # (d) the dict-level host loop on a few classes and tracks, step 3: EXTRAPOLATED by tracks
    n, k = max(1, min(a.host_classes, C)), max(1, min(a.host_tracks, T))
    tracks, anchors, ntracks = (x.cpu().numpy() for x in greedy(3)(True))
    det_info = np.hstack([np.repeat(np.arange(1, F + 1), a.boxes)[:, None].astype(np.float64),
                          boxes.reshape(-1, 4).cpu().numpy().astype(np.float64),
                          scores[:, :, :n].reshape(-1, n).cpu().numpy().astype(np.float64)])
    vid = {'video': 'benchvid', 'root_path': '', 'frames': [{'frame': f + 1, 'path': ''} for f in range(F)]}
    opts = Opts(step=3, max_frames=None, max_tracks=k, thres=0.0, nms_thres=0.3, grid=S, radius=R, min_conf=0.5)
    track._pixel_video.clear()
    track._pixel_video[('benchvid', F)] = images          # (the upload is not part of what is compared)
    view = lambda proto: [[(b['frame'], b['bbox'], b['score']) for b in t] for t in proto['tracks']]
    secs, made, equal = 0.0, 0, True
    try:
        for c in range(n):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            host = track.greedily_track_from_raw_dets(vid, det_info, track.pixel_tracker, c + 1, opts)
            torch.cuda.synchronize()
            secs += time.perf_counter() - t0
            made += len(host['tracks'])
            mine = ops.tracks_to_proto('benchvid', tracks[c], anchors[c], min(int(ntracks[c]), k), method='pixel_tracker')
            equal = equal and view(host) == view(mine)
    finally:
        track._pixel_video.clear()
    res["d_host_loop_step3"] = {"classes": n, "tracks_per_class": k, "tubelets": made, "seconds": round(secs, 2),
                                "includes": "the class's sort of %d detections on the host" % (F * a.boxes),
                                "equal_to_device": bool(equal),
                                "EXTRAPOLATED_video_s": round(secs / max(made, 1) * C * T, 1)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
