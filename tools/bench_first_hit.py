#!/usr/bin/env python3
"""Time the first-hit pass (Camera.first_hit: depth, voxel and material per primary ray) against the colour frame
(Camera.render) of the same camera, in one process, at the BASELINE config 2 and config 3 shapes over the default scene.

Both are bracketed by HIP events, after warm-up, and repeated; the medians are compared.  The colour frame is timed twice
(before and after the first-hit pass) and the spread between its two medians is reported next to the ratio.  The pass is
timed for every sample slot (all_samples, the rays of the colour frame) and for first samples only.  One JSON line per
shape goes to stdout and, with --out, is appended to that file.

    python tools/bench_first_hit.py --out profiles/first_hit_bench.jsonl
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPES = [dict(name="c2_1920x1080x1", width=1920, height=1080, samples=1, max_bounces=4),      # BASELINE config 2
          dict(name="c3_3840x2160x8", width=3840, height=2160, samples=8, max_bounces=8)]      # BASELINE config 3


def timed(torch, fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


def run_shape(shape, warmup, repeats):
    import torch
    import oracle_lib as ol
    from gpu_util import camera_for, settings_store
    sc = ol.default_scene()
    st = ol.make_settings(width=shape["width"], height=shape["height"], samples=shape["samples"], max_bounces=shape["max_bounces"])
    cam = camera_for(sc, settings_store(st), sc.cam_pos, sc.cam_rot, sc.cam_lens, grid=sc.grid_lod0)
    dp = cam.upload_pixels(np.concatenate(ol.pixel_lists(shape["width"], shape["height"], 1)))

    def frame():
        cam.render(0, pixels=dp, check=False)

    def hits_all():
        cam.first_hit(0, pixels=dp, all_samples=True)

    def hits_first():
        cam.first_hit(0, pixels=dp)

    # one checked pass of each first: the two must agree on which rays found a voxel before anything is timed
    r = cam.render(0, pixels=dp)
    h = cam.first_hit(0, pixels=dp, all_samples=True)
    assert int(h.stats[8]) == int(r.stats[8]), (h.stats, r.stats)
    h1 = cam.first_hit(0, pixels=dp)
    assert torch.equal(h1.material, h.material[:: h.max_samples])
    draws = cam.fast_draws
    frame_a = timed(torch, frame, warmup, repeats)
    all_ms = timed(torch, hits_all, warmup, repeats)
    first_ms = timed(torch, hits_first, warmup, repeats)
    frame_b = timed(torch, frame, warmup, repeats)
    assert cam.fast_draws == draws
    med_a, med_b = statistics.median(frame_a), statistics.median(frame_b)
    med_frame = statistics.median(frame_a + frame_b)
    med_all, med_first = statistics.median(all_ms), statistics.median(first_ms)
    rays = int(h.stats[8])
    return dict(shape=shape["name"], rays=rays, rays_that_hit=int(h.stats[4]), first_sample_rays=int(h1.stats[8]), warmup=warmup,
                repeats=repeats, device=torch.cuda.get_device_name(0),
                render_ms=round(med_frame, 4), render_ms_first=round(med_a, 4), render_ms_second=round(med_b, 4),
                render_spread=round(abs(med_a - med_b) / med_frame, 4),
                first_hit_all_samples_ms=round(med_all, 4), first_hit_all_samples_min_ms=round(min(all_ms), 4),
                first_hit_all_samples_max_ms=round(max(all_ms), 4),
                first_hit_ms=round(med_first, 4), first_hit_min_ms=round(min(first_ms), 4), first_hit_max_ms=round(max(first_ms), 4),
                render_over_first_hit_all_samples=round(med_frame / med_all, 3),
                first_hit_all_samples_mrays_per_s=round(rays / med_all / 1e3, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--shape", default="", help="name of one shape (default: both)")
    ap.add_argument("--out", default="", help="append the JSON lines to this file")
    args = ap.parse_args()
    for shape in SHAPES:
        if args.shape and shape["name"] != args.shape:
            continue
        line = json.dumps(run_shape(shape, args.warmup, args.repeats))
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
