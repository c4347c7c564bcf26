#!/usr/bin/env python3
"""Time V views of one scene rendered as ONE batch (Camera.render_views) against the same V views as a loop of
Camera.render with the pose set in between -- what a caller had to do before the batch existed, and the yardstick.

Both are bracketed by HIP events around the whole sequence (V frames or one batch), after warm-up, and repeated; the
medians are compared and the spread between the loop's own repeats is reported next to the ratio: the batch only counts
as faster if it wins by more than that.  The loop is timed twice (before and after the batch) for the same reason.  One
JSON line per shape goes to stdout and, with --out, is appended to that file.

    python tools/bench_views.py --out profiles/views_bench.jsonl
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

SHAPES = [dict(name="64x48x1_v64", width=64, height=48, samples=1, views=64),       # the reference's default window
          dict(name="640x360x2_v16", width=640, height=360, samples=2, views=16)]


def poses_for(sc, n):
    """A camera path round the scene's own camera: small steps and a slow turn, deterministic."""
    rng = np.random.default_rng(2024)
    pos0 = np.asarray(sc.cam_pos, np.float64)
    out = []
    for i in range(n):
        a = 0.35 * np.sin(2 * np.pi * i / max(n, 1))
        q = np.array([0.0, np.sin(a / 2), 0.0, np.cos(a / 2)])
        out.append((tuple(pos0 + rng.uniform(-1.5, 1.5, 3)), tuple(q)))
    return out


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
    from python_raytracer_amd.lib import vec3, quaternion
    sc = ol.default_scene()
    st = ol.make_settings(width=shape["width"], height=shape["height"], samples=shape["samples"], max_bounces=4)
    cam = camera_for(sc, settings_store(st), sc.cam_pos, sc.cam_rot, sc.cam_lens, grid=sc.grid_lod0)
    dp = cam.upload_pixels(np.concatenate(ol.pixel_lists(shape["width"], shape["height"], 1)))
    poses = poses_for(sc, shape["views"])

    def loop():
        for p, q in poses:
            cam.pos, cam.rot = vec3(*p), quaternion(*q)
            cam.render(0, pixels=dp, check=False)

    def batch():
        cam.render_views(poses, pixels=dp, check=False)

    # one checked pass of each first: the results must agree before anything is timed
    ref = []
    for p, q in poses:
        cam.pos, cam.rot = vec3(*p), quaternion(*q)
        ref.append(cam.render(0, pixels=dp))
    got = cam.render_views(poses, pixels=dp)
    for a, b in zip(got, ref):
        assert torch.equal(a.rgba_f32, b.rgba_f32) and torch.equal(a.image_u8, b.image_u8)
    draws = cam.fast_draws
    loop_a = timed(torch, loop, warmup, repeats)
    batch_ms = timed(torch, batch, warmup, repeats)
    loop_b = timed(torch, loop, warmup, repeats)
    assert cam.fast_draws == draws
    med_a, med_b, med_batch = statistics.median(loop_a), statistics.median(loop_b), statistics.median(batch_ms)
    med_loop = statistics.median(loop_a + loop_b)
    v = shape["views"]
    return dict(shape=shape["name"], views=v, rays_per_view=int(ref[0].stats[8]), warmup=warmup, repeats=repeats,
                device=torch.cuda.get_device_name(0),
                loop_ms=round(med_loop, 4), loop_ms_first=round(med_a, 4), loop_ms_second=round(med_b, 4),
                loop_spread=round(abs(med_a - med_b) / med_loop, 4),
                loop_min_ms=round(min(loop_a + loop_b), 4), loop_max_ms=round(max(loop_a + loop_b), 4),
                batch_ms=round(med_batch, 4), batch_min_ms=round(min(batch_ms), 4), batch_max_ms=round(max(batch_ms), 4),
                ratio=round(med_loop / med_batch, 3),
                loop_ms_per_view=round(med_loop / v, 5), batch_ms_per_view=round(med_batch / v, 5))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=30)
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
