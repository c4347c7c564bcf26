#!/usr/bin/env python3
"""Time the surface pass (Camera.surfaces -> vrt_hit_surfaces) against the first-hit pass that produced its records, on a
1920 x 1080 frame (one record per pixel), in one process, over two worlds:

    default      the default scene of the benchmarks (resolutions 1 and 2)
    sparse_lod   a sparse random world of 12 x 8 x 12 chunks of 16 at resolutions 1..3 with holes (gpu_util.sparse_scene), the
                 camera inside it: many rays end in the void, the hits lie in chunks of every resolution

Before anything is timed the pass's statistics are checked against the first-hit pass's (as many records examined as rays hit,
none refused, none orphaned).  Per world, alternating within every round (a round = one timed window of `--inner` calls of each),
bracketed by HIP events after warm-up: first_hit, pixel_rays (the rays the pass reads the velocities of) and surfaces.  Medians
over the rounds, each series' spread, the ratio surfaces / first_hit, and the bytes the pass moves per record: 48 (the hit) +
24 (the ray's velocity; the lines of the whole 64-byte ray record are fetched) read and 64 written, probes apart.  The windows
time calls through the Python layer.  One JSON object goes to stdout and, with --out, to that file.

    python tools/bench_surfaces.py --out profiles/surfaces_bench.json
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

WIDTH, HEIGHT = 1920, 1080
RECORD_BYTES = dict(hit_read=48, velocity_read=24, ray_lines_fetched=64, surface_written=64)


def window(torch, fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def world_camera(name):
    import oracle_lib as ol
    from gpu_util import camera_for, settings_store, sparse_scene
    if name == "default":
        sc = ol.default_scene()
        st = ol.make_settings(width=WIDTH, height=HEIGHT, samples=1, max_bounces=4)
        return sc, camera_for(sc, settings_store(st), sc.cam_pos, sc.cam_rot, sc.cam_lens, grid=sc.grid_lod0)
    sc = sparse_scene(404, 3, chunk_size=16, dims=(12, 8, 12), fill=0.03)
    st = ol.make_settings(width=WIDTH, height=HEIGHT, samples=1, max_bounces=4, chunk_size=16, dist_max=192)
    return sc, camera_for(sc, settings_store(st), (3.3, 2.6, -70.45), (0.0, 0.0, 0.0, 1.0), st["fov"] * np.pi / 8)


def run_world(name, warmup, rounds, inner):
    import torch
    import oracle_lib as ol
    from python_raytracer_amd import _native as nat
    sc, cam = world_camera(name)
    dp = cam.upload_pixels(np.concatenate(ol.pixel_lists(WIDTH, HEIGHT, 1)))
    hits = cam.first_hit(0, pixels=dp)
    rays, used = cam.pixel_rays(0, pixels=dp)
    s = cam.surfaces(hits, rays)
    assert int(s.stats[nat.S_SURFACE_EXAMINED]) == int(hits.stats[4]) == int(s.stats[nat.S_SURFACE_RESOLVED]), (s.stats, hits.stats)
    assert int(s.stats[nat.S_SURFACE_INVALID]) == 0 and int(s.stats[nat.S_SURFACE_ORPHANS]) == 0
    legs = {"first_hit": lambda: cam.first_hit(0, pixels=dp), "pixel_rays": lambda: cam.pixel_rays(0, pixels=dp),
            "surfaces": lambda: cam.surfaces(hits, rays)}
    for fn in legs.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in legs}
    for _ in range(rounds):
        for k, fn in legs.items():
            ms[k].append(window(torch, fn, inner))
    med = {k: statistics.median(v) for k, v in ms.items()}
    got = s.numpy()
    ok = got["status"] == 0
    n = int(len(got))
    res = sc.res[sc.present != 0]
    out = dict(world=name, chunk_size=int(sc.chunk_size), chunks_listed=int((sc.present != 0).sum()),
               chunks_at_resolution={str(r): int((res == r).sum()) for r in (1, 2, 3)},
               records=n, records_that_hit=int(ok.sum()), ambiguous=int(s.stats[nat.S_SURFACE_AMBIGUOUS]),
               enclosed=int(s.stats[nat.S_SURFACE_ENCLOSED]),
               resolved_at_resolution={str(r): int((got["resolution"][ok] == r).sum()) for r in (1, 2, 3)},
               asked=int((ok & (got["side"] | got["reflect"] | got["fetched"] != 0)).sum()),
               neighbours_through_chunk_get=int(np.unpackbits(got["fetched"][ok]).sum()))
    for k, v in ms.items():
        out[k + "_ms"] = round(med[k], 4)
        out[k + "_min_ms"] = round(min(v), 4)
        out[k + "_max_ms"] = round(max(v), 4)
        q = statistics.quantiles(v, n=4)
        out[k + "_iqr_over_median"] = round((q[2] - q[0]) / med[k], 4)
    out["surfaces_over_first_hit"] = round(med["surfaces"] / med["first_hit"], 4)
    moved = RECORD_BYTES["hit_read"] + RECORD_BYTES["velocity_read"] + RECORD_BYTES["surface_written"]
    out["bytes_per_record"] = moved
    out["surfaces_gb_per_s"] = round(n * moved / med["surfaces"] / 1e6, 1)
    out["surfaces_mrecords_per_s"] = round(n / med["surfaces"] / 1e3, 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--inner", type=int, default=10, help="calls per timed window")
    ap.add_argument("--worlds", nargs="*", default=["default", "sparse_lod"])
    ap.add_argument("--out", default="", help="write the JSON object to this file")
    args = ap.parse_args()
    import torch
    worlds = [run_world(w, args.warmup, args.rounds, args.inner) for w in args.worlds]
    out = dict(shape="%dx%dx1, first sample per pixel" % (WIDTH, HEIGHT), warmup=args.warmup, rounds=args.rounds,
               calls_per_window=args.inner, device=torch.cuda.get_device_name(0), record_bytes=RECORD_BYTES, worlds=worlds)
    text = json.dumps(out, indent=1)
    print(text, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
