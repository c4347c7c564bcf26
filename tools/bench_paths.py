#!/usr/bin/env python3
"""Time hit paths (Camera.path_rays) against shaded explicit rays (Camera.shade_rays, colours only) ON THE SAME RAYS AND DRAWS,
in one process, at the BASELINE config 2 shape (1920 x 1080 x 1, max_bounces 4) over the default scene: what the stores of
the hit records cost, which nobody fixed in advance -- shade_rays itself runs the code it ran before.

The rays are the frame's own, in slot order, from Camera.pixel_rays; a ray's draws are the row of its seed
(1 + x)(1 + y)(1 + s), made on the device (vrt_rng_draws), from index 1 + 2 on (the lod_random draw and the two lens draws
came first).  Before anything is timed path_rays' colours are asserted equal to the frame's per-sample colours and to
shade_rays', bit for bit.

Four things are timed, alternating within every round (a round = one timed window of `--inner` calls of each), bracketed by
HIP events after warm-up: shade_rays(want_records=False), and path_rays at max_hits 1, 8 and 32.  Medians over the rounds
are reported, with each series' own spread, and the ratios to shade_rays.  One JSON object goes to stdout and, with --out,
to that file.

    python tools/bench_paths.py --out profiles/path_bench.json
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

from bench_cast import SHAPE, window   # noqa: E402  (the same shape and timing window)

MAX_HITS = (1, 8, 32)


def run(warmup, rounds, inner):
    import torch
    import oracle_lib as ol
    from gpu_util import camera_for, settings_store
    from python_raytracer_amd import _native as nat
    shape = SHAPE
    sc = ol.default_scene()
    st = ol.make_settings(width=shape["width"], height=shape["height"], samples=shape["samples"], max_bounces=shape["max_bounces"])
    cam = camera_for(sc, settings_store(st), sc.cam_pos, sc.cam_rot, sc.cam_lens, grid=sc.grid_lod0)
    dp = cam.upload_pixels(np.concatenate(ol.pixel_lists(shape["width"], shape["height"], 1)))
    max_life = float(st["dist_max"])
    frame = cam.render(0, pixels=dp, want_image=False, want_f32=False, want_ray_rgba=True)
    rays, used = cam.pixel_rays(pixels=dp, all_samples=True)
    px = dp.array.astype(np.int64)
    smax = frame.max_samples
    seeds = (((1 + px[:, 0]) * (1 + px[:, 1]))[:, None] * (1 + np.arange(smax))[None, :]).reshape(-1)
    keep = used.cpu().numpy()
    d_rec = rays[used].contiguous()
    n = int(d_rec.shape[0])
    first = 1 + (2 if st["dof"] != 0 else 0)
    d_seeds = torch.from_numpy(np.ascontiguousarray(seeds[keep])).cuda()
    for width in (32, 64):       # (the frame's 32-draw rows, unless a ray outruns one)
        rows = torch.empty((n, width), dtype=torch.float64, device="cuda")
        nat.check(nat.lib().vrt_rng_draws(d_seeds.data_ptr(), n, width, rows.data_ptr(), torch.cuda.current_stream().cuda_stream),
                  "vrt_rng_draws")
        d_draws = rows[:, first:].contiguous()
        shade = cam.shade_rays(d_rec, draws=d_draws, max_life=max_life, want_records=False)
        if int(shade.stats[10]) == 0:
            break

    # the calls must give the frame's colours before anything is timed
    want = frame.ray_rgba.cpu().numpy().view(np.uint32)[keep]
    assert np.array_equal(shade.rgba.cpu().numpy().view(np.uint32), want), "shade_rays' colours are not the frame's"
    hist = None
    for mh in MAX_HITS:
        got = cam.path_rays(d_rec, draws=d_draws, max_life=max_life, max_hits=mh)
        assert np.array_equal(got.rgba.cpu().numpy().view(np.uint32), want), "path_rays' colours are not the frame's"
        assert np.array_equal(got.stats[:11], shade.stats[:11]) and int(got.stats[8]) == n and int(got.stats[9]) == 0
        counts = got.counts.cpu().numpy()
        assert int(got.stats[13]) == int(np.minimum(counts, mh).sum()) and int(got.stats[12]) == int((counts > mh).sum())
        hist = np.bincount(counts)
    del got

    legs = {"shade": lambda: cam.shade_rays(d_rec, draws=d_draws, max_life=max_life, want_records=False)}
    for mh in MAX_HITS:
        legs["path_%d" % mh] = (lambda mh=mh: cam.path_rays(d_rec, draws=d_draws, max_life=max_life, max_hits=mh))
    for fn in legs.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in legs}
    for _ in range(rounds):
        for k, fn in legs.items():
            ms[k].append(window(torch, fn, inner))
    med = {k: statistics.median(v) for k, v in ms.items()}
    out = dict(shape=shape["name"], rays=n, hits=int(shade.stats[4]), most_hits_on_a_ray=int(len(hist) - 1),
               rays_by_hits=[int(v) for v in hist], draws_per_row=int(d_draws.shape[1]), warmup=warmup, rounds=rounds,
               calls_per_window=inner, device=torch.cuda.get_device_name(0))
    for k, v in ms.items():
        out[k + "_ms"] = round(med[k], 4)
        out[k + "_min_ms"] = round(min(v), 4)
        out[k + "_max_ms"] = round(max(v), 4)
        q = statistics.quantiles(v, n=4)
        out[k + "_iqr_over_median"] = round((q[2] - q[0]) / med[k], 4)
    for mh in MAX_HITS:
        out["path_%d_over_shade" % mh] = round(med["path_%d" % mh] / med["shade"], 4)
        out["path_%d_record_bytes" % mh] = n * mh * nat.HIT_BYTES
    out["shade_mrays_per_s"] = round(n / med["shade"] / 1e3, 1)
    out["path_8_mrays_per_s"] = round(n / med["path_8"] / 1e3, 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=40)
    ap.add_argument("--inner", type=int, default=10, help="calls per timed window")
    ap.add_argument("--out", default="", help="write the JSON object to this file")
    args = ap.parse_args()
    text = json.dumps(run(args.warmup, args.rounds, args.inner), indent=1)
    print(text, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
