#!/usr/bin/env python3
"""Time shaded explicit rays (Camera.shade_rays) against the frame (Camera.render) ON THE SAME RAYS, in one process, at the
BASELINE config 2 shape (1920 x 1080 x 1, max_bounces 4) over the default scene.

The rays are exactly the frame's, in slot order: the cached per-slot ray table is read back (lens quaternion and life per
slot), rot.multiply(o).vec_forward() and pos + vel * dist_min are formed in numpy in the reference's operation order; a
ray's draws are its slot's row of the cached draw table from index 1 + 2 on (the lod_random draw and the two lens draws came
first).  Before anything is timed the call's colours are asserted equal to the frame's per-sample colours, bit for bit.

Four things are timed, alternating within every round (a round = one timed window of `--inner` calls of each), bracketed by
HIP events after warm-up: Camera.render (image and per-pixel means, no traversed list, check=False so that nothing
synchronises inside a window: the yardstick, whose march is the frame's own kernel, not this one), shade_rays for colours only in slot order, the same rays under a fixed random permutation
-- what incoherent rays cost -- and shade_rays with records.  Medians over the rounds are reported, with each series' own
spread, and the ratios to the frame.  One JSON object goes to stdout and, with --out, to that file.

    python tools/bench_shade.py --out profiles/shade_bench.json
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

from bench_cast import SHAPE, camera_rays, window   # noqa: E402  (the same shape, ray reconstruction and timing window)


def run(warmup, rounds, inner):
    import torch
    import oracle_lib as ol
    from gpu_util import camera_for, settings_store
    shape = SHAPE
    sc = ol.default_scene()
    st = ol.make_settings(width=shape["width"], height=shape["height"], samples=shape["samples"], max_bounces=shape["max_bounces"])
    cam = camera_for(sc, settings_store(st), sc.cam_pos, sc.cam_rot, sc.cam_lens, grid=sc.grid_lod0)
    dp = cam.upload_pixels(np.concatenate(ol.pixel_lists(shape["width"], shape["height"], 1)))
    max_life = float(st["dist_max"])
    for fast_draws in (32, 64):       # (rows of the frame's 32-draw table, unless a ray of the frame outruns one)
        cam.fast_draws = fast_draws
        frame = cam.render(0, pixels=dp, want_image=True, want_f32=True, want_ray_rgba=True)
        rec, used = camera_rays(cam, dp, st)
        n, slots = len(rec), len(used)
        rows = dp.draw_table.cpu().numpy().view(np.float64).reshape(dp.n_distinct, -1)
        raw = dp.plan.cpu().numpy()
        off = 64 + ((4 * slots + 255) // 256) * 256
        seedidx = raw[off:off + 4 * slots].view(np.uint32)[used]
        first = 1 + (2 if st["dof"] != 0 else 0)
        draws = np.ascontiguousarray(rows[seedidx][:, first:])
        d_rec, d_draws = torch.from_numpy(rec).cuda(), torch.from_numpy(draws).cuda()
        if int(cam.shade_rays(d_rec, draws=d_draws, max_life=max_life, want_records=False).stats[10]) == 0:
            break
    cam.fast_draws = rows.shape[1]
    perm = np.random.default_rng(2024).permutation(n)
    d_perm, d_pdraws = torch.from_numpy(rec[perm]).cuda(), torch.from_numpy(draws[perm]).cuda()

    # the call must give the frame's colours before anything is timed
    want = frame.ray_rgba.cpu().numpy().view(np.uint32)[:slots][used]
    got = cam.shade_rays(d_rec, draws=d_draws, max_life=max_life)
    assert np.array_equal(got.rgba.cpu().numpy().view(np.uint32), want), "shade_rays' colours are not the frame's"
    assert int(got.stats[8]) == n == int(frame.stats[8]) and int(got.stats[9]) == 0 and int(got.stats[10]) == 0
    lean = cam.shade_rays(d_perm, draws=d_pdraws, max_life=max_life, want_records=False)
    assert np.array_equal(lean.rgba.cpu().numpy().view(np.uint32), want[perm])

    # (check=False: no statistics are copied to the host, so the frames of a window queue up like the calls of the other legs)
    legs = {"render": lambda: cam.render(0, pixels=dp, want_image=True, want_f32=True, want_traversed=False, check=False),
            "shade": lambda: cam.shade_rays(d_rec, draws=d_draws, max_life=max_life, want_records=False),
            "shade_permuted": lambda: cam.shade_rays(d_perm, draws=d_pdraws, max_life=max_life, want_records=False),
            "shade_records": lambda: cam.shade_rays(d_rec, draws=d_draws, max_life=max_life)}
    for fn in legs.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in legs}
    for _ in range(rounds):
        for k, fn in legs.items():
            ms[k].append(window(torch, fn, inner))
    med = {k: statistics.median(v) for k, v in ms.items()}
    hits = int(got.stats[4])
    out = dict(shape=shape["name"], rays=n, hits=hits, draws_per_row=int(draws.shape[1]), draw_bytes_per_ray=int(draws.shape[1]) * 8,
               warmup=warmup, rounds=rounds, calls_per_window=inner, device=torch.cuda.get_device_name(0))
    for k, v in ms.items():
        out[k + "_ms"] = round(med[k], 4)
        out[k + "_min_ms"] = round(min(v), 4)
        out[k + "_max_ms"] = round(max(v), 4)
        q = statistics.quantiles(v, n=4)
        out[k + "_iqr_over_median"] = round((q[2] - q[0]) / med[k], 4)
    out["shade_over_render"] = round(med["shade"] / med["render"], 4)
    out["shade_permuted_over_shade"] = round(med["shade_permuted"] / med["shade"], 3)
    out["shade_records_over_shade"] = round(med["shade_records"] / med["shade"], 3)
    out["shade_mrays_per_s"] = round(n / med["shade"] / 1e3, 1)
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
