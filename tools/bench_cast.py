#!/usr/bin/env python3
"""Time explicit rays (Camera.cast_rays) against the first-hit pass (Camera.first_hit) ON THE SAME RAYS, in one process, at
the BASELINE config 2 shape (1920 x 1080 x 1) over the default scene.

The rays are exactly those of Camera.first_hit(all_samples=True), in slot order: the cached per-slot ray table is read back
(lens quaternion and life per slot), rot.multiply(o).vec_forward() and pos + vel * dist_min are formed in numpy in the
reference's operation order, and the records of the cast are asserted equal to the first-hit pass's, bit for bit, before
anything is timed.  The yardstick reads one 64-byte record per ray as the cast does, plus the quaternion product.

Three things are timed, alternating within every round (a round = one timed window of `--inner` calls of each), bracketed by
HIP events after warm-up: first_hit, the cast in slot order, and the cast of the same rays in a fixed random permutation --
what incoherent rays cost.  Medians over the rounds are reported, with each series' own spread, the ratio
cast / first_hit (expected at most 1.10) and permuted / in-order (reported only).  One JSON object goes to stdout and, with
--out, to that file.

    python tools/bench_cast.py --out profiles/cast_bench.json
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

SHAPE = dict(name="c2_1920x1080x1", width=1920, height=1080, samples=1, max_bounces=4)      # BASELINE config 2


def window(torch, fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def camera_rays(cam, dp, st):
    """(records [n, 8] float64 of the used slots, used mask): the rays of first_hit(all_samples=True), from the cached ray table."""
    tab = dp.ray_table.cpu().numpy().view(np.float64).reshape(-1, 8)
    used = tab[:, 4] >= 0
    ox, oy, oz, ow = (tab[used, i] for i in range(4))
    x, y, z, w = (float(v) for v in (cam.rot.x, cam.rot.y, cam.rot.z, cam.rot.w))
    qx, qy = w * ox + z * oy - y * oz + x * ow, z * ox + w * oy + x * oz + y * ow     # lib.py:353-358
    qz, qw = y * ox - x * oy + w * oz + z * ow, x * ox - y * oy - z * oz + w * ow
    vel = np.stack([2 * (qz * qx + qw * qy), 2 * (qy * qx - qw * qz), 1 - 2 * (qz * qz + qy * qy)], -1)   # lib.py:372-376
    pos = np.array([float(cam.pos.x), float(cam.pos.y), float(cam.pos.z)])
    rec = np.zeros((int(used.sum()), 8))
    rec[:, 0:3] = pos + vel * float(st["dist_min"])
    rec[:, 3:6] = vel
    rec[:, 6] = tab[used, 4]
    return rec, used


def run(warmup, rounds, inner):
    import torch
    import oracle_lib as ol
    from gpu_util import camera_for, settings_store
    shape = SHAPE
    sc = ol.default_scene()
    st = ol.make_settings(width=shape["width"], height=shape["height"], samples=shape["samples"], max_bounces=shape["max_bounces"])
    cam = camera_for(sc, settings_store(st), sc.cam_pos, sc.cam_rot, sc.cam_lens, grid=sc.grid_lod0)
    dp = cam.upload_pixels(np.concatenate(ol.pixel_lists(shape["width"], shape["height"], 1)))
    h = cam.first_hit(0, pixels=dp, all_samples=True)
    rec, used = camera_rays(cam, dp, st)
    n = len(rec)
    perm = np.random.default_rng(2024).permutation(n)
    d_rec = torch.from_numpy(rec).cuda()
    d_perm = torch.from_numpy(rec[perm]).cuda()
    max_life = float(st["dist_max"])

    # the three must agree before anything is timed
    want = h.numpy()[: len(used)][used]
    got = cam.cast_rays(d_rec, max_life=max_life)
    assert got.numpy().tobytes() == want.tobytes(), "the cast's records are not the first-hit pass's"
    assert cam.cast_rays(d_perm, max_life=max_life).numpy().tobytes() == want[perm].tobytes()
    assert int(got.stats[8]) == int(h.stats[8]) == n and int(got.stats[4]) == int(h.stats[4]) and int(got.stats[9]) == 0

    legs = {"first_hit": lambda: cam.first_hit(0, pixels=dp, all_samples=True),
            "cast": lambda: cam.cast_rays(d_rec, max_life=max_life),
            "cast_permuted": lambda: cam.cast_rays(d_perm, max_life=max_life)}
    for fn in legs.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in legs}
    for _ in range(rounds):
        for k, fn in legs.items():
            ms[k].append(window(torch, fn, inner))
    med = {k: statistics.median(v) for k, v in ms.items()}
    out = dict(shape=shape["name"], rays=n, rays_that_hit=int(h.stats[4]), warmup=warmup, rounds=rounds, calls_per_window=inner,
               device=torch.cuda.get_device_name(0))
    for k, v in ms.items():
        out[k + "_ms"] = round(med[k], 4)
        out[k + "_min_ms"] = round(min(v), 4)
        out[k + "_max_ms"] = round(max(v), 4)
        q = statistics.quantiles(v, n=4)
        out[k + "_iqr_over_median"] = round((q[2] - q[0]) / med[k], 4)
    out["cast_over_first_hit"] = round(med["cast"] / med["first_hit"], 4)
    out["cast_permuted_over_cast"] = round(med["cast_permuted"] / med["cast"], 3)
    out["cast_mrays_per_s"] = round(n / med["cast"] / 1e3, 1)
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
