#!/usr/bin/env python3
"""Time K what-if runs by the two routes there are, in one process:

    (i)  DeviceWorld.run_many   the bodies are packed once, replicated K times with the variants patched in, uploaded once; one
                                launch of K workgroups (vrt_physics_run_batch) steps them all; one read-back
    (ii) the loop it replaces   K times DeviceWorld.run on a fresh twin of the objects with the variant applied (the twins are
                                made before the clock starts: the loop is charged for its runs alone)

on two workloads: the default mod (tests/physics_scenes.py, the 40 ticks of tests/golden/physics_default.npz) with the player
thrown K different ways, and the 64 + 1 bodies of tools/bench_physics.py falling onto their slab for 30 ticks with the first body
thrown K different ways; K = 1, 16, 64, 256.  Before anything is timed both routes must end every variant in the same bytes.
A route is timed by the wall clock from before the call until it returns (both end with a read-back, so the device has
finished); the kernels alone by HIP events (time_kernel=True) in runs of their own.  Medians over --reps runs after one untimed.
One JSON object goes to stdout and, with --out, to that file.  No ratio is fixed in advance: nobody had measured these.

    python tools/bench_physics_run_many.py --out profiles/physics_batch_bench.json
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

KS = (1, 16, 64, 256)


def throw(k):
    """Variant k's velocity for the thrown body: 256 different ones, all well inside the device's limits."""
    return (0.25 * (k % 8) - 0.875, 0.5 * ((k // 8) % 8), 0.125 * (k // 64) - 0.1875)


def measure(spec, who, ticks, reps, label):
    import physics_batch_util as bu
    import physics_scenes as ps
    from python_raytracer_amd.lib import vec3
    from python_raytracer_amd.world import DeviceWorld
    objects, _, _, st = ps.project_scene(spec)
    cam = vec3(*spec["cam"])
    dw, dw_loop = DeviceWorld(16), DeviceWorld(16)
    rows = []
    for K in KS:
        changes = [{who: dict(vel=throw(k))} for k in range(K)]
        variants = [bu.mapping(objects, c) for c in changes]
        # both routes end in the same bytes
        r = dw.run_many(objects, cam, st, ticks, variants)
        for k, change in enumerate(changes):
            t = dw_loop.run(bu.altered(objects, change), cam, st, ticks)
            assert r.records[k].tobytes() == t.records.tobytes(), "the two routes disagree at variant %d of %d (%s)" % (k, K, label)
        batch_ms, loop_ms = [], []
        for rep in range(reps):
            t0 = time.perf_counter()
            r = dw.run_many(objects, cam, st, ticks, variants)
            batch_ms.append((time.perf_counter() - t0) * 1e3)
            twins = [bu.altered(objects, change) for change in changes]
            t0 = time.perf_counter()
            for twin in twins:
                dw_loop.run(twin, cam, st, ticks)
            loop_ms.append((time.perf_counter() - t0) * 1e3)
        batch_kernel = [dw.run_many(objects, cam, st, ticks, variants, time_kernel=True).kernel_ms for rep in range(reps)]
        loop_kernel = sum(dw_loop.run(bu.altered(objects, change), cam, st, ticks, time_kernel=True).kernel_ms for change in changes)
        row = dict(K=K, launches=int(r.launches), run_many_ms=round(statistics.median(batch_ms), 3), loop_of_runs_ms=round(statistics.median(loop_ms), 3),
                   run_many_kernel_ms=round(statistics.median(batch_kernel), 3), loop_kernels_ms=round(loop_kernel, 3), samples=reps)
        row["loop_over_run_many"] = round(row["loop_of_runs_ms"] / row["run_many_ms"], 2)
        row["run_many_ms_per_variant"] = round(row["run_many_ms"] / K, 4)
        rows.append(row)
        print(label, row, file=sys.stderr, flush=True)
    return dict(workload=label, bodies=len(objects), ticks=ticks, thrown=who, rows=rows, routes_agree=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3, help="timed runs of either route per K")
    ap.add_argument("--out", default="", help="write the JSON object to this file")
    args = ap.parse_args()
    import torch
    import physics_scenes as ps
    from bench_physics import falling_bodies
    out = dict(device=torch.cuda.get_device_name(0),
               timing="wall clock per call incl. packing, upload and read-back, medians; kernels by HIP events in separate runs",
               workloads=[measure(ps.DEFAULT, len(ps.DEFAULT["objects"]) - 1, 40, args.reps, "default mod, 40 ticks, the player thrown"),
                          measure(falling_bodies(64), 1, 30, args.reps, "64 bodies of 12^3 onto a 128 x 128 slab, 30 ticks, the first thrown")])
    text = json.dumps(out, indent=1)
    print(text, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
