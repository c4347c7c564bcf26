#!/usr/bin/env python3
"""What a contact log costs a batch of what-if runs: DeviceWorld.run_many timed three ways on the same commit, in one process,

    (i)   without a log                          vrt_physics_run_batch, the kernel it always was
    (ii)  contacts=Contacts(mode="pairs", of=[the thrown body])    vrt_physics_run_batch_contacts: one record per touch of that body
    (iii) contacts=Contacts(mode="voxels")       ... every contact of every body, bound by the capacity (--capacity a run)

on the README's two cases: 64 throws of the default mod's player for 40 ticks, and 256 futures of the 64 + 1 bodies of
tools/bench_physics.py falling onto their slab for 30 ticks -- and, for the kernels that make the reference's draws
(run_many(rng=), vrt_physics_run_batch_draws against the drawing instance of the log), on 64 throws in `fluid` for 24 ticks.
Before anything is timed the three must end every variant in the same bytes, and on the first four variants (ii) must be the
filter of (iii) run with a capacity that loses nothing.  A way is timed by the wall clock from before the
call until it returns (all end with a read-back, so the device has finished); the kernels alone by HIP events (time_kernel=True)
in runs of their own.  The three ways alternate within every repetition; medians, with the least and the largest, over --reps
repetitions after one untimed.  One JSON object goes to stdout and, with --out, to that file.  No threshold is fixed: the calls
without contacts= run unchanged kernels, and what the log costs is to be reported, not assumed.

    python tools/bench_physics_contacts.py --out profiles/physics_contacts_bench.json
"""
import argparse
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def summary(ms):
    return dict(median=round(statistics.median(ms), 3), least=round(min(ms), 3), largest=round(max(ms), 3))


def measure(spec, who, ticks, K, reps, capacity, label, seed=None):
    """seed: the batch makes the reference's draws, every variant from a copy of random.Random(seed): the drawing kernels."""
    import physics_batch_util as bu
    import physics_scenes as ps
    from bench_physics_run_many import throw
    from python_raytracer_amd.lib import vec3
    from python_raytracer_amd.world import Contacts, DeviceWorld
    objects, _, _, st = ps.project_scene(spec)
    cam = vec3(*spec["cam"])
    dw = DeviceWorld(16)
    variants = [bu.mapping(objects, {who: dict(vel=throw(k))}) for k in range(K)]
    draws = dict(rng=random.Random(seed)) if seed is not None else {}
    ways = dict(no_log=dict(draws), pairs_of_thrown=dict(draws, contacts=Contacts(capacity, "pairs", of=[objects[who]])),
                voxels_all=dict(draws, contacts=Contacts(capacity, "voxels")))
    # the three end in the same bytes, and the masked pairs are the filter of the full log
    first = {name: dw.run_many(objects, cam, st, ticks, variants, **kw) for name, kw in ways.items()}
    for name, r in first.items():
        assert r.records.tobytes() == first["no_log"].records.tobytes() and r.launches == first["no_log"].launches, name
    # (checked on the first variants, with a capacity that loses nothing: the timed capacity cuts every full log short)
    checked = 0
    whole = dw.run_many(objects, cam, st, ticks, variants[:4], contacts=Contacts(1 << 19, "voxels"), **draws)
    for k in range(4):
        full = whole.contacts(k)
        assert full.lost == 0 and full.records[:capacity].tobytes() == first["voxels_all"].contacts(k).records.tobytes(), k
        rec = full.pairs()
        want = rec[(rec["mover"] == who) | (rec["other"] == who)]
        got = first["pairs_of_thrown"].contacts(k)
        assert got.total == len(want) and all((got.records[f] == want[f]).all() for f in got.records.dtype.names), k
        checked += 1
    wall, kernel = {name: [] for name in ways}, {name: [] for name in ways}
    for rep in range(reps + 1):
        for name, kw in ways.items():
            t0 = time.perf_counter()
            dw.run_many(objects, cam, st, ticks, variants, **kw)
            if rep:
                wall[name].append((time.perf_counter() - t0) * 1e3)
        for name, kw in ways.items():
            ms = dw.run_many(objects, cam, st, ticks, variants, time_kernel=True, **kw).kernel_ms
            if rep:
                kernel[name].append(ms)
    rows = {}
    for name in ways:
        r = first[name]
        rows[name] = dict(wall_ms=summary(wall[name]), kernel_ms=summary(kernel[name]), launches=int(r.launches))
        if r.contacts_total is not None:
            rows[name].update(records_logged=int(r.contacts_total.sum()), records_lost=int(r.contacts_lost.sum()),
                              records_a_run_at_most=int(r.contacts_total.max()), capacity=capacity)
    for name in ("pairs_of_thrown", "voxels_all"):
        rows[name]["wall_over_no_log"] = round(rows[name]["wall_ms"]["median"] / rows["no_log"]["wall_ms"]["median"], 3)
        rows[name]["kernel_over_no_log"] = round(rows[name]["kernel_ms"]["median"] / rows["no_log"]["kernel_ms"]["median"], 3)
    out = dict(workload=label, bodies=len(objects), ticks=ticks, K=K, thrown=who, draws=seed is not None, samples=reps, ways=rows, ways_agree=True,
               pairs_checked_against_voxels=checked)
    print(label, json.dumps(rows), file=sys.stderr, flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7, help="timed repetitions of every way")
    ap.add_argument("--capacity", type=int, default=4096, help="records a run keeps at most")
    ap.add_argument("--out", default="", help="write the JSON object to this file")
    args = ap.parse_args()
    import torch
    import physics_draw_scenes as pds
    import physics_scenes as ps
    from bench_physics import falling_bodies
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    out = dict(device=torch.cuda.get_device_name(0),
               timing="wall clock per call incl. packing, upload and read-back; kernels by HIP events in separate runs; the ways alternate",
               workloads=[measure(ps.DEFAULT, len(ps.DEFAULT["objects"]) - 1, 40, 64, args.reps, args.capacity,
                                  "default mod, 40 ticks, 64 throws of the player"),
                          measure(falling_bodies(64), 1, 30, 256, args.reps, args.capacity,
                                  "64 bodies of 12^3 onto a 128 x 128 slab, 30 ticks, 256 futures of the first"),
                          measure(pds.FLUID, 2, 24, 64, args.reps, args.capacity,
                                  "fluid (fractional solidity, the reference's draws), 24 ticks, 64 throws of the cube", seed=pds.SEED)])
    text = json.dumps(out, indent=1)
    print(text, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
