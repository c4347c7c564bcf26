#!/usr/bin/env python3
"""What scripted accelerations buy a batch of what-if runs, and what carrying them costs: on one commit, in one process,

    (a) run_many(impulses=)       K variants, variant k pushing the thrown body once before tick k mod T: ONE batch
                                  (vrt_physics_run_batch_impulses, no log)
    (b) the loop it replaces      per variant two DeviceWorld.run() calls with Object.accelerate between them (one call where
                                  the push comes before tick 0), on twins made before the clock starts: the parent's API
    (c) the cost of carrying it   run_many(impulses=[]) -- the new kernels with nothing to do -- against run_many() and, with
                                  contacts=, against run_many(contacts=): the kernels they restate

on the two workloads of DESIGN.md section 6i: the default mod for 40 ticks with K = 64, and 64 + 1 bodies of
tools/bench_physics.py for 30 ticks with K = 64.  Before anything is timed every way must end every variant in the same bytes:
(a) against (b) body for body, (c) against the batch without a list record for record.  A way is timed by the wall clock from
before its first call until its last returns (all end with a read-back, so the device has finished); kernels alone by HIP events
(time_kernel=True) in runs of their own.  The ways alternate within every repetition; medians, with the least and the largest,
over --reps repetitions after one untimed.  One JSON object goes to stdout and, with --out, to that file.  No ratio is fixed in
advance.

    python tools/bench_physics_impulses.py --out profiles/physics_impulses_bench.json
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


def summary(ms):
    return dict(median=round(statistics.median(ms), 3), least=round(min(ms), 3), largest=round(max(ms), 3))


def measure(spec, who, ticks, K, reps, label):
    import numpy as np
    import physics_batch_util as bu
    import physics_scenes as ps
    from bench_physics_run_many import throw
    from python_raytracer_amd.lib import vec3
    from python_raytracer_amd.world import Contacts, DeviceWorld
    objects, _, _, st = ps.project_scene(spec)
    cam = vec3(*spec["cam"])
    dw, dw_loop = DeviceWorld(16), DeviceWorld(16)
    pushes = [(k % ticks, throw(k)) for k in range(K)]
    variants = [{objects[who]: dict(impulses=[push])} for push in pushes]
    nothing = [{} for _ in range(K)]
    log = Contacts(4096, "pairs", of=[objects[who]])

    def batch():
        return dw.run_many(objects, cam, st, ticks, variants)

    def loop(twins):
        """Per variant: run to the push, accelerate, run on.  Returns the final (pos, vel) of every variant's bodies."""
        out = []
        for (t, vel), group in zip(pushes, twins):
            if t:
                dw_loop.run(group, cam, st, t)
            group[who].accelerate(vec3(*vel))
            dw_loop.run(group, cam, st, ticks - t)
            out.append(group)
        return out

    # (a) and (b) end every variant in the same bytes; (c) is the batch without a list record for record
    r = batch()
    ended = loop([bu.twins(objects) for _ in range(K)])
    for k, group in enumerate(ended):
        pos = np.array([o.pos.tuple() for o in group], np.float64)
        vel = np.array([o.vel.tuple() for o in group], np.float64)
        assert pos.tobytes() == np.ascontiguousarray(r.records[k]["pos"]).tobytes(), (label, k)
        assert vel.tobytes() == np.ascontiguousarray(r.records[k]["vel"]).tobytes(), (label, k)
    assert r.impulses_applied.tolist() == [1] * K and not r.impulses_skipped.any()
    carry = dict(plain=dict(), empty_list=dict(impulses=[]), log=dict(contacts=log), log_empty_list=dict(contacts=log, impulses=[]))
    first = {name: dw.run_many(objects, cam, st, ticks, nothing, **kw) for name, kw in carry.items()}
    for name, f in first.items():
        assert f.records.tobytes() == first["plain"].records.tobytes() and f.launches == first["plain"].launches, name
        assert (f.stats == first["plain"].stats).all(), name
    wall = {name: [] for name in ("batch", "loop", *carry)}
    kernel = {name: [] for name in ("batch", *carry)}
    for rep in range(reps + 1):
        twins = [bu.twins(objects) for _ in range(K)]      # (made before the clock starts)
        t0 = time.perf_counter()
        batch()
        t1 = time.perf_counter()
        loop(twins)
        t2 = time.perf_counter()
        if rep:
            wall["batch"].append((t1 - t0) * 1e3), wall["loop"].append((t2 - t1) * 1e3)
        for name, kw in carry.items():
            t0 = time.perf_counter()
            dw.run_many(objects, cam, st, ticks, nothing, **kw)
            if rep:
                wall[name].append((time.perf_counter() - t0) * 1e3)
        ms = dw.run_many(objects, cam, st, ticks, variants, time_kernel=True).kernel_ms
        if rep:
            kernel["batch"].append(ms)
        for name, kw in carry.items():
            ms = dw.run_many(objects, cam, st, ticks, nothing, time_kernel=True, **kw).kernel_ms
            if rep:
                kernel[name].append(ms)
    rows = {name: dict(wall_ms=summary(wall[name])) for name in wall}
    for name in kernel:
        rows[name]["kernel_ms"] = summary(kernel[name])
    med = lambda name, what: rows[name][what]["median"]  # noqa: E731
    rows["loop"]["runs"] = sum(2 if t else 1 for t, _ in pushes)
    rows["batch"].update(launches=int(r.launches), loop_over_batch_wall=round(med("loop", "wall_ms") / med("batch", "wall_ms"), 1))
    for new, old in (("empty_list", "plain"), ("log_empty_list", "log")):
        rows[new].update(kernel_over_restated=round(med(new, "kernel_ms") / med(old, "kernel_ms"), 3),
                         wall_over_restated=round(med(new, "wall_ms") / med(old, "wall_ms"), 3))
    rows["empty_list"]["kernel_over_log"] = round(med("empty_list", "kernel_ms") / med("log", "kernel_ms"), 3)
    out = dict(workload=label, bodies=len(objects), ticks=ticks, K=K, thrown=who, samples=reps, ways=rows, ways_agree=True)
    print(label, json.dumps(rows), file=sys.stderr, flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7, help="timed repetitions of every way")
    ap.add_argument("--out", default="", help="write the JSON object to this file")
    args = ap.parse_args()
    import torch
    import physics_scenes as ps
    from bench_physics import falling_bodies
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    out = dict(device=torch.cuda.get_device_name(0),
               timing="wall clock per way incl. packing, upload and read-back; kernels by HIP events in separate runs; the ways alternate",
               workloads=[measure(ps.DEFAULT, len(ps.DEFAULT["objects"]) - 1, 40, 64, args.reps,
                                  "default mod, 40 ticks, 64 variants: the player pushed once before tick k mod 40"),
                          measure(falling_bodies(64), 1, 30, 64, args.reps,
                                  "64 bodies of 12^3 onto a 128 x 128 slab, 30 ticks, 64 variants: the first pushed once before tick k mod 30")])
    text = json.dumps(out, indent=1)
    print(text, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
