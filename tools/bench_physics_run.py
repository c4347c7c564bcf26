#!/usr/bin/env python3
"""Time T physics ticks by the two device routes there are, in one process:

    (i)  DeviceWorld.run(ticks=T)     the body records go up once, vrt_physics_run steps them T times on the device (flags,
                                      validation and the tick's chain; as many launches as the work budget asks for), the records
                                      come back once
    (ii) T x DeviceWorld.tick         one upload, one vrt_physics_tick launch and one read-back per tick, the flags worked out
                                      on the host: the only route there was

on the workloads of tools/bench_physics.py: the default mod's 40 ticks, and N 12^3 bodies falling onto a 128 x 2 x 128 slab
(N = 16, 64, 256; 30 ticks).  Every run starts from the same state.  A route is timed by the wall clock from before its first
call until its last returns (both end with a read-back, so the device has finished): medians of --reps runs after one untimed
run of each, the routes alternating.  The kernels alone are timed by HIP events in runs of their own; the run's in ONE launch
(an unbounded budget), which also gives the cost of a work unit -- kernel time / VRT_S_PHYSICS_WORK -- that the default budget
is derived from.  Both routes must end every run in the same state, bit for bit.
One JSON object goes to stdout and, with --out, to that file.  No threshold is set anywhere: nobody had measured these.

    python tools/bench_physics_run.py --out profiles/physics_run_bench.json
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

from bench_physics import Run, falling_bodies, series  # noqa: E402

TARGET_MS, SPARE = 50.0, 2.0      # what the default budget is to keep a launch of the slowest workload near, and the room left


def measure(spec, ticks, reps, label):
    import torch
    from python_raytracer_amd import _native as nat
    from python_raytracer_amd.world import DeviceWorld
    run = Run(spec)
    dw = DeviceWorld(16)
    run_ms, loop_ms, ends, launches = [], [], set(), set()
    for rep in range(reps + 1):                       # (the first run of each route uploads the models: untimed)
        for route in ("run", "loop") if rep % 2 == 0 else ("loop", "run"):
            run.reset()
            t0 = time.perf_counter()
            if route == "run":
                r = dw.run(run.objects, run.cam, run.st, ticks)
                launches.add(r.launches)
            else:
                for k in range(ticks):
                    dw.tick(run.objects, run.cam, run.st)
            ms = (time.perf_counter() - t0) * 1e3
            if rep:
                (run_ms if route == "run" else loop_ms).append(ms)
            ends.add(run.state())
    assert len(ends) == 1, "the two routes disagree"
    # the kernels alone, in runs of their own
    run.reset()
    r = dw.run(run.objects, run.cam, run.st, ticks, budget=1 << 40, time_kernel=True)
    assert r.launches == 1 and run.state() in ends
    stats = r.stats
    run.reset()
    tick_kernel = sum(dw.tick(run.objects, run.cam, run.st, time_kernel=True).kernel_ms for k in range(ticks))
    assert run.state() in ends
    run.reset()
    shipped = dw.run(run.objects, run.cam, run.st, ticks, time_kernel=True)
    torch.cuda.synchronize()
    work = int(stats[nat.S_PHYSICS_WORK])
    a, b = statistics.median(run_ms), statistics.median(loop_ms)
    return dict(workload=label, bodies=len(run.objects), ticks=ticks, run_ms=series(run_ms), tick_loop_ms=series(loop_ms),
                tick_loop_over_run=round(b / a, 3), run_kernel_ms_one_launch=round(r.kernel_ms, 4), tick_loop_kernel_ms=round(tick_kernel, 4),
                work_units=work, us_per_work_unit=round(r.kernel_ms * 1e3 / work, 4),
                launches_at_default_budget=sorted(launches), kernel_ms_at_default_budget=round(shipped.kernel_ms, 4),
                mean_launch_ms_at_default_budget=round(shipped.kernel_ms / shipped.launches, 4),
                per_run=dict(stepped=int(stats[nat.S_PHYSICS_BODIES]), steps=int(stats[nat.S_PHYSICS_STEPS]),
                             blocked=int(stats[nat.S_PHYSICS_BLOCKED]), contacts=int(stats[nat.S_PHYSICS_CONTACTS]),
                             transfers=int(stats[nat.S_PHYSICS_TRANSFERS]), capped=int(stats[nat.S_PHYSICS_CAPPED])),
                routes_agree=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5, help="timed runs of each route per workload")
    ap.add_argument("--ticks", type=int, default=30, help="ticks of the falling-bodies runs")
    ap.add_argument("--out", default="", help="write the JSON object to this file")
    args = ap.parse_args()
    import torch
    import physics_scenes as ps
    from python_raytracer_amd import _native as nat
    out = dict(device=torch.cuda.get_device_name(0),
               timing="wall clock of T ticks incl. host work, uploads and read-backs, medians of %d after an untimed run, routes "
                      "alternating; kernels by HIP events in separate runs" % args.reps,
               workloads=[measure(ps.DEFAULT, 40, args.reps, "default mod, 40 ticks")])
    for n in (16, 64, 256):
        out["workloads"].append(measure(falling_bodies(n), args.ticks, args.reps, "%d bodies of 12^3 onto a 128 x 128 slab" % n))
    worst = max(w["us_per_work_unit"] for w in out["workloads"])
    out["budget"] = dict(shipped=nat.PHYSICS_RUN_BUDGET, worst_us_per_work_unit=worst, target_ms=TARGET_MS, spare_factor=SPARE,
                         units_for_target=int(TARGET_MS / SPARE * 1e3 / worst),
                         arithmetic="budget <= target_ms / spare_factor * 1000 / worst_us_per_work_unit, rounded down to a power of two")
    text = json.dumps(out, indent=1)
    print(text, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
