#!/usr/bin/env python3
"""Time the physics tick that makes the reference's random draws (DeviceWorld.tick(rng=), vrt_physics_tick_draws), in one process:

    fluid            the scene of tests/physics_draw_scenes.py (fractional solidities; 24 ticks, about 1400 draws a tick):
                     DeviceWorld.tick(rng=) against world.tick(rng=), the only route there was for such a world
    fluid, decided   the same scene with every fractional solidity rounded (0.25 -> 0, 0.5 and 0.75 -> 1), so no test waits for
                     its own first draw: the drawing tick against the tick that makes no draws.  With `fluid` this splits the
                     kernel's time: no draws -> draws (classes, prefix sums, regeneration) -> undecided tests (the serial walk)
    16 + 1, 256 + 1  the all-solid falling bodies of tools/bench_physics.py: the drawing tick against the tick that makes no draws
                     -- what the draws cost where they decide nothing

Every run starts from the same state and the same seed; a tick is timed by the wall clock from before the call until it returns
(DeviceWorld.tick ends with the read-back), the kernel alone by HIP events in runs of their own.  The routes compared must end
every run in the same state, bit for bit, and the generator where CPython's is after as many random() calls as the ticks counted
(fluid: where world.tick left its own).  One JSON object goes to stdout and, with --out, to that file.  No threshold is set.

    python tools/bench_physics_draws.py --out profiles/physics_draws_bench.json
"""
import argparse
import copy
import json
import os
import random
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_physics import Run, falling_bodies, series  # noqa: E402

SEED = 20261


def device_runs(run, dw, ticks, reps, seeded):
    """reps timed runs of `ticks` device ticks (after an untimed one), then one with the kernel timed by events.  Returns
    (per-tick wall ms [reps][ticks], per-tick kernel ms, summed statistics, end state, generator at the end or None)."""
    wall, gen = [], None
    for rep in range(reps + 1):
        run.reset()
        gen = random.Random(SEED) if seeded else None
        per = []
        for k in range(ticks):
            t0 = time.perf_counter()
            run_tick(dw, run, gen)
            per.append((time.perf_counter() - t0) * 1e3)
        if rep:
            wall.append(per)
        end = run.state()
    run.reset()
    gen = random.Random(SEED) if seeded else None
    kernel, totals = [], np.zeros(16, np.int64)
    for k in range(ticks):
        r = run_tick(dw, run, gen, time_kernel=True)
        kernel.append(r.kernel_ms)
        totals += r.stats
    assert run.state() == end
    return wall, kernel, totals, end, gen


def run_tick(dw, run, gen, time_kernel=False):
    if gen is None:
        return dw.tick(run.objects, run.cam, run.st, time_kernel=time_kernel)
    return dw.tick(run.objects, run.cam, run.st, rng=gen, time_kernel=time_kernel)


def counts(totals):
    from python_raytracer_amd import _native as nat
    return dict(stepped=int(totals[nat.S_PHYSICS_BODIES]), steps=int(totals[nat.S_PHYSICS_STEPS]), blocked=int(totals[nat.S_PHYSICS_BLOCKED]),
                contacts=int(totals[nat.S_PHYSICS_CONTACTS]), transfers=int(totals[nat.S_PHYSICS_TRANSFERS]),
                draws=int(totals[nat.S_PHYSICS_DRAWS]), generator_states=round(int(totals[nat.S_PHYSICS_DRAWS]) * 2 / 624, 1))


def after_draws(n):
    gen = random.Random(SEED)
    for _ in range(n):
        gen.random()
    return gen.getstate()


def measure_fluid(spec, ticks, reps):
    """The drawing tick against the host path with the same seed."""
    from python_raytracer_amd import world
    from python_raytracer_amd.world import DeviceWorld
    run = Run(spec)
    wall, kernel, totals, end, gen = device_runs(run, DeviceWorld(16), ticks, reps, True)
    host_ms = []
    for rep in range(2):
        run.reset()
        twin = random.Random(SEED)
        per = []
        for k in range(ticks):
            t0 = time.perf_counter()
            world.tick(run.objects, run.cam, run.st, rng=twin.random)
            per.append((time.perf_counter() - t0) * 1e3)
        host_ms.append(per)
        assert run.state() == end, "the two routes disagree"
        assert twin.getstate() == gen.getstate() == after_draws(counts(totals)["draws"]), "the generators disagree"
    dev, host = np.array(wall), np.array(host_ms)
    return dict(workload="fluid, %d ticks" % ticks, bodies=len(run.objects), ticks=ticks,
                device_tick_ms=series(dev.reshape(-1).tolist()), device_run_ms=series(dev.sum(1).tolist()),
                kernel_tick_ms_hip_events=series(kernel), kernel_run_ms=round(sum(kernel), 4),
                host_tick_ms=series(host.reshape(-1).tolist()), host_run_ms=series(host.sum(1).tolist()),
                per_run=counts(totals), routes_agree=True)


def measure_pair(spec, ticks, reps, label):
    """The drawing tick against the tick that makes no draws, alternating, on a world without fractional solidity."""
    from python_raytracer_amd.world import DeviceWorld
    run, dw = Run(spec), DeviceWorld(16)
    out = dict(workload=label, bodies=len(run.objects), ticks=ticks)
    ends = []
    for name, seeded in (("no_draws", False), ("draws", True), ("no_draws_again", False), ("draws_again", True)):
        wall, kernel, totals, end, gen = device_runs(run, dw, ticks, reps, seeded)
        dev = np.array(wall)
        out[name] = dict(device_tick_ms=series(dev.reshape(-1).tolist()), device_run_ms=series(dev.sum(1).tolist()),
                         kernel_tick_ms_hip_events=series(kernel), kernel_run_ms=round(sum(kernel), 4), per_run=counts(totals))
        ends.append(end)
        if seeded:
            assert gen.getstate() == after_draws(out[name]["per_run"]["draws"]), "the generator is not where CPython's is"
    assert len(set(ends)) == 1, "the two routes disagree"
    out["routes_agree"] = True
    return out


def decided(spec):
    """The scene with every fractional solidity rounded to 0 or 1."""
    spec = copy.deepcopy(spec)
    for m in spec["materials"]:
        if 0 < m["solidity"] < 1:
            m["solidity"] = 0 if m["solidity"] < 0.5 else 1
    return spec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5, help="timed runs per route and workload")
    ap.add_argument("--ticks", type=int, default=30, help="ticks of the falling-bodies runs")
    ap.add_argument("--out", default="", help="write the JSON object to this file")
    args = ap.parse_args()
    import torch
    import physics_draw_scenes as pds
    fluid = pds.SCENES["fluid"]
    out = dict(device=torch.cuda.get_device_name(0),
               timing="wall clock per tick incl. host work, upload and read-back; kernel by HIP events in separate runs",
               workloads=[measure_fluid(fluid, fluid["ticks"], args.reps),
                          measure_pair(decided(fluid), fluid["ticks"], args.reps, "fluid, decided (no fractional solidity), %d ticks" % fluid["ticks"])])
    for n in (16, 256):
        out["workloads"].append(measure_pair(falling_bodies(n), args.ticks, args.reps, "%d bodies of 12^3 onto a 128 x 128 slab" % n))
    text = json.dumps(out, indent=1)
    print(text, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
