#!/usr/bin/env python3
"""Time K futures of one world under K seeds by the two routes there are, in one process:

    (i)  DeviceWorld.run_many(rng=)  the bodies are packed once and replicated K times, the K generators go up as one [K][625]
                                     block; one launch of K workgroups (vrt_physics_run_batch_draws) steps them all; one read-back
    (ii) the loop it replaces        K times DeviceWorld.run(rng=) on a fresh twin of the objects with a copy of the seed's generator
                                     (twins and copies are made before the clock starts: the loop is charged for its runs alone)

on two workloads with fractional solidity: `wade` without its clock, the camera following (tests/physics_run_draw_scenes.py, 20
ticks), and `fluid` (tests/physics_draw_scenes.py, 24 ticks, about 1150 draws a tick); K = 1, 16, 64, 256, seeds 0 .. K - 1.  Before
anything is timed both routes must end every future in the same bytes: the records and the generator's 625 words.
A route is timed by the wall clock from before the call until it returns, packing and copies included (both end with a read-back,
so the device has finished); after one untimed run of each route the routes alternate, and the medians of --reps runs are
reported.  The kernels alone are timed by HIP events (time_kernel=True) in runs of their own.
One JSON object goes to stdout and, with --out, to that file.  No ratio is fixed in advance: run(rng=) is what it was, and nobody
had measured the batch.

    python tools/bench_physics_run_many_draws.py --out profiles/physics_batch_draws_bench.json
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

KS = (1, 16, 64, 256)


def copy_of(g):
    c = random.Random()
    c.setstate(g.getstate())
    return c


def measure(objects, st, cam, who, ticks, reps, label):
    import physics_batch_util as bu
    from python_raytracer_amd.world import DeviceWorld
    dw, dw_loop = DeviceWorld(16), DeviceWorld(16)
    at = objects.index(who) if who is not None else None

    def twins(gens):
        out = []
        for g in gens:
            twin = bu.twins(objects)
            out.append((twin, twin[at] if at is not None else None, copy_of(g)))
        return out

    def loop(made, **more):
        return [dw_loop.run(twin, cam, st, ticks, follow=follow, rng=g, **more) for twin, follow, g in made]

    rows = []
    for K in KS:
        gens = [random.Random(seed) for seed in range(K)]
        variants = [{}] * K
        # both routes end in the same bytes (and this is the untimed run of each)
        r = dw.run_many(objects, cam, st, ticks, variants, follow=who, rng=gens)
        made = twins(gens)
        for k, t in enumerate(loop(made)):
            assert r.records[k].tobytes() == t.records.tobytes(), "the two routes disagree at future %d of %d (%s)" % (k, K, label)
            assert r.rng_state(k) == made[k][2].getstate(), "the two routes leave other generators at future %d of %d (%s)" % (k, K, label)
        batch_ms, loop_ms = [], []
        for rep in range(reps):
            t0 = time.perf_counter()
            r = dw.run_many(objects, cam, st, ticks, variants, follow=who, rng=gens)
            batch_ms.append((time.perf_counter() - t0) * 1e3)
            made = twins(gens)
            t0 = time.perf_counter()
            loop(made)
            loop_ms.append((time.perf_counter() - t0) * 1e3)
        batch_kernel = [dw.run_many(objects, cam, st, ticks, variants, follow=who, rng=gens, time_kernel=True).kernel_ms for rep in range(reps)]
        loop_kernel = sum(t.kernel_ms for t in loop(twins(gens), time_kernel=True))
        draws = r.draws.astype(float)
        row = dict(K=K, launches=int(r.launches), run_many_ms=round(statistics.median(batch_ms), 3), loop_of_runs_ms=round(statistics.median(loop_ms), 3),
                   run_many_kernel_ms=round(statistics.median(batch_kernel), 3), loop_kernels_ms=round(loop_kernel, 3), samples=reps,
                   draws_min=int(draws.min()), draws_max=int(draws.max()), distinct_futures=len({r.records[k].tobytes() for k in range(K)}))
        row["loop_over_run_many"] = round(row["loop_of_runs_ms"] / row["run_many_ms"], 2)
        row["run_many_ms_per_future"] = round(row["run_many_ms"] / K, 4)
        row["one_run_kernel_ms"] = round(loop_kernel / K, 3)
        rows.append(row)
        print(label, row, file=sys.stderr, flush=True)
    return dict(workload=label, bodies=len(objects), ticks=ticks, rows=rows, routes_agree=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3, help="timed runs of either route per K")
    ap.add_argument("--out", default="", help="write the JSON object to this file")
    args = ap.parse_args()
    import torch
    import physics_run_draw_scenes as rd
    import physics_scenes as ps
    from python_raytracer_amd.lib import vec3
    _, wade, objects, _, st, who = rd.fresh("wade")
    workloads = [measure(objects, st, vec3(*wade["cam"]), who, wade["ticks"], args.reps, "wade without its clock, 20 ticks, the camera follows")]
    _, fluid = ps.load_fixture("fluid")
    objects, _, _, st = ps.project_scene(fluid)
    ps.clear_redraw(objects)
    workloads.append(measure(objects, st, vec3(*fluid["cam"]), None, fluid["ticks"], args.reps, "fluid, 24 ticks"))
    out = dict(device=torch.cuda.get_device_name(0),
               timing="wall clock per call incl. packing, copies, upload and read-back, medians of %d after an untimed run of each route, the "
                      "routes alternating; kernels by HIP events in separate runs" % args.reps,
               futures="K runs of the world as it stands ({}) under seeds 0 .. K - 1", workloads=workloads)
    text = json.dumps(out, indent=1)
    print(text, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
