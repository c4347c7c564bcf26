#!/usr/bin/env python3
"""Time T physics ticks WITH the reference's random draws by the routes there are, in one process:

    (i)   DeviceWorld.run(ticks=T, rng=)   the body records and the generator's 625 words go up once, vrt_physics_run_draws steps the
                                           bodies T times on the device (as many launches as the work budget asks for), records and
                                           generator come back once
    (ii)  T x DeviceWorld.tick(rng=)       one upload, one vrt_physics_tick_draws launch and one read-back of bodies and generator
                                           per tick, the flags (and a followed camera) worked out on the host: the route there was
    (iii) world.run(ticks=T, rng=)         the host path (timed --host-reps times: it is slow)
    (iv)  DeviceWorld.run(ticks=T)         the all-solid rows only: the run without draws, vrt_physics_run

on `fluid` (tests/physics_draw_scenes.py, 24 ticks), `wade` (tests/physics_run_draw_scenes.py: the camera rides on a body) and the
16 + 1 and 64 + 1 all-solid falling bodies of tools/bench_physics.py with a generator.  Every run starts from the same state and
the same seed.  The method is tools/bench_physics_run.py's: wall clock from before a route's first call until its last returns,
medians of --reps runs after one untimed run of each, the device routes alternating; the kernels alone by HIP events in runs of
their own, the run's in ONE launch (an unbounded budget), which gives the cost of a work unit.  Routes (i), (ii) and (iii) must end
every run in the same state and the same generator, bit for bit; (iv) in the same state.
One JSON object goes to stdout and, with --out, to that file.  No threshold is set anywhere.

    python tools/bench_physics_run_draws.py --out profiles/physics_run_draws_bench.json
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

from bench_physics import Run, falling_bodies, series  # noqa: E402

TARGET_MS, SPARE = 50.0, 2.0      # as tools/bench_physics_run.py: a launch of the slowest workload stays near target / spare


class FollowRun(Run):
    """A scene of tests/physics_anim_scenes.py's vocabulary: one body may carry the camera."""

    def __init__(self, spec):
        import physics_anim_scenes as an
        from python_raytracer_amd.lib import vec3
        self.spec, self.vec3 = spec, vec3
        self.objects, _, _, self.st, self.who = an.project_scene(spec)
        self.cam = vec3(*spec["cam"])
        self.reset()


def measure(run, ticks, reps, host_reps, label, seed, solid):
    import torch
    from python_raytracer_amd import _native as nat
    from python_raytracer_amd import world
    from python_raytracer_amd.world import DeviceWorld
    who = getattr(run, "who", None)
    dw = DeviceWorld(16)

    def loop(gen, time_kernel=False):
        ms = 0.0
        for k in range(ticks):
            r = dw.tick(run.objects, who.cam_pos if who is not None else run.cam, run.st, rng=gen, time_kernel=time_kernel)
            if who is not None:
                who.set_camera_pos()
            ms += r.kernel_ms or 0.0
        return ms

    times = dict(run=[], loop=[], plain=[])
    ends, gens, launches = set(), set(), set()
    routes = ("run", "loop") + (("plain",) if solid else ())
    for rep in range(reps + 1):                       # (the first run of each route uploads the models: untimed)
        for route in routes if rep % 2 == 0 else routes[::-1]:
            run.reset()
            gen = random.Random(seed)
            t0 = time.perf_counter()
            if route == "run":
                launches.add(dw.run(run.objects, run.cam, run.st, ticks, follow=who, rng=gen).launches)
            elif route == "loop":
                loop(gen)
            else:
                dw.run(run.objects, run.cam, run.st, ticks, follow=who)
            ms = (time.perf_counter() - t0) * 1e3
            if rep:
                times[route].append(ms)
            ends.add(run.state())
            if route != "plain":
                gens.add(gen.getstate())
    host_ms = []
    for rep in range(host_reps):
        run.reset()
        gen = random.Random(seed)
        t0 = time.perf_counter()
        world.run(run.objects, run.cam, run.st, ticks, follow=who, rng=gen.random)
        host_ms.append((time.perf_counter() - t0) * 1e3)
        ends.add(run.state()), gens.add(gen.getstate())
    assert len(ends) == 1 and len(gens) == 1, "the routes disagree"
    # the kernels alone, in runs of their own
    run.reset()
    r = dw.run(run.objects, run.cam, run.st, ticks, follow=who, rng=random.Random(seed), budget=1 << 40, time_kernel=True)
    assert r.launches == 1 and run.state() in ends
    stats = r.stats
    run.reset()
    tick_kernel = loop(random.Random(seed), time_kernel=True)
    assert run.state() in ends
    run.reset()
    shipped = dw.run(run.objects, run.cam, run.st, ticks, follow=who, rng=random.Random(seed), time_kernel=True)
    torch.cuda.synchronize()
    work = int(stats[nat.S_PHYSICS_WORK])
    a, b = statistics.median(times["run"]), statistics.median(times["loop"])
    out = dict(workload=label, bodies=len(run.objects), ticks=ticks, draws=r.draws, run_rng_ms=series(times["run"]),
               tick_rng_loop_ms=series(times["loop"]), tick_loop_over_run=round(b / a, 3),
               host_run_rng_ms=series(host_ms) if host_ms else None,
               run_kernel_ms_one_launch=round(r.kernel_ms, 4), tick_loop_kernel_ms=round(tick_kernel, 4),
               work_units=work, us_per_work_unit=round(r.kernel_ms * 1e3 / work, 4),
               launches_at_default_budget=sorted(launches), kernel_ms_at_default_budget=round(shipped.kernel_ms, 4),
               mean_launch_ms_at_default_budget=round(shipped.kernel_ms / shipped.launches, 4),
               per_run=dict(stepped=int(stats[nat.S_PHYSICS_BODIES]), steps=int(stats[nat.S_PHYSICS_STEPS]),
                            blocked=int(stats[nat.S_PHYSICS_BLOCKED]), contacts=int(stats[nat.S_PHYSICS_CONTACTS]),
                            transfers=int(stats[nat.S_PHYSICS_TRANSFERS]), capped=int(stats[nat.S_PHYSICS_CAPPED])),
               routes_agree=True)
    if solid:
        run.reset()
        p = dw.run(run.objects, run.cam, run.st, ticks, follow=who, budget=1 << 40, time_kernel=True)
        out.update(run_without_rng_ms=series(times["plain"]), run_rng_over_run_without=round(a / statistics.median(times["plain"]), 3),
                   run_without_rng_kernel_ms_one_launch=round(p.kernel_ms, 4), run_without_rng_work_units=int(p.stats[nat.S_PHYSICS_WORK]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5, help="timed runs of each device route per workload")
    ap.add_argument("--host-reps", type=int, default=1, help="timed runs of the host route per workload")
    ap.add_argument("--ticks", type=int, default=30, help="ticks of the falling-bodies runs")
    ap.add_argument("--out", default="", help="write the JSON object to this file")
    args = ap.parse_args()
    import torch
    import physics_draw_scenes as pds
    import physics_run_draw_scenes as rd
    from python_raytracer_amd import _native as nat
    out = dict(device=torch.cuda.get_device_name(0),
               timing="wall clock of T ticks incl. host work, uploads and read-backs, medians of %d after an untimed run, device routes "
                      "alternating; host route %d run(s); kernels by HIP events in separate runs" % (args.reps, args.host_reps),
               workloads=[measure(Run(pds.FLUID), pds.FLUID["ticks"], args.reps, args.host_reps, "fluid, 24 ticks", pds.SEED, False),
                          measure(FollowRun(rd.SCENES["wade"]), rd.SCENES["wade"]["ticks"], args.reps, args.host_reps,
                                  "wade, 20 ticks, the camera follows", rd.SCENES["wade"]["seed"], False)])
    for n in (16, 64):
        out["workloads"].append(measure(Run(falling_bodies(n)), args.ticks, args.reps, args.host_reps,
                                        "%d bodies of 12^3 onto a 128 x 128 slab, all solid, with a generator" % n, 11, True))
    worst = max(w["us_per_work_unit"] for w in out["workloads"])
    units = int(TARGET_MS / SPARE * 1e3 / worst)
    out["budget"] = dict(shipped=nat.PHYSICS_RUN_DRAWS_BUDGET, worst_us_per_work_unit=worst, target_ms=TARGET_MS, spare_factor=SPARE,
                         units_for_target=units, power_of_two=1 << (units.bit_length() - 1),
                         arithmetic="budget <= target_ms / spare_factor * 1000 / worst_us_per_work_unit, rounded down to a power of two")
    text = json.dumps(out, indent=1)
    print(text, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
