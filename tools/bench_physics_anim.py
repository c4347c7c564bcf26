#!/usr/bin/env python3
"""Time T physics ticks with the sprites animated, in one process:

    (i)   DeviceWorld.run(clock=)          vrt_physics_run_anim: the schedule goes up with the bodies, the switches happen on
                                           the device at the switching body's turn
    (ii)  DeviceWorld.run(clock=) held     the same kernel with the clock standing at 0: the indirection without a switch
    (iii) DeviceWorld.run()                vrt_physics_run on the same scene: no animation at all (what (ii) costs over this is
                                           the indirection, what (i) costs over (ii) the switches and what they set in motion)
    (iv)  world.run(clock=)                the host path

on the scenes of tests/physics_anim_scenes.py and on N bodies of a blinking 12^3 sprite falling onto a 128 x 2 x 128 slab
(N = 16, 64; 30 ticks; the sprite's second frame is its lower half, and every body shows it, so a switch rewrites all of them).
Every run starts from the same state.  A route is timed by the wall clock from before its call until it returns (the device
routes end with a read-back): medians of --reps runs after one untimed run of each, the routes alternating.  The kernels alone
are timed by HIP events in runs of their own.  (i) and (iv) must end every run in the same state, bit for bit.
One JSON object goes to stdout and, with --out, to that file.  No threshold is set anywhere: nobody had measured these.

    python tools/bench_physics_anim.py --out profiles/physics_anim_bench.json
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

from bench_physics import series  # noqa: E402


def falling_blinkers(n, ticks):
    import physics_anim_scenes as an
    import physics_scenes as ps
    body = an.frames((12, 12, 12), [[an.box((0, 0, 0), (11, 11, 11), 1)], [an.box((0, 0, 0), (11, 5, 11), 1)]], (0, 1, 0.1))
    objects = [ps.obj("slab", (0, 0, 0), physics=False)]
    for i in range(n):
        layer, k = divmod(i, 64)
        objects.append(ps.obj("body", (-56 + 16 * (k % 8) + layer % 2, 10 + 16 * layer, -56 + 16 * (k // 8) + layer // 2),
                              vel=(0.25 * ((i % 5) - 2), 0, 0.125 * ((i % 3) - 1))))
    spec = ps.scene({"slab": ps.full((128, 2, 128), 0), "body": body}, objects, ticks, dist_move=10 ** 6, dist_max=10 ** 6, gravity=2.0 ** -6)
    spec["clock"] = [0, 50]
    return spec


class Run:
    """One scene, its objects built once; reset() puts them and the sprites back to the start."""

    def __init__(self, spec):
        import physics_anim_scenes as an
        from python_raytracer_amd.lib import vec3
        self.spec, self.vec3 = spec, vec3
        self.objects, self.sprites, _, self.st, self.who = an.project_scene(spec)
        self.cam = vec3(*spec["cam"])
        self.reset()

    def reset(self):
        for s in self.sprites.values():
            s.frame = 0
        for o, d in zip(self.objects, self.spec["objects"]):
            o.visible = False
            o.move(self.vec3(*[float(v) for v in d["pos"]]))
            o.vel = self.vec3(*[float(v) for v in d["vel"]])
            o.set_weight()

    def state(self):
        import numpy as np
        import physics_scenes as ps
        s = ps.state(self.objects)
        return (s["pos"].tobytes() + s["vel"].tobytes() + s["mins"].tobytes() + s["visible"].tobytes()
                + np.array([float(o.weight) for o in self.objects]).tobytes() + bytes(int(v.frame) for v in self.sprites.values()))


ROUTES = ("anim", "held", "plain", "host")


def measure(spec, reps, label):
    import torch
    from python_raytracer_amd import _native as nat
    from python_raytracer_amd import world
    from python_raytracer_amd.world import DeviceWorld
    run = Run(spec)
    dw = DeviceWorld(16)
    ticks, clock = spec["ticks"], tuple(spec["clock"])

    def go(route, **kw):
        if route == "anim":
            return dw.run(run.objects, run.cam, run.st, ticks, follow=run.who, clock=clock, **kw)
        if route == "held":
            return dw.run(run.objects, run.cam, run.st, ticks, follow=run.who, clock=(0, 0), **kw)
        if route == "plain":
            return dw.run(run.objects, run.cam, run.st, ticks, follow=run.who, **kw)
        return world.run(run.objects, run.cam, run.st, ticks, follow=run.who, clock=clock)

    ms, ends = {r: [] for r in ROUTES}, {r: set() for r in ROUTES}
    for rep in range(reps + 1):                       # (the first run of each route uploads the models: untimed)
        for route in ROUTES if rep % 2 == 0 else ROUTES[::-1]:
            run.reset()
            t0 = time.perf_counter()
            go(route)
            took = (time.perf_counter() - t0) * 1e3
            if rep:
                ms[route].append(took)
            ends[route].add(run.state())
    assert all(len(e) == 1 for e in ends.values()) and ends["anim"] == ends["host"], "the device and the host disagree"
    assert ends["held"] == ends["plain"], "a held clock changed something"
    kernel, work, switches = {}, {}, 0
    for route in ROUTES[:3]:                          # the kernels alone, in runs of their own
        run.reset()
        r = go(route, budget=1 << 40, time_kernel=True)
        torch.cuda.synchronize()
        assert r.launches == 1
        kernel[route], work[route] = round(r.kernel_ms, 4), int(r.stats[nat.S_PHYSICS_WORK])
        if route == "anim":
            switches = int((r.records["pad"][:, 0] & nat.BODY_EVER_SWITCHED != 0).sum())
    med = {r: statistics.median(ms[r]) for r in ROUTES}
    return dict(workload=label, bodies=len(run.objects), ticks=ticks, clock=list(clock),
                run_clock_ms=series(ms["anim"]), run_clock_held_ms=series(ms["held"]), run_ms=series(ms["plain"]), host_run_clock_ms=series(ms["host"]),
                run_clock_over_run=round(med["anim"] / med["plain"], 3), host_over_run_clock=round(med["host"] / med["anim"], 3),
                kernel_ms_one_launch=dict(run_clock=kernel["anim"], run_clock_held=kernel["held"], run=kernel["plain"]),
                held_kernel_over_run_kernel=round(kernel["held"] / kernel["plain"], 3),
                work_units=dict(run_clock=work["anim"], run_clock_held=work["held"], run=work["plain"]),
                bodies_that_switched=switches, device_and_host_agree=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5, help="timed runs of each route per workload")
    ap.add_argument("--ticks", type=int, default=30, help="ticks of the falling-bodies runs")
    ap.add_argument("--out", default="", help="write the JSON object to this file")
    args = ap.parse_args()
    import torch
    import physics_anim_scenes as an
    out = dict(device=torch.cuda.get_device_name(0),
               timing="wall clock of T ticks incl. host work, uploads and read-backs, medians of %d after an untimed run, routes "
                      "alternating; kernels by HIP events in separate runs of one launch each" % args.reps,
               workloads=[measure(json.loads(json.dumps(an.SCENES[n])), args.reps, "scene `%s`" % n) for n in ("platform", "weights", "wake", "crowd")])
    for n in (16, 64):
        out["workloads"].append(measure(falling_blinkers(n, args.ticks), args.reps, "%d blinking bodies of 12^3 onto a 128 x 128 slab" % n))
    text = json.dumps(out, indent=1)
    print(text, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
