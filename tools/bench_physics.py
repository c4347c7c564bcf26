#!/usr/bin/env python3
"""Time one physics tick by the two routes there are, in one process:

    (i)  DeviceWorld.tick   the body records go up, one vrt_physics_tick launch runs the reference's sequential chain on the
                            resident models, the records come back and are written into the Objects
    (ii) world.tick         the host path: the reference's Python loops, restated (Object.update_physics)

on two workloads: the default mod (tests/physics_scenes.py: the castle, six material cubes, the player; the 40 ticks of
tests/golden/physics_default.npz, in which the player falls 22 voxels and lands), and N 12^3 bodies in layers of 8 x 8 falling
onto a 128 x 2 x 128 slab (N = 16, 64, 256: how the tick scales with the body count -- the chain is sequential by the
reference's semantics).  Every run starts from the same state; a tick is timed by the wall clock from before the call until it
returns (DeviceWorld.tick ends with the read-back, so the device has finished), and the kernel alone by HIP events
(DeviceWorld.tick(time_kernel=True), in runs of their own).  Both routes must end every run in the same state, bit for bit.
One JSON object goes to stdout and, with --out, to that file.  No threshold is set anywhere: nobody had measured these.

    python tools/bench_physics.py --out profiles/physics_bench.json
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def series(v):
    med = statistics.median(v)
    q = statistics.quantiles(v, n=4) if len(v) > 1 else [med, med, med]
    return dict(median_ms=round(med, 4), min_ms=round(min(v), 4), max_ms=round(max(v), 4),
                iqr_over_median=round((q[2] - q[0]) / med, 4) if med else 0.0, samples=len(v))


def falling_bodies(n):
    import physics_scenes as ps
    objects = [ps.obj("slab", (0, 0, 0), physics=False)]
    for i in range(n):
        layer, k = divmod(i, 64)
        objects.append(ps.obj("body", (-56 + 16 * (k % 8) + layer % 2, 10 + 16 * layer, -56 + 16 * (k // 8) + layer // 2),
                              vel=(0.25 * ((i % 5) - 2), 0, 0.125 * ((i % 3) - 1))))
    return ps.scene({"slab": ps.full((128, 2, 128), 0), "body": ps.full((12, 12, 12), 1)}, objects, 0, dist_move=10 ** 6, dist_max=10 ** 6,
                    gravity=2.0 ** -6)


class Run:
    """One scene, its objects built once; reset() puts them back to the start."""

    def __init__(self, spec):
        import physics_scenes as ps
        from python_raytracer_amd.lib import vec3
        self.spec, self.vec3 = spec, vec3
        self.objects, _, _, self.st = ps.project_scene(spec)
        self.cam = vec3(*spec["cam"])
        self.reset()

    def reset(self):
        for o, d in zip(self.objects, self.spec["objects"]):
            o.visible = False
            o.move(self.vec3(*[float(v) for v in d["pos"]]))
            o.vel = self.vec3(*[float(v) for v in d["vel"]])

    def state(self):
        import physics_scenes as ps
        s = ps.state(self.objects)
        return s["pos"].tobytes() + s["vel"].tobytes() + s["mins"].tobytes() + s["visible"].tobytes()


def measure(spec, ticks, host_ticks, reps, label):
    import torch
    from python_raytracer_amd import world
    from python_raytracer_amd.world import DeviceWorld
    run = Run(spec)
    dw = DeviceWorld(16)
    dev_ms, kernel_ms, counts = [], [], None
    for rep in range(reps + 1):                       # (the first run uploads the models: untimed)
        run.reset()
        per = []
        for k in range(ticks):
            t0 = time.perf_counter()
            r = dw.tick(run.objects, run.cam, run.st)
            per.append((time.perf_counter() - t0) * 1e3)
        if rep:
            dev_ms.append(per)
        end = run.state()
    run.reset()
    totals = np.zeros(16, np.int64)
    for k in range(ticks):
        r = dw.tick(run.objects, run.cam, run.st, time_kernel=True)
        kernel_ms.append(r.kernel_ms)
        totals += r.stats
    assert run.state() == end
    torch.cuda.synchronize()
    run.reset()
    host_ms = []
    for k in range(host_ticks):
        t0 = time.perf_counter()
        world.tick(run.objects, run.cam, run.st)
        host_ms.append((time.perf_counter() - t0) * 1e3)
    if host_ticks == ticks:
        assert run.state() == end, "the two routes disagree"
    dev = np.array(dev_ms)
    from python_raytracer_amd import _native as nat
    return dict(workload=label, bodies=len(run.objects), ticks=ticks, host_ticks=host_ticks,
                device_tick_ms=series(dev.reshape(-1).tolist()), device_run_ms=series(dev.sum(1).tolist()),
                kernel_tick_ms_hip_events=series(kernel_ms), kernel_run_ms=round(sum(kernel_ms), 4),
                host_tick_ms=series(host_ms), host_run_ms=round(sum(host_ms), 3),
                per_run=dict(stepped=int(totals[nat.S_PHYSICS_BODIES]), steps=int(totals[nat.S_PHYSICS_STEPS]),
                             blocked=int(totals[nat.S_PHYSICS_BLOCKED]), contacts=int(totals[nat.S_PHYSICS_CONTACTS]),
                             transfers=int(totals[nat.S_PHYSICS_TRANSFERS]), capped=int(totals[nat.S_PHYSICS_CAPPED])),
                routes_agree=bool(host_ticks == ticks))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5, help="timed runs of the device route per workload")
    ap.add_argument("--ticks", type=int, default=30, help="ticks of the falling-bodies runs")
    ap.add_argument("--host-ticks", type=int, default=30, help="ticks the host route runs of the 256-body workload (it is slow)")
    ap.add_argument("--out", default="", help="write the JSON object to this file")
    args = ap.parse_args()
    import torch
    import physics_scenes as ps
    out = dict(device=torch.cuda.get_device_name(0),
               timing="wall clock per tick incl. host work, upload and read-back; kernel by HIP events in separate runs",
               workloads=[measure(ps.DEFAULT, 40, 40, args.reps, "default mod, 40 ticks")])
    for n in (16, 64, 256):
        out["workloads"].append(measure(falling_bodies(n), args.ticks, args.host_ticks if n == 256 else args.ticks, args.reps,
                                        "%d bodies of 12^3 onto a 128 x 128 slab" % n))
    text = json.dumps(out, indent=1)
    print(text, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
