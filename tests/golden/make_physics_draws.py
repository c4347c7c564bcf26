#!/usr/bin/env python3
"""Generate tests/golden/physics_fluid.npz: the reference's own physics on the scene of tests/physics_draw_scenes.py, a world
with materials of fractional solidity, with its random draws seeded and counted.

The arrays are those of the other physics fixtures (make_physics.py, whose run_reference and run_host do the runs) plus
    draws              int64 [ticks]                 random.random() calls of the tick: the reference's data.py calls the
                                                     module function, which is wrapped while its run lasts
Nothing of the reference is copied: its modules are imported in place and its Object.update is called and observed.

The file is written only if
  (a) the reference, this project's host path (world.tick with random.Random(seed).random) and the host path restricted to what
      the device holds agree in every recorded field bit for bit, and in the draws of every tick;
  (b) some pass of 1024 tests (the device's unit: tests i * 1024 .. i * 1024 + 1023 of a step, in the reference's loop order) holds
      tests of all four classes -- no draw, one, two, one-or-two (vrt_physics_draws.hip);
  (c) the draws of some pass come from two states of the generator (its outputs cross a multiple of 624);
  (d) some step has more than 1024 tests and contacts beyond the first pass;
  (e) tests that make one or two draws went both ways;
  (f) another seed changes a recorded field.
`reached` in the file (JSON) says how often each was met, besides the counts make_physics.py keeps.

The classes are observed from inside the host path's loop, which restates the reference's statement for statement: the draw
function handed to world.tick looks at the loop's variables (the test's number in the step, both materials).

Usage:  python tests/golden/make_physics_draws.py
"""
import json
import os
import random
import sys

import numpy as np

import make_physics as mp
from make_golden import load_reference

OUT = os.path.dirname(os.path.abspath(__file__))
PASS = 1024      # tests the device classifies at a time (vrt_physics_draws.hip, VRT_PHYS_BLOCK)
STATE = 624      # outputs per state of the generator; a draw takes two


def run_counted(data, lib, spec):
    """make_physics.run_reference with the module function random.random counted per tick."""
    made, per_tick = [0], []
    real, observe = random.random, mp.observe

    def counted():
        made[0] += 1
        return real()

    def observed(objects, rec):
        per_tick.append(made[0] - sum(per_tick))
        observe(objects, rec)

    random.random, mp.observe = counted, observed
    outside = []
    try:
        ref = mp.run_reference(data, lib, spec, outside)
    finally:
        random.random, mp.observe = real, observe
    return ref, np.array(per_tick, np.int64), outside


def run_classes(spec, seed):
    """The host path with a draw function that watches the loop it is called from.  Returns (arrays, draws per tick, passes):
    passes maps (tick, object, step, pass) to dict(flats: the tests of the pass that drew, one/two/open_pass/open_fail: how many of
    each class, first/last: the generator's output positions the pass used, counted from the seeding)."""
    import physics_scenes as ps
    from python_raytracer_amd import Material, make_settings, world
    from python_raytracer_amd.lib import vec3
    objects, _, _ = ps.build(spec, Material, world.Sprite, world.Object, vec3)
    st = make_settings(**spec["settings"])
    gen = random.Random(seed)
    made, passes, now, last = [0], {}, [0, None], [None]

    def draw():
        f = sys._getframe(1)
        v = f.f_locals
        me, flat = v["self"], v["flat"] - 1
        test = (now[0], objects.index(me), v["steps"], flat)
        d = gen.random()
        p = passes.setdefault(test[:3] + (flat // PASS,), dict(flats=set(), one=0, two=0, open_pass=0, open_fail=0, first=STATE + 2 * made[0], last=0))
        p["last"] = STATE + 2 * made[0] + 1
        made[0] += 1
        if last[0] != test:        # the first draw of the test: what kind of test is it?
            g = v["obj_mat"]
            h = v["self_spr"].get_voxel(None, v["pos"] - me.mins - v["vel_dir"], me.rot)
            p["flats"].add(flat)
            if not g.solidity > 0 or h is None:
                p["one"] += 1
            elif g.solidity >= 1:
                p["two"] += 1
            else:
                p["open_pass" if g.solidity > d else "open_fail"] += 1
        last[0] = test
        return d

    rec = {k: [] for k in ("pos", "vel", "mins", "maxs", "visible", "redraw")}
    cam, per_tick = spec["cam"], []
    for k in range(spec["ticks"]):
        now[0] = k
        ps.clear_redraw(objects)
        cam = ps.apply_script(spec, k, objects, vec3, cam)
        world.tick(objects, vec3(*cam), st, rng=draw)
        per_tick.append(made[0] - sum(per_tick))
        mp.observe(objects, rec)
    return mp.arrays(rec, objects), np.array(per_tick, np.int64), passes


def same(a, b):
    return np.array_equal(a.view(np.uint64), b.view(np.uint64)) if a.dtype == np.float64 else np.array_equal(a, b)


def main():
    data, lib, mod = load_reference()
    import physics_draw_scenes as pds
    import physics_scenes as ps
    for name, spec in pds.SCENES.items():
        spec = json.loads(json.dumps(spec))
        ref, draws, outside = run_counted(data, lib, spec)
        # (a)
        host, trace, counters = mp.run_host(spec)
        dense, _, dense_counters = mp.run_host(spec, dense=True)
        watched, host_draws, passes = run_classes(spec, spec["seed"])
        for k, v in ref.items():
            assert same(v, host[k]), "%s: the host path's %s differs from the reference's" % (name, k)
            assert same(v, dense[k]), "%s: a voxel outside a sprite's size and rim decides %s" % (name, k)
            assert k == "weight" or same(v, watched[k]), "%s: the watched run's %s differs" % (name, k)
        assert all(np.array_equal(a, b) for a, b in zip(counters, dense_counters)), "%s: ... decides a count" % name
        assert np.array_equal(draws, host_draws), (draws, host_draws)
        r = mp.reach(trace, counters)
        r["outside"] = len(outside)
        # (b) - (e)
        every = lambda p: p["one"] and p["two"] and p["open_pass"] + p["open_fail"] and sorted(p["flats"]) != list(range(min(p["flats"]) // PASS * PASS, max(p["flats"]) + 1))  # noqa: E731
        r["passes_of_all_four_classes"] = sum(bool(every(p)) for p in passes.values())
        r["passes_across_a_regeneration"] = sum(p["first"] // STATE != p["last"] // STATE for p in passes.values())
        r["open_passed"] = sum(p["open_pass"] for p in passes.values())
        r["open_failed"] = sum(p["open_fail"] for p in passes.values())
        r["draws_min"], r["draws_max"] = int(draws.min()), int(draws.max())
        # (f)
        other, _, _ = run_classes(spec, spec["seed"] + 1)
        r["fields_another_seed_changes"] = sum(not same(ref[k], other[k]) for k in ("pos", "vel", "mins", "maxs"))
        r = {k: int(v) for k, v in r.items()}
        print("%-8s %2d ticks %2d objects; draws %s; %s" % (name, spec["ticks"], len(spec["objects"]), draws.tolist(), r))
        for key in ("passes_of_all_four_classes", "passes_across_a_regeneration", "slab_over_1024_contact_beyond", "open_passed",
                    "open_failed", "fields_another_seed_changes", "blocked_steps"):
            assert r[key] >= 1, "%s does not reach what it is for: %s (%r)" % (name, key, r)
        out = dict(ref, draws=draws, spec=np.frombuffer(json.dumps(spec).encode(), np.uint8),
                   reached=np.frombuffer(json.dumps(r).encode(), np.uint8))
        path = ps.fixture_path(name)
        if mp.unchanged(path, out):
            print(os.path.relpath(path, OUT), "unchanged")
            continue
        np.savez_compressed(path, **out)
        print(os.path.relpath(path, OUT), os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
