#!/usr/bin/env python3
"""Generate tests/golden/physics_{fluid,brim,classes,crowd_fluid}.npz: the reference's own physics on the scenes of
tests/physics_draw_scenes.py, worlds with materials of fractional solidity, with its random draws seeded and counted.

The arrays are those of the other physics fixtures (make_physics.py, whose run_reference and run_host do the runs) plus
    draws              int64 [ticks]                 random.random() calls of the tick: the reference's data.py calls the
                                                     module function, which is wrapped while its run lasts
    passes             int64 [passes, 8]             (not in `fluid`) every pass of 1024 tests that drew, in the order of the run:
                                                     tick, object, step, pass, and how many of its tests make one draw, two,
                                                     one-or-two with a second, one-or-two without
Nothing of the reference is copied: its modules are imported in place and its Object.update is called and observed.

A file is written only if
  (a) the reference, this project's host path (world.tick with random.Random(seed).random) and the host path restricted to what
      the device holds agree in every recorded field bit for bit, and in the draws of every tick;
  (f) another seed changes a recorded field;
and the run reached what its scene is for.  A pass is the device's unit: tests i * 1024 .. i * 1024 + 1023 of a step, in the
reference's loop order; the classes are those of vrt_physics_draws.hip -- no draw, one, two, one-or-two.
  fluid        (b) some pass holds tests of all four classes; (c) the draws of some pass come from two states of the generator (its
               outputs cross a multiple of 624); (d) some step has more than 1024 tests and contacts beyond the first pass; (e) tests
               that make one or two draws went both ways
  brim         (a) some pass has 1024 tests of two draws and starts at output 624 (the first output of a fresh seed: its outputs
               are 624 .. 4719, the last one word 351 of the eighth state); (b) some pass has 1024 tests of one or two draws that
               went both ways; (c) some pass has 1024 of them that all made a second; (d) some pass has 1024 contacts; (e) every
               step's tests are a multiple of 1024, each with a draw
  classes      every stripe's material was drawn for; every test on the stripes of NaN, -inf, -0.0, 0.0 and 5e-324 made one draw,
               every test on those of 1.0, nextafter(1, 2) and +inf under a voxel of the raft made two; some pass holds at least
               six of the ten
  crowd_fluid  some step draws for a candidate below index 1024 and for one at or above it, with a test of one or two draws in
               each
`reached` in the file (JSON) says how often each was met, besides the counts make_physics.py keeps.

The classes are observed from inside the host path's loop, which restates the reference's statement for statement: the draw
function handed to world.tick looks at the loop's variables (the test's number in the step, both materials, the neighbour).

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
KINDS = ("one", "two", "open_pass", "open_fail")


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


def run_classes(spec, seed, tests=None):
    """The host path with a draw function that watches the loop it is called from.  Returns (arrays, draws per tick, passes):
    passes maps (tick, object, step, pass) to dict(flats: the tests of the pass that drew, one/two/open_pass/open_fail: how many of
    each class, first/last: the generator's output positions the pass used, counted from the seeding).  tests: a dict that
    receives, for every test that drew, (tick, object, step, test) -> [the neighbour's material index, whether the mover has a
    voxel there, the neighbour's index, the class, the draws made]."""
    import physics_scenes as ps
    from python_raytracer_amd import Material, make_settings, world
    from python_raytracer_amd.lib import vec3
    objects, _, mats = ps.build(spec, Material, world.Sprite, world.Object, vec3)
    number, material = {id(o): i for i, o in enumerate(objects)}, {id(m): i for i, m in enumerate(mats)}
    st = make_settings(**spec["settings"])
    gen = random.Random(seed)
    made, passes, now, last = [0], {}, [0, None], [None]

    def draw():
        f = sys._getframe(1)
        v = f.f_locals
        me, flat = v["self"], v["flat"] - 1
        test = (now[0], number[id(me)], v["steps"], flat)
        d = gen.random()
        p = passes.setdefault(test[:3] + (flat // PASS,), dict(flats=set(), one=0, two=0, open_pass=0, open_fail=0, first=STATE + 2 * made[0], last=0))
        p["last"] = STATE + 2 * made[0] + 1
        made[0] += 1
        if last[0] != test:        # the first draw of the test: what kind of test is it?
            g = v["obj_mat"]
            h = v["self_spr"].get_voxel(None, v["pos"] - me.mins - v["vel_dir"], me.rot)
            p["flats"].add(flat)
            if not g.solidity > 0 or h is None:
                kind = "one"
            elif g.solidity >= 1:
                kind = "two"
            else:
                kind = "open_pass" if g.solidity > d else "open_fail"
            p[kind] += 1
            if tests is not None:
                tests[test] = [material[id(g)], h is not None, number[id(v["obj"])], kind, 0]
        if tests is not None:
            tests[test][4] += 1
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


def steps_of(trace):
    """{(tick, object, step): step dict} of make_physics.run_host's trace."""
    out = {}
    for t, steps in enumerate(trace):
        seen = {}
        for k, s in steps:
            out[(t, k, seen.setdefault(k, 0))] = s
            seen[k] += 1
    return out


# ---- what each scene is for: (reached, the keys that must be at least 1) -----------------------------------------------------------
def reach_fluid(r, spec, passes, tests, trace):
    every = lambda p: p["one"] and p["two"] and p["open_pass"] + p["open_fail"] and sorted(p["flats"]) != list(range(min(p["flats"]) // PASS * PASS, max(p["flats"]) + 1))  # noqa: E731
    r["passes_of_all_four_classes"] = sum(bool(every(p)) for p in passes.values())
    r["passes_across_a_regeneration"] = sum(p["first"] // STATE != p["last"] // STATE for p in passes.values())
    r["open_passed"] = sum(p["open_pass"] for p in passes.values())
    r["open_failed"] = sum(p["open_fail"] for p in passes.values())
    return ("passes_of_all_four_classes", "passes_across_a_regeneration", "slab_over_1024_contact_beyond", "open_passed", "open_failed",
            "blocked_steps")


def reach_brim(r, spec, passes, tests, trace):
    r["passes_of_1024_two_from_624"] = sum(p["two"] == PASS and p["first"] == STATE and p["last"] == STATE + 4 * PASS - 1 for p in passes.values())
    r["passes_of_1024_open_both_ways"] = sum(p["open_pass"] + p["open_fail"] == PASS and p["open_pass"] > 0 and p["open_fail"] > 0 for p in passes.values())
    r["passes_of_1024_open_all_passed"] = sum(p["open_pass"] == PASS for p in passes.values())
    r["passes_of_2048_draws"] = sum(p["last"] - p["first"] + 1 == 4 * PASS for p in passes.values())
    steps = steps_of(trace)
    contacts = {}
    for key, s in steps.items():
        for i in s["index"]:
            contacts[key + (i // PASS,)] = contacts.get(key + (i // PASS,), 0) + 1
    r["passes_of_1024_contacts"] = sum(n == PASS for n in contacts.values())
    drew = {}
    for key, p in passes.items():
        drew[key[:3]] = drew.get(key[:3], 0) + len(p["flats"])
    whole = 0
    for key, s in steps.items():
        n = (s["slab"][3] - s["slab"][0] + 1) * (s["slab"][4] - s["slab"][1] + 1) * (s["slab"][5] - s["slab"][2] + 1)
        whole += n % PASS == 0 and drew.get(key, 0) == n      # (one neighbour, and every test of the slab drew)
    r["steps"], r["steps_of_whole_passes"] = len(steps), whole
    assert whole == len(steps) == len(drew), "brim: a step whose tests are not a multiple of 1024 (%d of %d)" % (whole, len(steps))
    return ("passes_of_1024_two_from_624", "passes_of_1024_open_both_ways", "passes_of_1024_open_all_passed", "passes_of_2048_draws",
            "passes_of_1024_contacts", "steps_of_whole_passes", "order_dependent_sums", "blocked_steps")


def reach_classes(r, spec, passes, tests, trace):
    import physics_draw_scenes as pds
    stripes = range(len(pds.STRIPES))
    name = lambda i: "stripe_%d" % i  # noqa: E731
    for i in stripes:
        r[name(i) + "_tests"] = sum(t[0] == i for t in tests.values())
        r[name(i) + "_draws"] = sum(t[4] for t in tests.values() if t[0] == i)
    solid = lambda i: spec["materials"][i]["solidity"]  # noqa: E731
    once = [i for i in stripes if not solid(i) > 0 or solid(i) == 5e-324]
    twice = [i for i in stripes if solid(i) >= 1]
    assert len(once) == 5 and len(twice) == 3, (once, twice)
    for i in once:
        assert all(t[4] == 1 for t in tests.values() if t[0] == i), "classes: a test on stripe %d (%r) drew twice" % (i, solid(i))
    for i in twice:
        under = [t for t in tests.values() if t[0] == i and t[1]]
        assert under and all(t[4] == 2 for t in under), "classes: a test on stripe %d (%r) under the raft did not draw twice" % (i, solid(i))
    r["tests_of_one_draw_checked"] = sum(t[0] in once for t in tests.values())
    r["tests_of_two_draws_checked"] = sum(t[0] in twice and t[1] for t in tests.values())
    in_pass = {}
    for (t, k, s, flat), v in tests.items():
        if v[0] in stripes:
            in_pass.setdefault((t, k, s, flat // PASS), set()).add(v[0])
    r["stripes_in_one_pass_max"] = max(len(v) for v in in_pass.values())
    r["passes_of_six_stripes"] = sum(len(v) >= 6 for v in in_pass.values())
    r["open_passed"] = sum(p["open_pass"] for p in passes.values())
    r["open_failed"] = sum(p["open_fail"] for p in passes.values())
    return tuple(name(i) + "_draws" for i in stripes) + ("tests_of_one_draw_checked", "tests_of_two_draws_checked", "passes_of_six_stripes",
                                                         "open_passed", "open_failed", "blocked_steps")


def reach_crowd_fluid(r, spec, passes, tests, trace):
    by_step = {}
    for key, v in tests.items():
        by_step.setdefault(key[:3], []).append(v)
    both = both_open = 0
    for vs in by_step.values():
        low, high = [v for v in vs if v[2] < mp.TILE], [v for v in vs if v[2] >= mp.TILE]
        both += bool(low and high)
        both_open += any(v[3].startswith("open") for v in low) and any(v[3].startswith("open") for v in high)
    r["steps_drawing_on_both_sides_of_1024"], r["steps_open_on_both_sides_of_1024"] = both, both_open
    r["open_passed"] = sum(p["open_pass"] for p in passes.values())
    r["open_failed"] = sum(p["open_fail"] for p in passes.values())
    return ("steps_drawing_on_both_sides_of_1024", "steps_open_on_both_sides_of_1024", "open_passed", "open_failed", "blocked_steps")


REACH = dict(fluid=reach_fluid, brim=reach_brim, classes=reach_classes, crowd_fluid=reach_crowd_fluid)


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
        tests = {}
        watched, host_draws, passes = run_classes(spec, spec["seed"], tests)
        for k, v in ref.items():
            assert same(v, host[k]), "%s: the host path's %s differs from the reference's" % (name, k)
            assert same(v, dense[k]), "%s: a voxel outside a sprite's size and rim decides %s" % (name, k)
            assert k == "weight" or same(v, watched[k]), "%s: the watched run's %s differs" % (name, k)
        assert all(np.array_equal(a, b) for a, b in zip(counters, dense_counters)), "%s: ... decides a count" % name
        assert np.array_equal(draws, host_draws), (draws, host_draws)
        assert sum(t[4] for t in tests.values()) == draws.sum()
        r = mp.reach(trace, counters)
        r["outside"] = len(outside)
        # what the scene is for
        needed = REACH[name](r, spec, passes, tests, trace)
        r["draws_min"], r["draws_max"] = int(draws.min()), int(draws.max())
        # (f)
        other, _, _ = run_classes(spec, spec["seed"] + 1)
        r["fields_another_seed_changes"] = sum(not same(ref[k], other[k]) for k in ("pos", "vel", "mins", "maxs"))
        r = {k: int(v) for k, v in r.items()}
        print("%-11s %2d ticks %2d objects; draws %s; %s" % (name, spec["ticks"], len(spec["objects"]), draws.tolist(), r))
        for key in needed + ("fields_another_seed_changes",):
            assert r[key] >= 1, "%s does not reach what it is for: %s (%r)" % (name, key, r)
        out = dict(ref, draws=draws, spec=np.frombuffer(json.dumps(spec).encode(), np.uint8),
                   reached=np.frombuffer(json.dumps(r).encode(), np.uint8))
        if name != "fluid":
            out["passes"] = np.array([list(key) + [p[c] for c in KINDS] for key, p in passes.items()], np.int64).reshape(-1, 8)
        path = ps.fixture_path(name)
        if mp.unchanged(path, out):
            print(os.path.relpath(path, OUT), "unchanged")
            continue
        np.savez_compressed(path, **out)
        print(os.path.relpath(path, OUT), os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
