#!/usr/bin/env python3
"""Generate tests/golden/physics_run_draws.npz: the reference's own Object.update -- flags, animation, physics with its random
draws -- observed tick by tick on the scenes of tests/physics_run_draw_scenes.py, with the camera on the body that carries it,
a scripted clock and a seeded generator.

Needs the reference checkout make_golden.py needs; the test-suite only reads the committed output.  Nothing of the reference is
copied: its modules are imported in place (make_golden.load_reference), the pygame stand-in's time.get_ticks -- the clock
Sprite.anim_update reads -- is set to the scene's clock, random.seed(seed) is called per scene, the scenes are built from ITS
Material, Sprite and Object, and every tick is `for obj in objects: obj.update(cam)` with cam = data.player.cam_pos before the
tick, as init.py:464 has it (a scene without `follow`: the scene's camera).

Per scene <s>, every key prefixed "<s>/": the fields make_physics_anim.py records --
    pos, vel           float64 [ticks, objects, 3]   after every tick
    mins, maxs         int64   [ticks, objects, 3]
    visible, redraw    bool    [ticks, objects]
    weight             float64 [ticks, objects]      Object.weight after every tick
    frame              int64   [ticks, sprites]      Sprite.frame after every tick, sprites in the scene's order
    weight0            float64 [objects]             Object.weight as set_sprite left it
-- and
    draws              int64   [ticks]               random.random() calls of the tick (the module function, wrapped for the run)
    state              uint32  [625]                 random.getstate()[1] after the last tick
    held_pos, held_vel float64 [ticks, objects, 3]   the same scene HELD: `wade` with the camera left where it stood at the start,
    held_draws         int64   [ticks]               `tide` with the clock held at 0 -- again the reference's own run
and once: spec {scene: its description} (JSON), reached (JSON: how often each REACH condition was met).

Between ticks `redraw` is cleared on every object that has a sprite, as the renderer would.

After the reference's runs the same scenes run through this project's host path, world.run(follow=, clock=, rng=), tick by tick
and as one run: it must agree bit for bit in every field, in every tick's draws and in the generator's final state.  The file is
written only if every REACH condition holds, checked from the host path (which restates the reference statement for statement,
so a draw function can look at the loop it is called from):
  held_camera_changes_end_and_draws   `wade` under the held camera ends elsewhere and has another `draws` sequence: flags that
                                      only the followed camera gives decide how many draws a tick makes
  asleep_would_have_drawn             a body is asleep at a tick at which, awake (dist_move lifted for that tick), it draws
  held_clock_changes_draws_from_switch `tide` under the held clock has the same draws before the first switch and others from it on
  earlier_twin_drew_against_old_frame in a tick with a switch, a body before the switching one drew, and with the switch made
                                      before the tick's first object the tick's draws come out differently
  tick_crosses_a_state                some tick's outputs cross a multiple of 624, and each scene uses more than 3 * 624 outputs
  open_both_ways_in_one_pass          in `wade`, a pass of 1024 tests holds undecided tests that made a second draw and that did not
  another_seed_changes_run            seed + 1 changes a recorded field of each scene

Usage:  python tests/golden/make_physics_run_draws.py
"""
import json
import os
import random
import sys

import numpy as np

from make_golden import load_reference

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(OUT))
sys.path.insert(0, os.path.dirname(os.path.dirname(OUT)))

from make_physics import arrays, observe, unchanged  # noqa: E402

PASS, STATE = 1024, 624
REACH = ("held_camera_changes_end_and_draws", "asleep_would_have_drawn", "held_clock_changes_draws_from_switch",
         "earlier_twin_drew_against_old_frame", "tick_crosses_a_state", "open_both_ways_in_one_pass", "another_seed_changes_run")


def run_reference(data, lib, spec, held=False):
    """held: the scene's camera stays where it stood at the start and the clock at 0."""
    import physics_anim_scenes as an
    import physics_scenes as ps
    import pygame as pg
    now, made = [0], [0]
    pg.time.get_ticks = lambda: now[0]
    data.objects.clear()
    for k, v in spec["settings"].items():
        setattr(data.settings, k, v)
    objects, sprites, _, who = an.build(spec, data.Material, data.Sprite, data.Object, lib.vec3, lib.vec2)
    data.player = who
    weight0 = [float(o.weight) for o in objects]
    rec = {k: [] for k in ("pos", "vel", "mins", "maxs", "visible", "redraw")}
    weights, frames, draws = [], [], []
    real = random.random

    def counted():
        made[0] += 1
        return real()

    random.seed(spec["seed"])
    random.random = counted
    try:
        for k in range(spec["ticks"]):
            ps.clear_redraw(objects)
            now[0] = 0 if held else spec["clock"][0] + k * spec["clock"][1]
            cam = data.player.cam_pos if who is not None and not held else lib.vec3(*spec["cam"])
            for o in objects:
                o.update(cam)
            draws.append(made[0] - sum(draws))
            observe(objects, rec)
            weights.append([float(o.weight) for o in objects])
            frames.append([int(sprites[name].frame) for name in an.sprite_names(spec)])
    finally:
        random.random = real
        now[0] = 0
    out = arrays(rec, objects)
    out.update(weight=np.array(weights, np.float64), frame=np.array(frames, np.int64), weight0=np.array(weight0, np.float64),
               draws=np.array(draws, np.int64), state=np.array(random.getstate()[1], np.uint32))
    return out


def run_host(spec, seed, held=False, early=False, lift=None):
    """The project's host path, tick by tick, with a draw function that watches the loop it is called from.  Returns (the
    reference's arrays, anim samples per tick, draws [ticks][objects], passes: {(tick, object, step, pass): [undecided tests that
    made a second draw, that did not]}).  early: the deliberately WRONG variant that makes every switch of a tick before the
    tick's first object moves.  lift: a tick at which dist_move is lifted so that nothing sleeps."""
    import physics_anim_scenes as an
    import physics_scenes as ps
    from python_raytracer_amd import make_settings, world
    objects, sprites, _, st, who = an.project_scene(spec)
    number = {id(o): i for i, o in enumerate(objects)}
    gen = random.Random(seed)
    weight0 = [float(o.weight) for o in objects]
    rec = {k: [] for k in ("pos", "vel", "mins", "maxs", "visible", "redraw")}
    weights, frames, anim = [], [], []
    per_object = np.zeros((spec["ticks"], len(objects)), np.int64)
    passes, now, last = {}, [0], [None]

    def draw():
        v = sys._getframe(1).f_locals
        me, flat = v["self"], v["flat"] - 1
        test = (now[0], number[id(me)], v["steps"], flat)
        d = gen.random()
        per_object[now[0], number[id(me)]] += 1
        if last[0] != test:      # the first draw of the test
            g = v["obj_mat"]
            h = v["self_spr"].get_voxel(None, v["pos"] - me.mins - v["vel_dir"], me.rot)
            if g.solidity > 0 and h is not None and not g.solidity >= 1:
                passes.setdefault(test[:3] + (flat // PASS,), [0, 0])[0 if g.solidity > d else 1] += 1
        last[0] = test
        return d

    start, step = spec["clock"]
    for k in range(spec["ticks"]):
        now[0] = k
        ps.clear_redraw(objects)
        cam = who.cam_pos if who is not None and not held else world.vec3(*spec["cam"])
        clock = 0 if held else start + k * step
        s = make_settings(**dict(spec["settings"], dist_move=1e9)) if lift == k else st
        if early:
            for o in objects:
                dist = o.pos.distance(cam)
                if o.sprite and dist <= s.dist_max + max(o.size.x, o.size.y, o.size.z) and dist <= s.dist_move:
                    old = o.sprite.frame
                    o.sprite.anim_update(clock)
                    if old != o.sprite.frame:
                        o.redraw = True
                        o.set_weight()
            world.tick(objects, cam, s, rng=draw)
            anim.append(None)
        else:
            _, _, a = world.run(objects, cam, s, 1, trace=True, clock=(clock, 0), rng=draw)
            anim.append(a[0])
        observe(objects, rec)
        weights.append([float(o.weight) for o in objects])
        frames.append([int(sprites[name].frame) for name in an.sprite_names(spec)])
    out = arrays(rec, objects)
    out.update(weight=np.array(weights, np.float64), frame=np.array(frames, np.int64), weight0=np.array(weight0, np.float64),
               draws=per_object.sum(axis=1), state=np.array(gen.getstate()[1], np.uint32))
    return out, anim, per_object, passes


def run_whole(spec):
    """world.run(follow=, clock=, rng=) as ONE run: (trace, anim, the generator afterwards)."""
    import physics_anim_scenes as an
    import physics_scenes as ps
    from python_raytracer_amd import world
    objects, sprites, _, st, who = an.project_scene(spec)
    ps.clear_redraw(objects)
    gen = random.Random(spec["seed"])
    _, trace, anim = world.run(objects, world.vec3(*spec["cam"]), st, spec["ticks"], follow=who, trace=True, rng=gen.random,
                               clock=tuple(spec["clock"]))
    return trace, anim, gen


def same(a, b):
    return np.array_equal(a.view(np.uint64), b.view(np.uint64)) if a.dtype == np.float64 else np.array_equal(a, b)


def reach(name, spec, ref, held, host):
    got, anim, per_object, passes = host
    r = dict.fromkeys(REACH, 0)
    ticks = spec["ticks"]
    differs = not same(ref["pos"][-1], held["pos"][-1]) and not np.array_equal(ref["draws"], held["draws"])
    switched = np.array([a["switched"] != 0 for a in anim])                       # [ticks, objects]
    if name == "wade":
        r["held_camera_changes_end_and_draws"] = int(differs)
        r["open_both_ways_in_one_pass"] = sum(1 for a, b in passes.values() if a and b)
    # a body asleep at tick k (its `awake` sample) that draws at tick k once dist_move is lifted for that tick
    whole_trace, _, _ = run_whole(spec)
    for k in range(ticks):
        asleep = [i for i, o in enumerate(spec["objects"]) if o["physics"] and not whole_trace[k]["awake"][i]]
        if not asleep:
            continue
        lifted = run_host(spec, spec["seed"], lift=k)[2]
        r["asleep_would_have_drawn"] += sum(int(per_object[k][i] == 0 and lifted[k][i] > 0) for i in asleep)
    if name == "tide":
        first = int(np.nonzero(switched.any(axis=1))[0][0])
        before = np.array_equal(ref["draws"][:first], held["draws"][:first])
        r["held_clock_changes_draws_from_switch"] = int(before and first > 0 and ref["draws"][first] != held["draws"][first])
        early = run_host(spec, spec["seed"], early=True)
        for k in np.nonzero(switched.any(axis=1))[0]:
            who = int(np.nonzero(switched[k])[0][0])
            drew_before = per_object[k][:who].sum() > 0
            # (the runs are identical up to tick k only for the first such tick: compare there, and count the others by their draws)
            if drew_before and (k != first or early[0]["draws"][k] != ref["draws"][k]):
                r["earlier_twin_drew_against_old_frame"] += 1
        assert early[0]["draws"][first] != ref["draws"][first], "tide: the switch made early leaves the switching tick's draws as they are"
    outputs = 2 * np.concatenate([[0], np.cumsum(ref["draws"])]) + STATE      # the generator's position, counted from the seeding
    crosses = sum(int(outputs[k] // STATE != (outputs[k + 1] - 1) // STATE) for k in range(ticks) if ref["draws"][k])
    r["tick_crosses_a_state"] = crosses if 2 * ref["draws"].sum() > 3 * STATE else 0
    other = run_host(spec, spec["seed"] + 1)[0]
    r["another_seed_changes_run"] = int(any(not same(ref[k], other[k]) for k in ("pos", "vel", "mins", "maxs")))
    return r


def main():
    import physics_run_draw_scenes as rd
    data, lib, mod = load_reference()
    out, total, specs = {}, dict.fromkeys(REACH, 0), {}
    per_scene = {}
    for name, spec in rd.SCENES.items():
        spec = json.loads(json.dumps(spec))
        specs[name] = spec
        assert len(spec["objects"]) <= 8
        ref = run_reference(data, lib, spec)
        held = run_reference(data, lib, spec, held=True)
        host = run_host(spec, spec["seed"])
        for k, v in ref.items():
            assert same(v, host[0][k]), "%s: the host path's %s differs from the reference's" % (name, k)
        host_held = run_host(spec, spec["seed"], held=True)[0]
        for k, v in held.items():
            assert same(v, host_held[k]), "%s: the host path's held %s differs from the reference's" % (name, k)
        trace, anim, gen = run_whole(spec)
        assert same(np.ascontiguousarray(trace["pos"]), ref["pos"]) and same(np.ascontiguousarray(trace["vel"]), ref["vel"]), name
        assert np.array_equal(np.array(gen.getstate()[1], np.uint32), ref["state"]), "%s: world.run leaves another generator" % name
        r = reach(name, spec, ref, held, host)
        per_scene[name] = r
        print("%-5s %2d ticks %d objects; draws %s; held %s; %s" % (name, spec["ticks"], len(spec["objects"]), ref["draws"].tolist(),
                                                                  held["draws"].tolist(), {k: v for k, v in r.items() if v}))
        for k in total:
            total[k] += r[k]
        for k, v in ref.items():
            out["%s/%s" % (name, k)] = v
        out["%s/held_pos" % name], out["%s/held_vel" % name], out["%s/held_draws" % name] = held["pos"], held["vel"], held["draws"]
    print("reached:", total)
    short = [k for k in REACH if total[k] < 1]
    short += ["%s: %s" % (n, k) for n, r in per_scene.items() for k in ("tick_crosses_a_state", "another_seed_changes_run") if r[k] < 1]
    assert not short, "the scenes do not exercise: %r" % (short,)
    out["spec"] = np.frombuffer(json.dumps(specs).encode(), np.uint8)
    out["reached"] = np.frombuffer(json.dumps({k: int(v) for k, v in total.items()}).encode(), np.uint8)
    if unchanged(rd.PATH, out):
        print(os.path.relpath(rd.PATH, OUT), "unchanged")
        return
    np.savez_compressed(rd.PATH, **out)
    print(os.path.relpath(rd.PATH, OUT), os.path.getsize(rd.PATH), "bytes")


if __name__ == "__main__":
    main()
