#!/usr/bin/env python3
"""Generate tests/golden/physics_anim.npz: the reference's own physics with its sprites animated, observed tick by tick on the
scenes of tests/physics_anim_scenes.py under a scripted clock.

Needs the reference checkout make_golden.py needs; the test-suite only reads the committed output.  Nothing of the reference is
copied: its modules are imported in place (make_golden.load_reference), the pygame stand-in's time.get_ticks -- the clock
Sprite.anim_update reads (data.py:306) -- is set to the scene's clock, the scenes are built from ITS Material, Sprite and Object,
ITS Sprite.anim_set is called, and every tick is `for obj in objects: obj.update(cam)` with the clock at start_ms + k * step_ms
(with `follow`, cam is data.player.cam_pos before the tick, as init.py:464 has it).

Per scene <s>, every key prefixed "<s>/":
    pos, vel           float64 [ticks, objects, 3]   after every tick
    mins, maxs         int64   [ticks, objects, 3]
    visible, redraw    bool    [ticks, objects]
    weight             float64 [ticks, objects]      Object.weight after every tick
    frame              int64   [ticks, sprites]      Sprite.frame after every tick, sprites in the scene's order
    weight0            float64 [objects]             Object.weight as set_sprite left it
    held_pos, held_vel float64 [ticks, objects, 3]   the same scene with the clock held at 0: no sprite ever changes its frame
                                                     (a scene of more than 8 objects: the last tick only, [1, objects, 3])
and once:
    spec               {scene: its description} (JSON)
    table_anim         float64 [rows, 3]             frame_start, frame_end, frame_time as given to anim_set (TABLE_FRAMES frames)
    table_now          int64   [rows]                the clock's reading
    table_frame        int64   [rows]                Sprite.frame after the reference's anim_update

Between ticks `redraw` is cleared on every object that has a sprite, as the renderer would.

After the reference's runs the same scenes run through this project's host path (world.run(clock=)), which must agree bit for bit
in every recorded field.  The file is written only if the scenes exercise what can go wrong (REACH below); the host path, which
restates the reference and says which object made which switch, checks each condition.

Usage:  python tests/golden/make_physics_anim.py
"""
import json
import os
import sys

import numpy as np

from make_golden import load_reference

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(OUT))
sys.path.insert(0, os.path.dirname(os.path.dirname(OUT)))

from make_physics import arrays, observe, unchanged  # noqa: E402

REACH = ("switches_and_final_differs", "stale_weight_decides_velocity", "frame_behind_schedule", "switch_inside_tick_matters",
         "plays_backwards", "non_physical_switch_redraws", "crowd_both_sides_of_tile")


def run_reference(data, lib, spec, clock):
    """clock: the scene's (start_ms, step_ms), or None: held at 0."""
    import physics_anim_scenes as an
    import physics_scenes as ps
    import pygame as pg
    now = [0]
    pg.time.get_ticks = lambda: now[0]
    data.objects.clear()
    for k, v in spec["settings"].items():
        setattr(data.settings, k, v)
    objects, sprites, _, who = an.build(spec, data.Material, data.Sprite, data.Object, lib.vec3, lib.vec2)
    data.player = who
    weight0 = [float(o.weight) for o in objects]
    rec = {k: [] for k in ("pos", "vel", "mins", "maxs", "visible", "redraw")}
    weights, frames = [], []
    for k in range(spec["ticks"]):
        ps.clear_redraw(objects)
        now[0] = clock[0] + k * clock[1] if clock else 0
        cam = data.player.cam_pos if who is not None else lib.vec3(*spec["cam"])
        for o in objects:
            o.update(cam)
        observe(objects, rec)
        weights.append([float(o.weight) for o in objects])
        frames.append([int(sprites[name].frame) for name in an.sprite_names(spec)])
    out = arrays(rec, objects)
    out.update(weight=np.array(weights, np.float64), frame=np.array(frames, np.int64), weight0=np.array(weight0, np.float64))
    now[0] = 0
    return out


def run_host(spec, early=False):
    """The project's host path, tick by tick: (the reference's arrays, the anim samples per tick).  early: the deliberately WRONG
    variant that makes every switch of a tick before the tick's first object moves."""
    import physics_anim_scenes as an
    import physics_scenes as ps
    from python_raytracer_amd import world
    objects, sprites, _, st, who = an.project_scene(spec)
    weight0 = [float(o.weight) for o in objects]
    rec = {k: [] for k in ("pos", "vel", "mins", "maxs", "visible", "redraw")}
    weights, frames, anim = [], [], []
    start, step = spec["clock"]
    for k in range(spec["ticks"]):
        ps.clear_redraw(objects)
        cam = who.cam_pos if who is not None else world.vec3(*spec["cam"])
        if early:
            for o in objects:
                dist = o.pos.distance(cam)
                if o.sprite and dist <= st.dist_max + max(o.size.x, o.size.y, o.size.z) and dist <= st.dist_move:
                    old = o.sprite.frame
                    o.sprite.anim_update(start + k * step)
                    if old != o.sprite.frame:
                        o.redraw = True
                        o.set_weight()
            world.tick(objects, cam, st)
            anim.append(None)
        else:
            _, _, a = world.run(objects, cam, st, 1, trace=True, clock=(start + k * step, 0))
            anim.append(a[0])
        observe(objects, rec)
        weights.append([float(o.weight) for o in objects])
        frames.append([int(sprites[name].frame) for name in an.sprite_names(spec)])
    out = arrays(rec, objects)
    out.update(weight=np.array(weights, np.float64), frame=np.array(frames, np.int64), weight0=np.array(weight0, np.float64))
    return out, anim


def same(a, b):
    return np.array_equal(a.view(np.uint64), b.view(np.uint64)) if a.dtype == np.float64 else np.array_equal(a, b)


def reach(name, spec, ref, held, anim):
    """What the scene's run shows, from the reference's records and the host path's samples (which object switched when)."""
    import physics_anim_scenes as an
    from python_raytracer_amd import world
    r = dict.fromkeys(REACH, 0)
    names = an.sprite_names(spec)
    start, step = spec["clock"]
    switched = np.array([a["switched"] != 0 for a in anim])                      # [ticks, objects]
    r["switches_and_final_differs"] = int(switched.any() and not same(ref["pos"][-1], held["pos"][-1]))
    sprite_of = [o["sprite"] for o in spec["objects"]]
    for i in range(len(sprite_of)):
        for j in range(i + 1, len(sprite_of)):
            if sprite_of[i] is None or sprite_of[i] != sprite_of[j] or "anim" not in spec["sprites"][sprite_of[i]]:
                continue
            apart = np.nonzero(ref["weight"][:, i] != ref["weight"][:, j])[0]
            twins = spec["objects"][i]["vel"] == spec["objects"][j]["vel"] and spec["objects"][i]["pos"][1] == spec["objects"][j]["pos"][1]
            if len(apart) and twins and (ref["vel"][apart[0] + 1:, i, 1] != ref["vel"][apart[0] + 1:, j, 1]).any():
                r["stale_weight_decides_velocity"] += 1
    # the schedule, by the project's frame_at on the project's sprites
    _, sprites, _, _, _ = an.project_scene(spec)
    early, _ = run_host(spec, early=True)
    r["switch_inside_tick_matters"] = int(not same(early["pos"][-1], ref["pos"][-1]) or not same(early["vel"][-1], ref["vel"][-1]))
    for c, sname in enumerate(names):
        spr = sprites[sname]
        if not isinstance(spr, world.Sprite) or not spr.animated:
            continue
        due = np.array([spr.frame_at(start + k * step) for k in range(spec["ticks"])])
        r["frame_behind_schedule"] += int((ref["frame"][:, c] != due).any())
        if spr.frame_time < 0 and (np.diff(np.concatenate([[0], ref["frame"][:, c]])) != 0).any():
            r["plays_backwards"] += 1
    for k, o in enumerate(spec["objects"]):
        if not o["physics"] and switched[:, k].any():
            t = np.nonzero(switched[:, k])[0]
            r["non_physical_switch_redraws"] += int(ref["redraw"][t, k].all() and (ref["pos"][:, k] == ref["pos"][0, k]).all())
    if name == "crowd":
        R = an.CROWD_ROLES
        assert R["blink_low"] < R["mover_low"] < an.TILE < R["switcher"] < R["mover_high"] < R["blink_high"]
        who = set(np.nonzero(switched.any(axis=0))[0].tolist())
        movers_differ = all(not same(ref["pos"][-1][R[m]], held["pos"][-1][R[m]]) for m in ("mover_low", "mover_high"))
        r["crowd_both_sides_of_tile"] = int(who == {R["switcher"]} and movers_differ)
    return r


def table(data):
    import physics_anim_scenes as an
    import pygame as pg
    now = [0]
    pg.time.get_ticks = lambda: now[0]
    rows = []
    spr = data.Sprite(frames=an.TABLE_FRAMES)
    for first, last, ft in an.TABLE_ANIMS:
        spr.anim_set(first, last, ft)
        for t in an.TABLE_NOWS:
            now[0] = t
            spr.anim_update()
            rows.append((first, last, ft, t, spr.frame))
    now[0] = 0
    rows = np.array(rows, np.float64)
    return dict(table_anim=rows[:, :3].copy(), table_now=rows[:, 3].astype(np.int64), table_frame=rows[:, 4].astype(np.int64))


def main():
    import physics_anim_scenes as an
    data, lib, mod = load_reference()
    out, total = {}, dict.fromkeys(REACH, 0)
    specs = {}
    for name, spec in an.SCENES.items():
        spec = json.loads(json.dumps(spec))
        specs[name] = spec
        ref = run_reference(data, lib, spec, spec["clock"])
        held = run_reference(data, lib, spec, None)
        assert (held["frame"] == 0).all(), "%s: a sprite changes its frame under the clock held at 0" % name
        got, anim = run_host(spec)
        for k, v in ref.items():
            assert same(v, got[k]), "%s: the host path's %s differs from the reference's" % (name, k)
        r = reach(name, spec, ref, held, anim)
        print("%-10s %2d ticks %4d objects; %s" % (name, spec["ticks"], len(spec["objects"]), {k: v for k, v in r.items() if v}))
        for k in total:
            total[k] += r[k]
        for k, v in ref.items():
            out["%s/%s" % (name, k)] = v
        keep = slice(-1, None) if len(spec["objects"]) > 8 else slice(None)
        out["%s/held_pos" % name], out["%s/held_vel" % name] = held["pos"][keep], held["vel"][keep]
    print("reached:", total)
    short = [k for k in REACH if total[k] < 1]
    assert not short, "the scenes do not exercise: %r" % (short,)
    out.update(table(data))
    out["spec"] = np.frombuffer(json.dumps(specs).encode(), np.uint8)
    if unchanged(an.PATH, out):
        print(os.path.relpath(an.PATH, OUT), "unchanged")
        return
    np.savez_compressed(an.PATH, **out)
    print(os.path.relpath(an.PATH, OUT), os.path.getsize(an.PATH), "bytes")


if __name__ == "__main__":
    main()
