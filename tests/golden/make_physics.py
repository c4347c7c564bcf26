#!/usr/bin/env python3
"""Generate tests/golden/physics_<scene>.npz: the reference's own physics, `for obj in objects: obj.update(cam_pos)`
(init.py:469-470, data.py:495-587), observed tick by tick on the scenes of tests/physics_scenes.py.

Needs the reference checkout make_golden.py needs; the test-suite only reads the committed output.  Nothing of the reference is
copied: its modules are imported in place (make_golden.load_reference), the scenes are built from ITS Material, Sprite and
Object, its settings store gets the scene's [PHYSICS] values, and its Object.update is called and observed.

    pos, vel           float64 [ticks, objects, 3]   after every tick
    mins, maxs         int64   [ticks, objects, 3]
    visible, redraw    bool    [ticks, objects]      (Object.visible is a Sprite or None in the reference: its truth value)
    weight             float64 [objects]             Object.weight as set_sprite left it
    spec               the scene (JSON), as tests/physics_scenes.py describes it
    reached            JSON: what the run reached (below)

Between ticks the script of the scene runs and `redraw` is cleared on every object that has a sprite, as the renderer would.

After the reference's run the same scene runs through this project's host path (world.tick) and must agree with it bit for bit
in every recorded field; the host path restates the reference statement for statement and counts as it goes, so its counts --
steps, blocked steps, contacts, transfer factors, slab sizes, the friction terms in order -- describe the reference's run.  The
files are written only if, over the scenes the device runs, the runs reached what they are for (REACH below).
The reference's lookups also find voxels OUTSIDE a sprite's size -- the import's off-by-one plane at model x = size.x, which
the box test of data.py:463-464 reaches: the default mod's cubes rest on it.  The device holds that plane besides the dense model
(vrt_body.rim) and nothing else outside the size.  So each device scene runs a second time with lookups restricted to what the
device holds; that run, too, must equal the reference's in every field, counts included.  `outside` in `reached` says how many
voxels the reference's lookups found outside the sprites' sizes.

Usage:  python tests/golden/make_physics.py
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


def observe(objects, rec):
    rec["pos"].append([[float(c) for c in (o.pos.x, o.pos.y, o.pos.z)] for o in objects])
    rec["vel"].append([[float(c) for c in (o.vel.x, o.vel.y, o.vel.z)] for o in objects])
    rec["mins"].append([[int(c) for c in (o.mins.x, o.mins.y, o.mins.z)] for o in objects])
    rec["maxs"].append([[int(c) for c in (o.maxs.x, o.maxs.y, o.maxs.z)] for o in objects])
    rec["visible"].append([bool(o.visible) for o in objects])
    rec["redraw"].append([bool(o.redraw) for o in objects])


def arrays(rec, objects):
    return dict(pos=np.array(rec["pos"], np.float64).reshape(-1, len(objects), 3), vel=np.array(rec["vel"], np.float64).reshape(-1, len(objects), 3),
                mins=np.array(rec["mins"], np.int64).reshape(-1, len(objects), 3), maxs=np.array(rec["maxs"], np.int64).reshape(-1, len(objects), 3),
                visible=np.array(rec["visible"], bool).reshape(-1, len(objects)), redraw=np.array(rec["redraw"], bool).reshape(-1, len(objects)),
                weight=np.array([float(o.weight) for o in objects], np.float64))


def run_reference(data, lib, spec, outside):
    import physics_scenes as ps
    data.objects.clear()
    for k, v in spec["settings"].items():
        setattr(data.settings, k, v)
    objects, sprites, _ = ps.build(spec, data.Material, data.Sprite, data.Object, lib.vec3)
    assert list(data.objects.values()) == objects
    weights = [float(o.weight) for o in objects]
    if spec["seed"] is not None:
        random.seed(spec["seed"])
    rec = {k: [] for k in ("pos", "vel", "mins", "maxs", "visible", "redraw")}
    cam = spec["cam"]
    get_voxel = data.Sprite.get_voxel

    def watched(self, frame, pos, rot):
        m = get_voxel(self, frame, pos, rot)
        if m is not None and not (0 <= pos.x < self.size.x and 0 <= pos.y < self.size.y and 0 <= pos.z < self.size.z):
            outside.append((pos.tuple(), self.size.tuple()))
        return m

    data.Sprite.get_voxel = watched
    try:
        for k in range(spec["ticks"]):
            ps.clear_redraw(objects)
            cam = ps.apply_script(spec, k, objects, lib.vec3, cam)
            for o in objects:
                o.update(lib.vec3(*cam))
            observe(objects, rec)
    finally:
        data.Sprite.get_voxel = get_voxel
    out = arrays(rec, objects)
    out["weight"] = np.array(weights, np.float64)
    return out


def run_host(spec, dense=False):
    """dense: lookups outside a sprite's size and its rim plane (model x = size.x) find nothing, whatever the Frame holds there
    -- what the device's models give."""
    import physics_scenes as ps
    from python_raytracer_amd import Material, make_settings
    from python_raytracer_amd import world
    from python_raytracer_amd.lib import vec3
    objects, _, _ = ps.build(spec, Material, world.Sprite, world.Object, vec3)
    st = make_settings(**spec["settings"])
    rng = random.Random(spec["seed"]).random if spec["seed"] is not None else None
    rec = {k: [] for k in ("pos", "vel", "mins", "maxs", "visible", "redraw")}
    cam, trace, counters = spec["cam"], [], []
    get_voxel = world.Sprite.get_voxel

    def inside_only(self, frame, pos, rot):
        q = self.pos_rotated(pos, rot)
        if not (0 <= q.x <= self.size.x and 0 <= q.y < self.size.y and 0 <= q.z < self.size.z):
            return None
        return get_voxel(self, frame, pos, rot)

    if dense:
        world.Sprite.get_voxel = inside_only
    try:
        for k in range(spec["ticks"]):
            ps.clear_redraw(objects)
            cam = ps.apply_script(spec, k, objects, vec3, cam)
            steps = []
            counters.append(world.tick(objects, vec3(*cam), st, rng=rng, trace=steps))
            trace.append(steps)
            observe(objects, rec)
    finally:
        world.Sprite.get_voxel = get_voxel
    return arrays(rec, objects), trace, counters


def reach(trace, counters):
    """What a run reached, from the host path's step records."""
    r = dict(blocked_steps=0, transfers_inside=0, transfers_one=0, body_ticks_3_steps=0, tie_steps=0, slab_over_1024_contact_beyond=0,
             steps_over_256_contacts=0, order_dependent_sums=0)
    for steps, cnt in zip(trace, counters):
        r["body_ticks_3_steps"] += int((cnt["steps"] >= 3).sum())
        per_body = {}
        for k, s in steps:
            r["blocked_steps"] += bool(s["blocked"])
            r["transfers_inside"] += sum(0 < f < 1 for f in s["factors"])
            r["transfers_one"] += sum(f == 1 for f in s["factors"])
            r["tie_steps"] += sum(d != 0 for d in s["dir"]) > 1
            n = (s["slab"][3] - s["slab"][0] + 1) * (s["slab"][4] - s["slab"][1] + 1) * (s["slab"][5] - s["slab"][2] + 1)
            r["slab_over_1024_contact_beyond"] += n > 1024 and any(i >= 1024 for i in s["index"])
            r["steps_over_256_contacts"] += len(s["terms"]) > 256
            per_body.setdefault(k, []).extend(s["terms"])
        for terms in per_body.values():
            fwd = rev = 0
            for t in terms:
                fwd += t
            for t in reversed(terms):
                rev += t
            r["order_dependent_sums"] += np.float64(fwd).view(np.uint64) != np.float64(rev).view(np.uint64)
    return {k: int(v) for k, v in r.items()}


REACH = dict(blocked_steps=30, transfers_inside=5, transfers_one=1, body_ticks_3_steps=1, tie_steps=1, slab_over_1024_contact_beyond=1,
             steps_over_256_contacts=1, order_dependent_sums=1)


def main():
    import physics_scenes as ps
    data, lib, mod = load_reference()
    # the default mod as the reference's own init script built it: this project's description of it must give the same weights
    mod_weights = [float(o.weight) for o in data.objects.values()]
    mod_cam = [float(c) for c in data.player.cam_pos.tuple()]
    assert mod_cam == ps.DEFAULT["cam"], mod_cam
    files, total = {}, dict.fromkeys(REACH, 0)
    for name, spec in ps.SCENES.items():
        spec = json.loads(json.dumps(spec))
        outside = []
        ref = run_reference(data, lib, spec, outside)
        got, trace, counters = run_host(spec)
        for k, v in ref.items():
            same = np.array_equal(v.view(np.uint64), got[k].view(np.uint64)) if v.dtype == np.float64 else np.array_equal(v, got[k])
            assert same, "%s: the host path's %s differs from the reference's" % (name, k)
        if name == "default":
            assert ref["weight"].tolist() == mod_weights, (ref["weight"].tolist(), mod_weights)
        r = reach(trace, counters)
        r["outside"] = len(outside)
        if name in ps.DEVICE_SCENES:
            dense, _, dense_counters = run_host(spec, dense=True)
            for k, v in ref.items():
                same = np.array_equal(v.view(np.uint64), dense[k].view(np.uint64)) if v.dtype == np.float64 else np.array_equal(v, dense[k])
                assert same, "%s: a voxel outside a sprite's size and rim decides %s" % (name, k)
            assert all(np.array_equal(a, b) for a, b in zip(counters, dense_counters)), "%s: ... decides a count" % name
            for k in total:
                total[k] += r[k]
        moved = int((np.diff(ref["pos"], axis=0) != 0).any(axis=(0, 2)).sum())
        print("%-16s %2d ticks %2d objects, %2d moved; %s" % (name, spec["ticks"], len(spec["objects"]), moved, r))
        files[name] = dict(ref, spec=np.frombuffer(json.dumps(spec).encode(), np.uint8), reached=np.frombuffer(json.dumps(r).encode(), np.uint8))
    print("reached:", total)
    short = {k: (total[k], REACH[k]) for k in REACH if total[k] < REACH[k]}
    assert not short, "the scenes do not reach what they are for: %r" % (short,)
    for name, out in files.items():
        np.savez_compressed(ps.fixture_path(name), **out)
        print(os.path.relpath(ps.fixture_path(name), OUT), os.path.getsize(ps.fixture_path(name)), "bytes")


if __name__ == "__main__":
    main()
