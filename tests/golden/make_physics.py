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
The scene `crowd` has more bodies than the device walks at a time; its file is written only if the run also shows what that scene
is for (crowd_reach).  A file whose arrays come out as they are on disk is not written again.

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


TILE = 1024     # the bodies the device walks at a time (vrt_physics.hip, VRT_PHYS_BLOCK)
CROWD_REACH = ("contacts_both_sides_one_step", "transfers_both_sides_one_step", "movers_from_1024", "visible_before_met", "visible_now_met")


def crowd_reach(ref, trace):
    """What the scene `crowd` is for, from the reference's record, the host path's step records and the scene's roles: every
    count must be at least 1."""
    import physics_scenes as ps
    R, T = ps.CROWD_ROLES, ps.CROWD_SCRIPT_TICK
    spec = ps.CROWD
    friction = lambda role: spec["materials"][spec["sprites"][spec["objects"][R[role]]["sprite"]]["boxes"][0][2]]["friction"]  # noqa: E731
    f_bar, f_low, f_high = friction("bar"), friction("block_low"), friction("block_high")
    assert R["block_low"] < R["bar"] < TILE < R["block_high"] and f_low * f_bar != f_high * f_bar
    assert R["taker_low"] < TILE <= R["giver"] < R["taker_high"] and R["mover_low"] < TILE < R["late_high"]
    assert R["late_low"] < TILE <= R["mover_1024"]
    r = dict.fromkeys(CROWD_REACH, 0)
    for t, steps in enumerate(trace):
        for k, s in steps:
            if k == R["bar"] and s["blocked"]:
                # the lower block's terms first, then the higher block's: each block's friction is its own
                low, high = s["terms"].count(f_low * f_bar * 1.0), s["terms"].count(f_high * f_bar * 1.0)
                fwd = rev = 0
                for term in s["terms"]:
                    fwd += term
                for term in reversed(s["terms"]):
                    rev += term
                if low and high and low + high == len(s["terms"]) and s["terms"][:low] == [f_low * f_bar * 1.0] * low and fwd != rev:
                    r["contacts_both_sides_one_step"] += 1
            if k == R["giver"] and sum(0 < f < 1 for f in s["factors"]) >= 2:
                before = ref["vel"][t - 1] if t else np.array([o["vel"] for o in spec["objects"]], np.float64)
                took = [(ref["vel"][t][R[role]] != before[R[role]]).any() for role in ("taker_low", "taker_high")]
                r["transfers_both_sides_one_step"] += all(took)
            r["movers_from_1024"] += k >= TILE and not s["blocked"]
    x, z = ref["pos"][:, R["mover_low"], 0], ref["pos"][:, R["mover_1024"], 2]
    # late_high comes into view at the script's tick; mover_low, before it in the order, still moves on then and stops a tick later
    seen = ref["visible"][:, R["late_high"]]
    r["visible_before_met"] = int(not seen[T - 1] and seen[T] and x[T] > x[T - 1] and x[T + 1] == x[T])
    # late_low likewise; mover_1024, after it in the order, stops at the script's tick
    seen = ref["visible"][:, R["late_low"]]
    r["visible_now_met"] = int(not seen[T - 1] and seen[T] and z[T - 1] > z[T - 2] and z[T] == z[T - 1])
    return {k: int(v) for k, v in r.items()}


def unchanged(path, out):
    """The file at `path` already holds exactly the arrays `out`: it is left as it is (a zip archive carries the time of writing)."""
    if not os.path.exists(path):
        return False
    z = np.load(path)
    if sorted(z.files) != sorted(out):
        return False
    return all(z[k].dtype == np.asarray(v).dtype and z[k].shape == np.asarray(v).shape and z[k].tobytes() == np.asarray(v).tobytes()
               for k, v in out.items())


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
        if name == "crowd":
            r.update(crowd_reach(ref, trace))
            short = {k: r[k] for k in CROWD_REACH if r[k] < 1}
            assert not short, "crowd does not reach what it is for: %r" % (r,)
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
        if unchanged(ps.fixture_path(name), out):
            print(os.path.relpath(ps.fixture_path(name), OUT), "unchanged")
            continue
        np.savez_compressed(ps.fixture_path(name), **out)
        print(os.path.relpath(ps.fixture_path(name), OUT), os.path.getsize(ps.fixture_path(name)), "bytes")


if __name__ == "__main__":
    main()
