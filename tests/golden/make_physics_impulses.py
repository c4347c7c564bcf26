#!/usr/bin/env python3
"""Generate tests/golden/physics_impulses.npz: the reference's own physics with bodies accelerated between ticks, observed tick by
tick on the scenes of tests/physics_impulse_scenes.py.

Needs the reference checkout make_golden.py needs; the test-suite only reads the committed output.  Nothing of the reference is
copied: its modules are imported in place (make_golden.load_reference), the scenes are built from ITS Material, Sprite and
Object, every tick is `for obj in objects: obj.update(cam)` (init.py:469-470), and before a tick the scene's script calls ITS
Object.accelerate (data.py:491-492) -- where the reference's window calls it: after every object's update of the tick before.

For every run R (a scene, or a scene with one of its `alt` scripts: "<scene>@<alt>"):
    R/pos, R/vel         float64 [ticks, objects, 3]   after every tick
    R/mins, R/maxs       int64   [ticks, objects, 3]
    R/visible            bool    [ticks, objects]
    R/draws              int64   [ticks]               random.random() calls of the tick (seeded scenes only)
    R/cam                float64 [ticks, 3]            the camera each tick was given
and once: spec (JSON: every scene), reached (JSON: what the runs showed, below).

After the reference's run the same run goes through this project's host path (world.tick, Object.accelerate) and must agree with
it bit for bit in every recorded field and in the draws.  The file is written ONLY IF the scenes show what they are named for
(shows(), below), and only within LIMIT bytes.

Usage:  python tests/golden/make_physics_impulses.py
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

from make_physics import unchanged  # noqa: E402

LIMIT = 400000
FIELDS = ("pos", "vel", "mins", "maxs", "visible")


def observe(objects, rec):
    rec["pos"].append([[float(c) for c in (o.pos.x, o.pos.y, o.pos.z)] for o in objects])
    rec["vel"].append([[float(c) for c in (o.vel.x, o.vel.y, o.vel.z)] for o in objects])
    rec["mins"].append([[int(c) for c in (o.mins.x, o.mins.y, o.mins.z)] for o in objects])
    rec["maxs"].append([[int(c) for c in (o.maxs.x, o.maxs.y, o.maxs.z)] for o in objects])
    rec["visible"].append([bool(o.visible) for o in objects])


def arrays(rec, n, cams, draws):
    out = dict(pos=np.array(rec["pos"], np.float64).reshape(-1, n, 3), vel=np.array(rec["vel"], np.float64).reshape(-1, n, 3),
               mins=np.array(rec["mins"], np.int64).reshape(-1, n, 3), maxs=np.array(rec["maxs"], np.int64).reshape(-1, n, 3),
               visible=np.array(rec["visible"], bool).reshape(-1, n), cam=np.array(cams, np.float64).reshape(-1, 3))
    if draws is not None:
        out["draws"] = np.array(draws, np.int64)
    return out


def script_tick(spec, k, objects, vec3, cam):
    """Tick k's script: the reference's (or this project's) Object.accelerate for ["acc", i, vel], the camera for ["cam", pos]."""
    for op in spec["script"].get(str(k), ()):
        if op[0] == "acc":
            objects[op[1]].accelerate(vec3(*op[2]))
        elif op[0] == "cam":
            cam = list(op[1])
        else:
            raise AssertionError(op)
    return cam


def run_ticks(spec, objects, vec3, vec2, draw_count):
    """The loop both sets of classes go through.  draw_count(): the draws made so far, or None."""
    import physics_scenes as ps
    player = None
    if "follow" in spec:
        player = objects[spec["follow"]]
        player.set_camera(vec2(*spec["cam_vec"]))
    rec, cams, draws = {k: [] for k in FIELDS}, [], []
    cam = spec["cam"]
    for k in range(spec["ticks"]):
        ps.clear_redraw(objects)
        cam = script_tick(spec, k, objects, vec3, cam)
        at = player.cam_pos if player is not None else vec3(*cam)
        cams.append([float(c) for c in at.tuple()])
        before = draw_count()
        for o in objects:
            o.update(at)
        if before is not None:
            draws.append(draw_count() - before)
        observe(objects, rec)
    return arrays(rec, len(objects), cams, draws if spec["seed"] is not None else None)


def run_reference(data, lib, spec):
    import physics_scenes as ps
    data.objects.clear()
    for k, v in spec["settings"].items():
        setattr(data.settings, k, v)
    objects, _, _ = ps.build(spec, data.Material, data.Sprite, data.Object, lib.vec3)
    assert list(data.objects.values()) == objects
    if "follow" in spec:
        data.player = objects[spec["follow"]]
    made, real = [0], random.random

    def counted():
        made[0] += 1
        return real()

    if spec["seed"] is not None:
        random.seed(spec["seed"])
        random.random = counted
    try:
        return run_ticks(spec, objects, lib.vec3, lib.vec2, lambda: made[0] if spec["seed"] is not None else None)
    finally:
        random.random = real


def run_host(spec):
    """The same loop on this project's classes: world.Object.update is tick()'s loop body without draws; with a seed the draws
    come from random.Random(seed), counted."""
    import physics_scenes as ps
    from python_raytracer_amd import Material, make_settings, world
    from python_raytracer_amd.lib import vec2, vec3
    objects, _, _ = ps.build(spec, Material, world.Sprite, world.Object, vec3)
    st = make_settings(**spec["settings"])
    gen = random.Random(spec["seed"]) if spec["seed"] is not None else None
    made = [0]

    def draw():
        made[0] += 1
        return gen.random()

    class Updating:
        """An object whose update(cam) is this project's Object._update against all the objects"""
        def __init__(self, o):
            self.__dict__["o"] = o

        def __getattr__(self, name):
            return getattr(self.__dict__["o"], name)

        def __setattr__(self, name, value):
            setattr(self.__dict__["o"], name, value)

        def update(self, cam):
            self.__dict__["o"]._update(cam, st, objects, draw if gen else None)

    return run_ticks(spec, [Updating(o) for o in objects], vec3, vec2, lambda: made[0] if gen else None)


def shows(ref, committed_fluid_draws):
    """What each scene is named for, from the reference's records; every value must be true."""
    import physics_impulse_scenes as sc
    r = {}
    bits = lambda a: np.asarray(a, np.float64).view(np.uint64)  # noqa: E731
    # jump: at rest before the impulse, leaves the slab, lands again, and ends elsewhere than the run without
    j, w = ref["jump"], ref["jump@without"]
    y = j["pos"][:, 1, 1]
    r["jump_at_rest_before"] = bool((j["pos"][2, 1] == j["pos"][1, 1]).all() and (j["pos"][2] == w["pos"][2]).all())
    r["jump_leaves_the_slab"] = bool(y[3:].max() > y[2] + 1)
    r["jump_lands_again"] = bool(y[-1] == y[-2] == y[-3] and j["mins"][-1, 1, 1] == j["mins"][2, 1, 1])
    r["jump_ends_elsewhere"] = bool((j["pos"][-1, 1] != w["pos"][-1, 1]).any())
    # order: the two final velocities differ in the last bit, the other body's do not
    o, v = ref["order"], ref["order@reversed"]
    r["order_last_bit"] = bool(o["vel"][-1, 0, 0] == 1.0 and v["vel"][-1, 0, 0] == 1.0 + 2.0 ** -52)
    r["order_other_body_commutes"] = bool((bits(o["vel"][:, 1]) == bits(v["vel"][:, 1])).all() and o["vel"][-1, 1, 2] != 0)
    # asleep: velocity held, nothing moves, until the camera wakes the sleeper
    a, R = ref["asleep"], sc.ASLEEP_ROLES
    wake = R["wakes_at"]
    held = [R["sleeper"], R["not_physical"], R["no_sprite"]]
    r["asleep_velocity_held"] = bool((a["vel"][2:wake, held] == a["vel"][2, held]).all() and (a["vel"][2, held] != 0).any(axis=1).all())
    r["asleep_nothing_moves"] = bool((a["pos"][:wake, held] == a["pos"][0, held]).all())
    r["asleep_two_impulses_summed"] = bool(a["vel"][2, R["sleeper"], 0] == 0.25 and a["vel"][2, R["sleeper"], 2] == 1.5)
    r["asleep_sleeper_moves_when_woken"] = bool((a["pos"][wake, R["sleeper"]] != a["pos"][0, R["sleeper"]]).any())
    r["asleep_others_never_move"] = bool((a["pos"][:, held[1:]] == a["pos"][0, held[1:]]).all() and (a["vel"][-1, held[1:]] != 0).any(axis=1).all())
    # ends: the first impulse moves the cube in tick 0; the last shows in the final velocity and in no position
    e, w = ref["ends"], ref["ends@without_last"]
    r["ends_first_moves_at_tick_0"] = bool(e["pos"][0, 1, 0] != 0)
    r["ends_last_in_no_position"] = bool((bits(e["pos"]) == bits(w["pos"])).all())
    r["ends_last_in_final_velocity"] = bool((bits(e["vel"][-1, 1]) != bits(w["vel"][-1, 1])).any() and (bits(e["vel"][:-1]) == bits(w["vel"][:-1])).all())
    # kick: the neighbour takes velocity in the tick of the kick
    k = ref["kick"]
    r["kick_handed_on_in_that_tick"] = bool((k["vel"][0] == 0).all() and k["vel"][1, 1, 0] > 0 and k["vel"][1, 0, 0] > 0 and (k["vel"][:, 2] == 0).all())
    # wade_thrust: the draws are the committed fluid run's before the thrust and not from its first tick on
    t, first = ref["wade_thrust"], sc.THRUST_TICKS[0]
    r["thrust_draws_as_committed_before"] = bool((t["draws"][:first] == committed_fluid_draws[:first]).all())
    r["thrust_draws_differ_from_first_tick"] = bool(t["draws"][first] != committed_fluid_draws[first])
    # follow: the camera goes where the impulses take the followed body
    f = ref["follow"]
    r["follow_camera_moves_along_z"] = bool(abs(f["cam"][-1, 2] - f["cam"][0, 2]) > 1 and f["pos"][-1, sc.fs.FOLLOW, 2] != 0)
    return r


def main():
    import physics_impulse_scenes as sc
    import physics_scenes as ps
    data, lib, mod = load_reference()
    ref = {}
    for key, (name, spec) in sc.runs().items():
        spec = json.loads(json.dumps(spec))
        ref[key] = run_reference(data, lib, spec)
        got = run_host(spec)
        assert sorted(got) == sorted(ref[key])
        for f, v in ref[key].items():
            same = np.array_equal(v.view(np.uint64), got[f].view(np.uint64)) if v.dtype == np.float64 else np.array_equal(v, got[f])
            assert same, "%s: the host path's %s differs from the reference's" % (key, f)
        print("%-22s %2d ticks %d objects%s" % (key, spec["ticks"], len(spec["objects"]),
                                                 "; draws %s" % ref[key]["draws"].tolist() if "draws" in ref[key] else ""))
    fluid = np.load(ps.fixture_path("fluid"))["draws"]
    reached = shows(ref, fluid)
    for k, v in reached.items():
        print("  %-40s %s" % (k, v))
    short = [k for k, v in reached.items() if not v]
    assert not short, "the scenes do not show what they are named for: %r" % (short,)
    out = {"%s/%s" % (key, f): v for key, rec in ref.items() for f, v in rec.items()}
    out["spec"] = np.frombuffer(json.dumps(sc.SCENES).encode(), np.uint8)
    out["reached"] = np.frombuffer(json.dumps(reached).encode(), np.uint8)
    if unchanged(sc.PATH, out):
        print(os.path.relpath(sc.PATH, OUT), "unchanged")
        return
    np.savez_compressed(sc.PATH, **out)
    size = os.path.getsize(sc.PATH)
    print(os.path.relpath(sc.PATH, OUT), size, "bytes")
    if size > LIMIT:
        os.remove(sc.PATH)
        raise AssertionError("the fixture would be %d bytes, more than %d" % (size, LIMIT))


if __name__ == "__main__":
    main()
