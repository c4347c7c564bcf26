"""The scenes of tests/golden/physics_impulses.npz (tests/golden/make_physics_impulses.py records them from the real reference):
worlds in which bodies are accelerated between ticks -- Object.accelerate, as the reference's window calls it for its player after
every object's update, and mods for jumps, thrusters, wind and kicks.  Described with the vocabulary of tests/physics_scenes.py
-- the same dict, the same builder; tests/physics_scenes.py itself is untouched -- with one more op in the script:

    ["acc", i, vel]     before tick k: objects[i].accelerate(vec3(*vel))

The ops of a tick run in the order written, and ["cam", pos] keeps its meaning.  A scene may carry `alt`: further scripts by name,
each recorded as a run of its own (fixture key "<scene>@<alt>") -- the same world with the impulses left out, or in another order.
`follow` and `cam_vec` are those of tests/physics_follow_scenes.py: the camera is attached to that object and re-read every tick.
Plain data; nothing of the GPU is imported."""
import os

import physics_draw_scenes as ds
import physics_follow_scenes as fs
import physics_scenes as ps

P53 = ps.P53
PATH = os.path.join(ps.GOLDEN, "physics_impulses.npz")


def _script(script):
    return {str(k): v for k, v in script.items()}


def _with(spec, alt=None, **more):
    spec = dict(spec, **more)
    spec["alt"] = {name: _script(s) for name, s in (alt or {}).items()}
    return spec


# a cube at rest on a slab gets +y before tick 3, leaves the slab and lands again; without the impulse it ends elsewhere (the
# jump carries it along x, which friction holds while it rests)
JUMP = _with(ps.scene({"slab": ps.full((24, 2, 24), 0), "cube": ps.full((4, 4, 4), 1)},
                      [ps.obj("slab", (0, 0, 0), physics=False), ps.obj("cube", (0, 4, 0))], 12,
                      script={3: [["acc", 1, [0.75, 6.0, 0.0]]]}),
             alt={"without": {}})

# three impulses on one body before one tick: 1.0, 2^-53, 2^-53 ends at 1.0; the replay has them reversed and ends at 1 + 2^-52.
# No gravity, no air friction, nothing in the way: the velocity survives a tick as it is
ORDER = _with(ps.scene({"cube": ps.full((2, 2, 2), 0)}, [ps.obj("cube", (0, 0, 0)), ps.obj("cube", (0, 8, 0))], 4,
                       script={2: [["acc", 0, [1.0, 0, 0]], ["acc", 0, [P53, 0, 0]], ["acc", 0, [P53, 0, 0]], ["acc", 1, [0, 0, 0.5]]]},
                       gravity=0.0, friction_air=0.0),
              alt={"reversed": {2: [["acc", 1, [0, 0, 0.5]], ["acc", 0, [P53, 0, 0]], ["acc", 0, [P53, 0, 0]], ["acc", 0, [1.0, 0, 0]]]}})

# impulses on a body beyond dist_move, on a non-physical object and on an object without a sprite: the velocity is held and
# nothing moves; the sleeping body moves when the camera comes near and wakes it
ASLEEP = _with(ps.scene({"b0": ps.full((2, 2, 2), 0), "b1": ps.full((2, 2, 2), 1)},
                        [ps.obj("b0", (50, 0, 0)), ps.obj("b1", (5, 0, 0), physics=False), ps.obj(None, (0, 10, 0)), ps.obj("b1", (-6, 0, 0))], 8,
                        script={1: [["acc", 0, [0, 0, 1.5]], ["acc", 1, [1, 0, 0]], ["acc", 2, [0, 1, 0]]], 2: [["acc", 0, [0.25, 0, 0]]],
                                5: [["cam", [40.0, 0.0, 0.0]]]},
                        gravity=0.0, dist_move=32))
ASLEEP_ROLES = dict(sleeper=0, not_physical=1, no_sprite=2, wakes_at=5)

# one impulse before tick 0 and one before the last tick; the last one pushes the resting cube into the slab: it shows in the
# final velocity and in no position
ENDS = _with(ps.scene({"slab": ps.full((24, 2, 24), 0), "cube": ps.full((4, 4, 4), 1)},
                      [ps.obj("slab", (0, 0, 0), physics=False), ps.obj("cube", (0, 4, 0))], 6,
                      script={0: [["acc", 1, [1.5, 0, 0]]], 5: [["acc", 1, [0, -2.0, 0]]]}),
             alt={"without_last": {0: [["acc", 1, [1.5, 0, 0]]]}})

# an impulse on a body in contact with a physical neighbour: the transfer of data.py:523-527 hands part of it on in that tick
KICK = _with(ps.scene({"b0": ps.full((2, 2, 2), 0), "b1": ps.full((2, 2, 2), 1)},
                      [ps.obj("b0", (0, 0, 0)), ps.obj("b1", (3, 0, 0)), ps.obj("b1", (0, 0, 9))], 5,
                      script={1: [["acc", 0, [2.0, 0, 0]]]}, gravity=0.0))

# the seeded `fluid` scene of physics_draw_scenes.py with a thrust of four consecutive ticks on the cube of solidity 0.5, down
# into the pool and along it: from the first thrust tick on the draws per tick are no longer those of physics_fluid.npz
THRUST_TICKS = (3, 4, 5, 6)
WADE_THRUST = _with(dict(ds.FLUID, ticks=10, script=_script({k: [["acc", 2, [0.5, -6.0, 0.25]]] for k in THRUST_TICKS})))

# the scene of physics_follow_scenes.py with impulses on the followed cube: the camera goes where they take it
FOLLOW = _with(dict(fs.SCENE, script=_script({2: [["acc", fs.FOLLOW, [0.0, 0.0, 1.5]]], 9: [["acc", fs.FOLLOW, [-0.5, 3.0, 0.0]]]})))

SCENES = {"jump": JUMP, "order": ORDER, "asleep": ASLEEP, "ends": ENDS, "kick": KICK, "wade_thrust": WADE_THRUST, "follow": FOLLOW}


def runs():
    """Every recorded run: fixture key -> (scene name, spec with that run's script)."""
    out = {}
    for name, spec in SCENES.items():
        out[name] = (name, spec)
        for alt, script in spec["alt"].items():
            out["%s@%s" % (name, alt)] = (name, dict(spec, script=script))
    return out


def impulses_of(spec, objects, start=0, end=None):
    """The "acc" ops of ticks [start, end) as run(impulses=) takes them, ticks counted from `start`: [(tick, Object, vel)]."""
    end = spec["ticks"] if end is None else end
    return [(k - start, objects[op[1]], tuple(op[2])) for k in range(start, end) for op in spec["script"].get(str(k), ()) if op[0] == "acc"]


def segments(spec):
    """The run cut where the script moves the camera: [(first tick, end tick, camera position)] -- one run() call each."""
    cuts, cam, out = [0], {0: list(spec["cam"])}, []
    for k in range(spec["ticks"]):
        for op in spec["script"].get(str(k), ()):
            assert op[0] in ("acc", "cam"), op
            if op[0] == "cam":
                if k != cuts[-1]:
                    cuts.append(k)
                cam[k] = list(op[1])
    at = None
    for a, b in zip(cuts, cuts[1:] + [spec["ticks"]]):
        at = cam.get(a, at)
        out.append((a, b, at))
    return out
