"""The scenes of the physics fixtures (tests/golden/physics_*.npz), described once: tests/golden/make_physics.py builds them
from the real reference's classes and records what its Object.update does tick by tick, the tests build them from this project's
classes and hold world.tick and DeviceWorld.tick to the records.  Plain data and one builder that works on either set of
classes (they take the same keyword arguments); nothing of the GPU is imported.

A scene: settings (the [PHYSICS] keys and dist_max), the camera position, materials (solidity, weight, friction, elasticity),
sprites (a Goxel file with a colour map, or filled boxes [lo, hi, material] applied in order, material None = dug out again),
objects in PHYSICS ORDER (sprite name or None, pos, rot, vel, physics), the number of ticks, and a script: before tick k,
["move", i, pos] teleports object i (Object.move), ["vel", i, vel] replaces its velocity, ["cam", pos] moves the camera.
Except in the default mod every weight, friction and elasticity is a dyadic rational, so a weight sum cannot depend on the voxel
order -- a friction sum still can: P53 = 2^-53 under 1.0 is lost when added after it and kept when added before."""
import os

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MOD_VOXELS = os.path.join(GOLDEN, "mod_default", "voxels")

P53 = 2.0 ** -53
BASE = dict(gravity=1.0, friction=1.0, friction_air=0.125, min_velocity=2.0 ** -7, max_velocity=8.0, dist_move=64, dist_max=96)


def mat(solidity=1, weight=2.0 ** -4, friction=0.5, elasticity=0.0):
    return dict(solidity=solidity, weight=weight, friction=friction, elasticity=elasticity)


# the materials every synthetic scene shares, by index
MATS = [mat(),                                             # 0 plain
        mat(weight=2.0 ** -5, friction=0.25, elasticity=0.25),   # 1 light
        mat(weight=2.0 ** -6, friction=0.0, elasticity=0.5),     # 2 elastic, no friction
        mat(weight=2.0 ** -8, friction=1.0),                     # 3 friction 1
        mat(weight=2.0 ** -8, friction=P53),                     # 4 friction 2^-53
        mat(solidity=0, weight=2.0 ** -4),                       # 5 not solid
        mat(solidity=0.5, weight=2.0 ** -4)]                     # 6 solid every other time (host path only)


def full(size, m=0, lod=0):
    return dict(size=list(size), lod=lod, boxes=[[[0, 0, 0], [size[0] - 1, size[1] - 1, size[2] - 1], m]])


def obj(sprite, pos, vel=(0, 0, 0), physics=True, rot=(0, 0, 0)):
    return dict(sprite=sprite, pos=list(pos), rot=list(rot), vel=list(vel), physics=physics)


def scene(sprites, objects, ticks, script=None, cam=(0.0, 0.0, 0.0), seed=None, **settings):
    return dict(settings={**BASE, **settings}, cam=list(cam), materials=MATS, sprites=sprites, objects=objects, ticks=ticks,
                script={str(k): v for k, v in (script or {}).items()}, seed=seed)


# an L-shaped 4^3 model and a stepped 8 x 4 x 6 one: no quarter turn maps either onto itself
ELL = dict(size=[4, 4, 4], lod=0, boxes=[[[0, 0, 0], [3, 0, 3], 0], [[0, 0, 0], [0, 3, 1], 1], [[3, 1, 3], [3, 2, 3], 0]])
STEPS = dict(size=[8, 4, 6], lod=0, boxes=[[[0, 0, 0], [7, 1, 5], 0], [[0, 2, 0], [3, 3, 2], 1], [[6, 2, 4], [7, 2, 5], 0]])
FAR = float(2 ** 27)

EDGES = {
    # a 2^3 sprite: the slab under it is one column wide on each side of its box
    "tiny": scene({"tiny": full((2, 2, 2)), "slab": full((16, 2, 16))},
                  [obj("slab", (0, 0, 0), physics=False), obj("tiny", (0, 5, 0))], 10),
    # a 40 x 34 face resting on a floor: 1360 contacts in a slab of 41 x 2 x 35 voxels, three passes of 1024; the floor's first
    # row has friction 1 and the rest 2^-53, so the order of the sum shows
    "face": scene({"face": full((40, 2, 34), 3),
                   "floor": dict(size=[48, 2, 40], lod=0, boxes=[[[0, 0, 0], [47, 1, 39], 4], [[0, 0, 0], [5, 1, 39], 3]])},
                  [obj("face", (0, 3.5, 0)), obj("floor", (0, 0, 0), physics=False)], 6),
    # ties: (0.5, 0.5, 0) flies free, (-1, 1, 1) meets a block that only the x slab sees
    "ties": scene({"cube": full((4, 4, 4)), "block": full((2, 8, 8), 1)},
                  [obj("cube", (0, 0, 0), vel=(0.5, 0.5, 0)), obj("cube", (20, 0, 0), vel=(-1, 1, 1)),
                   obj("block", (15, 2, 2), physics=False)], 6, gravity=0.0),
    # |vel| = 3.7: two free steps, blocked on the third
    "fast": scene({"cube": full((4, 4, 4)), "wall": full((2, 8, 8), 1)},
                  [obj("cube", (0, 0, 0), vel=(3.7, 0, 0)), obj("wall", (5, 0, 0), physics=False)], 3, gravity=0.0),
    # two rotated movers over a rotated obstacle; the obstacle's turn about y is one the size rule ignores (8 != 6), the
    # second mover's about x and z both count
    "rot": scene({"ell": ELL, "steps": STEPS},
                 [obj("steps", (0, 0, 0), physics=False, rot=(0, 90, 0)), obj("ell", (-2, 7, 0), rot=(0, 90, 0)),
                  obj("ell", (2, 8, 1), rot=(90, 0, 180)), obj("ell", (2, 14, 1), rot=(0, 0, 270))], 12),
    # sprites of lod 1: cells of 2^3 voxels
    "lod": scene({"pad": full((8, 4, 8), 1, lod=1),
                  "knob": dict(size=[4, 4, 4], lod=1, boxes=[[[0, 0, 0], [3, 1, 3], 0], [[0, 2, 0], [1, 3, 1], 0]])},
                 [obj("pad", (0, 0, 0), physics=False), obj("knob", (1, 7, 1)), obj("knob", (-2, 12, -1), rot=(0, 180, 0))], 12),
    # transfer chains A -> B -> C within one tick: B listed before A (first row), and after it (second row)
    "chain": scene({"b0": full((2, 2, 2), 0), "b1": full((2, 2, 2), 1), "b2": full((2, 2, 2), 2)},
                   [obj("b1", (3, 0, 0)), obj("b0", (0, 0, 0), vel=(2, 0, 0)), obj("b2", (6, 0, 0)),
                    obj("b0", (0, 0, 20), vel=(2, 0, 0)), obj("b1", (3, 0, 20)), obj("b2", (6, 0, 20))], 8, gravity=0.0),
    # dist_max 16: the small obstacle at distance 18 is invisible (18 > 16 + 1) and passed through; the bar is moved into view,
    # right in front of the mover, before tick 3 and is still not there for the mover, which comes before it in the order,
    # until tick 4 blocks on it
    "vis": scene({"long": full((32, 4, 4)), "dot": full((2, 2, 2), 1), "bar": full((8, 2, 2), 1)},
                 [obj("long", (-2, 0, 0), vel=(1.5, 0, 0)), obj("dot", (18, 0, 0), physics=False),
                  obj("bar", (60, 30, 0), physics=False)], 8, script={3: [["move", 2, [20, 0, 0]]]}, gravity=0.0, dist_max=16),
    # asleep (further than dist_move), yet it takes the velocity an awake neighbour hands it; and an object without a sprite
    "sleep": scene({"b0": full((2, 2, 2), 0), "b1": full((2, 2, 2), 1)},
                   [obj("b1", (33, 0, 0), vel=(0, 0.5, 0)), obj("b0", (30, 0, 0), vel=(2, 0, 0)), obj(None, (5, 0, 0), vel=(1, 0, 0)),
                    obj("b0", (-20, 0, 0), vel=(0, 0, 1.25))], 6, gravity=0.0, dist_move=32),
    # at 2^27 with a fraction: the spacing of binary64 there is 2^-25
    "far": scene({"cube": full((4, 4, 4)), "slab": full((16, 2, 16), 1)},
                 [obj("slab", (FAR, 0, 0), physics=False), obj("cube", (FAR + 0.25, 6.25, 0.5), vel=(0.375, 0, 0))], 10,
                 cam=(FAR, 0.0, 0.0)),
    # a non-physical obstacle the script teleports under a falling body, and away again
    "teleport": scene({"cube": full((4, 4, 4)), "shelf": full((8, 2, 8), 1), "slab": full((16, 2, 16))},
                      [obj("cube", (0, 20, 0)), obj("shelf", (30, 14, 0), physics=False), obj("slab", (0, 0, 0), physics=False)], 16,
                      script={2: [["move", 1, [0, 13, 0]]], 8: [["move", 1, [30, 14, 0]]]}),
    # elasticity > 0 and friction 0 on both sides; and a material that is not solid at all, which holds nothing up
    "elastic": scene({"ball": full((4, 4, 4), 2), "bed": full((12, 2, 12), 2), "ghost": full((12, 2, 12), 5)},
                     [obj("ghost", (0, 6, 0), physics=False), obj("bed", (0, 0, 0), physics=False),
                      obj("ball", (0, 12, 0), vel=(0.25, 0, 0))], 14),
}

# fractional solidity: the host path only, with the reference's draws
FRACTION = scene({"cube": full((4, 4, 4), 6), "slab": full((12, 2, 12), 6)},
                 [obj("slab", (0, 0, 0), physics=False), obj("cube", (0, 6, 0)), obj("cube", (3, 12, 1))], 16, seed=20251)


def _pile():
    sprites = {"s0": full((2, 2, 2), 0), "s1": full((2, 2, 2), 1), "m0": full((4, 4, 4), 1), "m2": full((4, 2, 4), 2),
               "slab": full((32, 2, 32), 0)}
    objects = [obj("slab", (0, 0, 0), physics=False)]
    names = ["s0", "s1", "m0", "m2"]
    for i in range(24):
        col, layer = i % 8, i // 8
        x, z = -9 + 6 * (col % 4) + (layer % 2), -4 + 8 * (col // 4) + (layer // 2)
        objects.append(obj(names[(i * 7 + layer) % 4], (x, 5 + 6 * layer + (i % 3) * 0.5, z), vel=(0.25 * ((i % 5) - 2), 0, 0.125 * ((i % 3) - 1))))
    return scene(sprites, objects, 30)


PILE = _pile()

# More bodies than one tile of the device's walk over them (vrt_physics.hip: VRT_PHYS_BLOCK = 1024 bodies at a time, the
# validation loop strides alike).  CROWD_ROLES: where the bodies that matter stand in the physics order, on both sides of 1024.
CROWD_N = 1100
CROWD_ROLES = dict(block_low=1, bar=2, taker_low=5, mover_low=7, late_low=9, mover_1024=1024, block_high=1050, giver=1060,
                   taker_high=1080, late_high=1090)
CROWD_SCRIPT_TICK = 2


def _crowd():
    """1100 objects, 4 ticks, no gravity, everything within dist_max and dist_move of the camera but the two parked obstacles.
    1090 static 2^3 dots stand on a lattice at y = -60, out of the way.  Every object starts with visible = False, so what a body
    meets at a HIGHER index it meets from tick 1 on: the stations below play at ticks 1 to 3.
      bar (2)         12 x 2 x 2 of friction 1, falls (tick 0: free; tick 1: one free step, then blocked) on block_low (1: two
                      contacts of friction 1, terms 1.0) and block_high (1050: eight contacts of friction 2^-53) in one step: the
                      sum is 2.0 in the order of the indices and 2 + 2^-50 the other way round
      giver (1060)    a light 4^3 cube at 1.25 along x: at tick 1 its slab meets taker_low (5) and taker_high (1080) side by side,
                      and both take velocity in the same step, by factors inside (0, 1)
      mover_low (7)   a 4^3 cube at 1.5 along x; before tick 2 the script moves late_high (1090, parked out of sight) right in
                      front of it: not yet visible for a mover BEFORE it in the order (last tick's flag), which moves on into it
                      and is blocked at tick 3
      mover_1024      a 4^3 cube at 1.5 along z; before tick 2 late_low (9) is moved in front of it: already visible for a mover
                      AFTER it in the order (this tick's flag), which is blocked at tick 2"""
    sprites = {"dot": full((2, 2, 2), 1), "dot0": full((2, 2, 2), 0), "dot2": full((2, 2, 2), 2), "dot3": full((2, 2, 2), 3),
               "cube": full((4, 4, 4), 0), "cube2": full((4, 4, 4), 2), "bar": full((12, 2, 2), 3), "block4": full((4, 2, 2), 4)}
    objects = [obj("dot", (-99 + 6 * (i % 34), -60, -99 + 6 * (i // 34)), physics=False) for i in range(CROWD_N)]
    R = CROWD_ROLES
    objects[R["block_low"]] = obj("dot3", (-5, 0, -1), physics=False)
    objects[R["block_high"]] = obj("block4", (4, 0, 0), physics=False)
    objects[R["bar"]] = obj("bar", (0, 4.5, 0), vel=(0, -1.5, 0))
    objects[R["giver"]] = obj("cube2", (58.75, 0, 0), vel=(1.25, 0, 0))
    objects[R["taker_low"]] = obj("dot0", (64, 0, -1))
    objects[R["taker_high"]] = obj("dot2", (64, 0, 2))
    objects[R["mover_low"]] = obj("cube", (-60, 0, 0), vel=(1.5, 0, 0))
    objects[R["late_high"]] = obj("dot", (0, 2000, 0), physics=False)
    objects[R["mover_1024"]] = obj("cube", (0, 0, 60), vel=(0, 0, 1.5))
    objects[R["late_low"]] = obj("dot", (40, 2000, 0), physics=False)
    script = {CROWD_SCRIPT_TICK: [["move", R["late_high"], [-54, 0, 0]], ["move", R["late_low"], [0, 0, 66]]]}
    return scene(sprites, objects, 4, script=script, gravity=0.0, dist_max=512, dist_move=512)


CROWD = _crowd()

# mods/default/init.py:6-214: the physics properties of its materials, its sprites and where its objects stand
DEFAULT_MATS = dict(stone_marble=mat(1, 0.0025, 0.125, 0), stone_light=mat(1, 0.0025, 0.25, 0), stone_gray=mat(1, 0.0025, 0.375, 0),
                    stone_dark=mat(1, 0.0025, 0.5, 0), metal=mat(1, 0.0025, 0.125, 0), material=mat(1, 0.0005, 0.5, 0),
                    material_rough=mat(1, 0.0005, 1, 0.25), material_light=mat(1, 0.00025, 0.5, 0.25),
                    material_scatter=mat(1, 0.0005, 1, 0.5), material_glass=mat(1, 0.00125, 0, 0), material_shiny=mat(1, 0.00125, 0.25, 0),
                    material_mist=mat(1, 0.00025, 0, 1), player=mat(1, 0.0005, 0.1, 0.5))
_NAMES = list(DEFAULT_MATS)


def _default():
    idx = {n: i for i, n in enumerate(_NAMES)}
    sprites = {"castle": dict(size=[128, 64, 128], lod=0, file="castle.txt.gz",
                              cmap={"000000": idx["metal"], "3f3f3f": idx["stone_dark"], "7f7f7f": idx["stone_gray"],
                                    "bfbfbf": idx["stone_light"], "ffffff": idx["stone_marble"]}),
               "player": dict(size=[12, 16, 12], lod=0, file="player.txt.gz", cmap={"7f7f7f": idx["player"]})}
    objects = [obj("castle", (0, 0, 0), physics=False)]
    for special, pos in (("rough", (-56, -16, 56)), ("light", (12, -24, 24)), ("scatter", (48, -24, -48)), ("glass", (-4, 18, 16)),
                         ("shiny", (-56, 18, 16)), ("mist", (-36, 18, -36))):
        sprites[special] = dict(size=[12, 12, 12], lod=0, file="material.txt.gz",
                                cmap={"7f7f7f": idx["material"], "ffffff": idx["material_" + special]})
        objects.append(obj(special, pos))
    objects.append(obj("player", (-12, 0, -8)))
    # the camera stands where the player's attachment puts it at the start (set_camera(vec2(12, 4)), data.py:614-618)
    return dict(settings=dict(gravity=1.0, friction=1.0, friction_air=0.1, min_velocity=0.01, max_velocity=10.0, dist_move=64, dist_max=192),
                cam=[-12.0, 4.0, 4.0], materials=[DEFAULT_MATS[n] for n in _NAMES], sprites=sprites, objects=objects, ticks=40,
                script={}, seed=None)


DEFAULT = _default()

# fixture file (tests/golden/physics_<name>.npz) -> scene
SCENES = {"default": DEFAULT, "pile": PILE, "fraction": FRACTION, **{"edges_" + k: v for k, v in EDGES.items()}, "crowd": CROWD}
DEVICE_SCENES = [n for n in SCENES if n != "fraction"]


def fixture_path(name):
    return os.path.join(GOLDEN, "physics_%s.npz" % name)


def build(spec, Material, Sprite, Object, vec3, extra=None):
    """The scene from either set of classes: (objects in physics order, sprites by name, materials).  extra: attributes every
    Material gets besides the four physical ones (the renderer's, where the scene is also drawn)."""
    mats = [Material(**{**(extra(i) if extra else {}), **m}) for i, m in enumerate(spec["materials"])]
    sprites = {}
    for name, s in spec["sprites"].items():
        spr = Sprite(size=vec3(*s["size"]), frames=1, lod=s["lod"])
        if "file" in s:
            spr.load([os.path.join(MOD_VOXELS, s["file"])], {c: mats[i] for c, i in s["cmap"].items()})
        else:
            for lo, hi, m in s["boxes"]:
                spr.get_frame(0).set_voxels({(x, y, z): (mats[m] if m is not None else None) for x in range(lo[0], hi[0] + 1)
                                             for y in range(lo[1], hi[1] + 1) for z in range(lo[2], hi[2] + 1)}, True)
        sprites[name] = spr
    objects = []
    for o in spec["objects"]:
        ob = Object(pos=vec3(*o["pos"]), rot=vec3(*o["rot"]), vel=vec3(*o["vel"]), physics=o["physics"])
        if o["sprite"] is not None:
            ob.set_sprite(sprites[o["sprite"]])
        objects.append(ob)
    return objects, sprites, mats


def apply_script(spec, k, objects, vec3, cam):
    """Tick k's script on the objects; returns the camera position (a list) for the tick."""
    for op in spec["script"].get(str(k), ()):
        if op[0] == "move":
            objects[op[1]].move(vec3(*op[2]))
        elif op[0] == "vel":
            objects[op[1]].vel = vec3(*op[2])
        elif op[0] == "cam":
            cam = list(op[1])
        else:
            raise AssertionError(op)
    return cam


def clear_redraw(objects):
    """What the renderer does between ticks: an object that has a sprite is voxelised again and its flag cleared."""
    for o in objects:
        if o.sprite:
            o.redraw = False


# ---- what the tests share: the recorded runs, this project's objects for a scene, and the comparison ---------------------------
def load_fixture(name):
    """(the arrays of tests/golden/physics_<name>.npz, its scene)."""
    import json
    import numpy as np
    z = np.load(fixture_path(name))
    return z, json.loads(bytes(z["spec"]).decode())


def project_scene(spec, extra=None):
    """The scene from this project's classes: (objects, sprites, materials, settings store)."""
    from python_raytracer_amd import Material, make_settings, world
    from python_raytracer_amd.lib import vec3
    objects, sprites, mats = build(spec, Material, world.Sprite, world.Object, vec3, extra)
    return objects, sprites, mats, make_settings(**spec["settings"])


def state(objects):
    """The recorded fields of the objects as arrays: dict(pos, vel, mins, maxs, visible, redraw)."""
    import numpy as np
    return dict(pos=np.array([[float(c) for c in o.pos.tuple()] for o in objects], np.float64).reshape(-1, 3),
                vel=np.array([[float(c) for c in o.vel.tuple()] for o in objects], np.float64).reshape(-1, 3),
                mins=np.array([[int(c) for c in o.mins.tuple()] for o in objects], np.int64).reshape(-1, 3),
                maxs=np.array([[int(c) for c in o.maxs.tuple()] for o in objects], np.int64).reshape(-1, 3),
                visible=np.array([bool(o.visible) for o in objects], bool), redraw=np.array([bool(o.redraw) for o in objects], bool))


def assert_tick(z, k, objects, what):
    """The objects are what the reference's were after tick k: every field, the doubles bit for bit."""
    import numpy as np
    got = state(objects)
    for f, v in got.items():
        want = z[f][k]
        same = np.array_equal(v.view(np.uint64), want.view(np.uint64)) if v.dtype == np.float64 else np.array_equal(v, want)
        assert same, "%s, tick %d: %s\n%r\n%r" % (what, k, f, v, want)
