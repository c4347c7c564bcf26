"""The scenes of tests/golden/physics_anim.npz: worlds with animated sprites (the reference's Sprite.anim_set / anim_update,
data.py:297-306, as Object.update calls it: data.py:575-582), described once for tests/golden/make_physics_anim.py, which
builds them from the real reference's classes under a scripted clock, and for the tests, which build them from this project's.
Plain data on top of tests/physics_scenes.py; nothing of the GPU is imported.

A scene is one of physics_scenes.py's with these additions: a sprite may have `frames`: one list of boxes per frame instead
of `boxes`, and `anim`: [frame_start, frame_end, frame_time] for anim_set; the scene has `clock`: [start_ms, step_ms] -- tick
k reads start_ms + k * step_ms -- and may have `follow` and `cam_vec` (the object that carries the camera, set_camera's offset).
There are no scripts: a run of many ticks is one segment.

  platform  two light 4^3 cubes rest on a 12 x 2 x 12 platform that blinks (frame 1 keeps one corner column only); one cube
            comes BEFORE the platform in the physics order and one after it.  In the tick of a switch the earlier cube still
            meets the old frame, the later one the new.  The platform is not physical: it switches and gets `redraw`.
  weights   twins: two bodies of one three-frame sprite (64, 32 and 16 voxels of the light material), played BACKWARDS, fall
            side by side onto a slab.  The first one makes every switch and is weighed anew; the second keeps the weight of frame
            0, falls by it, and meets the slab with a frame it was never weighed for.
  wake      a lamp that blinks every tick lies asleep, 40 below the cube that carries the camera (dist_move 24): its frame
            stays behind the schedule until the falling cube brings the camera near, and then the cube lands on it.
  crowd     1030 bodies of 2^3, all but a handful asleep, 3 ticks.  The blinking sprite is shown by body 5 and body 1029, both
            asleep, and by body 1027, awake: the body that switches it for all three.  Mover 7 (before the switch in the order)
            runs at body 1029 and mover 1028 (after it) at body 5: whether they get through depends on the frame the walk over
            ALL bodies, 1024 at a time, has written."""
import json
import os

import physics_scenes as ps

PATH = os.path.join(ps.GOLDEN, "physics_anim.npz")
TILE = 1024


def frames(size, per_frame, anim, lod=0):
    return dict(size=list(size), lod=lod, frames=per_frame, anim=list(anim))


def box(lo, hi, m):
    return [list(lo), list(hi), m]


def _platform():
    plat = frames((12, 2, 12), [[box((0, 0, 0), (11, 1, 11), 0)], [box((0, 0, 0), (1, 1, 1), 0)]], (0, 1, 0.2))
    spec = ps.scene({"plat": plat, "cube": ps.full((4, 4, 4), 3)},
                    [ps.obj("cube", (2, 3, 2)), ps.obj("plat", (0, 0, 0), physics=False), ps.obj("cube", (-3, 3, -2))], 14)
    spec["clock"] = [0, 50]
    return spec


def _weights():
    blob = frames((4, 4, 4), [[box((0, 0, 0), (3, 3, 3), 1)], [box((0, 2, 0), (3, 3, 3), 1)], [box((0, 0, 0), (3, 0, 3), 1)]], (0, 2, -0.15))
    spec = ps.scene({"blob": blob, "slab": ps.full((12, 2, 12), 0)},
                    [ps.obj("blob", (-3, 9, 0)), ps.obj("blob", (3, 9, 0)), ps.obj("slab", (0, 0, 0), physics=False)], 16)
    spec["clock"] = [1000, 100]
    return spec


def _wake():
    lamp = frames((8, 4, 8), [[box((0, 0, 0), (7, 3, 7), 0)], [box((0, 0, 0), (7, 1, 7), 1)]], (0, 1, 0.05))
    spec = ps.scene({"lamp": lamp, "cube": ps.full((4, 4, 4), 0)},
                    [ps.obj("lamp", (0, 0, 0), physics=False), ps.obj("cube", (0, 40, 0), rot=(0, 90, 0))], 24,
                    cam=(3.0, 44.0, 0.0), dist_move=24, dist_max=96)
    spec["clock"] = [0, 50]
    spec["follow"], spec["cam_vec"] = 1, [3, 4]
    return spec


CROWD_N = 1030
CROWD_ROLES = dict(blink_low=5, mover_low=7, switcher=1027, mover_high=1028, blink_high=1029)


def _crowd():
    blink = frames((2, 2, 2), [[box((0, 0, 0), (1, 1, 1), 0)], []], (0, 1, 0.05))
    sprites = {"dot": ps.full((2, 2, 2), 1), "blink": blink, "mover": ps.full((2, 2, 2), 3)}
    # (the filler stands on 32 spots, one dot inside the other: asleep and met by nobody, and the fixture stays small)
    objects = [ps.obj("dot", (-93 + 6 * (i % 32), -60, -90), physics=False) for i in range(CROWD_N)]
    R = CROWD_ROLES
    objects[R["blink_low"]] = ps.obj("blink", (10, 0, 0), physics=False)
    objects[R["blink_high"]] = ps.obj("blink", (-10, 0, 0), physics=False)
    objects[R["switcher"]] = ps.obj("blink", (0, 0, 4), physics=False)
    objects[R["mover_low"]] = ps.obj("mover", (-6.5, 0, 0), vel=(-1.5, 0, 0))
    objects[R["mover_high"]] = ps.obj("mover", (6.5, 0, 0), vel=(1.5, 0, 0))
    spec = ps.scene(sprites, objects, 3, gravity=0.0, dist_max=512, dist_move=8)
    spec["clock"] = [0, 50]
    return spec


SCENES = {"platform": _platform(), "weights": _weights(), "wake": _wake(), "crowd": _crowd()}

# (frame_start, frame_end, frame_time) for anim_set on a sprite of TABLE_FRAMES frames, and the clock readings each is asked at:
# forwards, backwards, fractional, very small and very long frame times, readings up to 2^40 ms
TABLE_FRAMES = 8
TABLE_ANIMS = [(0, 7, 0.1), (0, 7, -0.1), (2, 5, 0.033), (2, 5, -0.033), (1, 6, 1e-9), (1, 6, -1e-9), (0, 3, 0.0625), (3, 3, 0.5),
               (0, 6, 1e-3), (0, 6, -1e-3), (1, 7, 12345.678), (0, 7, 1 / 3), (0, 7, -1 / 3), (0, 4, 2.5e-4), (0, 7, 0.7)]
TABLE_NOWS = [0, 1, 2, 3, 7, 16, 33, 99, 100, 101, 199, 200, 333, 999, 1000, 1001, 4999, 65536, 123456789, 2 ** 31 - 1, 2 ** 31,
              2 ** 40 - 1, 2 ** 40]


def sprite_names(spec):
    """The sprites in the order the fixture's `frame` columns have."""
    return list(spec["sprites"])


def build(spec, Material, Sprite, Object, vec3, vec2, extra=None):
    """The scene from either set of classes: (objects in physics order, sprites by name, materials, followed object or None).
    anim_set is called on every sprite that has `anim`, set_camera on the followed object."""
    mats = [Material(**{**(extra(i) if extra else {}), **m}) for i, m in enumerate(spec["materials"])]
    sprites = {}
    for name, s in spec["sprites"].items():
        per_frame = s["frames"] if "frames" in s else [s["boxes"]]
        spr = Sprite(size=vec3(*s["size"]), frames=len(per_frame), lod=s["lod"])
        for f, boxes in enumerate(per_frame):
            for lo, hi, m in boxes:
                spr.get_frame(f).set_voxels({(x, y, z): mats[m] for x in range(lo[0], hi[0] + 1) for y in range(lo[1], hi[1] + 1)
                                             for z in range(lo[2], hi[2] + 1)}, True)
        if "anim" in s:
            spr.anim_set(*s["anim"])
        sprites[name] = spr
    objects = []
    for o in spec["objects"]:
        ob = Object(pos=vec3(*o["pos"]), rot=vec3(*o["rot"]), vel=vec3(*o["vel"]), physics=o["physics"])
        if o["sprite"] is not None:
            ob.set_sprite(sprites[o["sprite"]])
        objects.append(ob)
    who = None
    if "follow" in spec:
        who = objects[spec["follow"]]
        who.set_camera(vec2(*spec["cam_vec"]))
    return objects, sprites, mats, who


# ---- what the tests share --------------------------------------------------------------------------------------------------
_fixture = None


def load_fixture():
    """(the arrays of tests/golden/physics_anim.npz, {scene name: spec}), read once."""
    global _fixture
    if _fixture is None:
        import numpy as np
        z = np.load(PATH)
        _fixture = ({k: z[k] for k in z.files}, json.loads(bytes(z["spec"]).decode()))
    return _fixture


def project_scene(spec, extra=None):
    """The scene from this project's classes: (objects, sprites, materials, settings store, followed object or None)."""
    from python_raytracer_amd import Material, make_settings, world
    from python_raytracer_amd.lib import vec2, vec3
    objects, sprites, mats, who = build(spec, Material, world.Sprite, world.Object, vec3, vec2, extra)
    return objects, sprites, mats, make_settings(**spec["settings"]), who


def assert_ticks(z, name, spec, objects, sprites, trace, anim, what):
    """Every tick of a run that started from the scene's first state with `redraw` cleared: the records of world.run or
    DeviceWorld.run (trace, anim) against the fixture."""
    import numpy as np
    import physics_run_util as ru
    pre = name + "/"
    zz = {k[len(pre):]: v for k, v in z.items() if k.startswith(pre)}
    has_sprite = np.array([bool(o["sprite"]) for o in spec["objects"]])
    assert has_sprite.all()
    entry = dict(visible=np.zeros(len(objects), bool), redraw=np.zeros(len(objects), bool))
    # assert_segment derives `redraw` from moves and visibility; a switch sets it too, so it is taken out of the comparison there
    # and held to the fixture here
    seen = entry["visible"]
    names = sprite_names(spec)
    for k in range(spec["ticks"]):
        row, a = trace[k], anim[k]
        for f in ("pos", "vel"):
            assert np.array_equal(ru.bits(row[f]), ru.bits(zz[f][k])), "%s, tick %d: %s" % (what, k, f)
        for f in ("mins", "maxs"):
            assert np.array_equal(row[f], zz[f][k]), "%s, tick %d: %s" % (what, k, f)
        visible = row["visible"] != 0
        assert np.array_equal(visible, zz["visible"][k]), "%s, tick %d: visible" % (what, k)
        redraw = (row["moved"] != 0) | (visible != seen) | (a["switched"] != 0)
        assert np.array_equal(redraw, zz["redraw"][k]), "%s, tick %d: redraw\n%r\n%r" % (what, k, redraw, zz["redraw"][k])
        assert np.array_equal(ru.bits(a["weight"]), ru.bits(zz["weight"][k])), "%s, tick %d: weight" % (what, k)
        for c, sname in enumerate(names):
            shown = [i for i, o in enumerate(spec["objects"]) if o["sprite"] == sname]
            want = int(zz["frame"][k][c]) if "anim" in spec["sprites"][sname] else -1
            assert all(int(a["frame"][i]) == want for i in shown), "%s, tick %d: frame of %s" % (what, k, sname)
            assert "anim" in spec["sprites"][sname] or zz["frame"][k][c] == 0
        seen = visible
    assert [int(sprites[s].frame) for s in names] == zz["frame"][-1].tolist(), what
    assert np.array_equal(ru.bits([float(o.weight) for o in objects]), ru.bits(zz["weight"][-1])), what


def fresh(name):
    """The scene from this project's classes as a run finds it, `redraw` cleared: (fixture arrays, spec, objects, sprites,
    settings store, followed object or None)."""
    import numpy as np
    import physics_run_util as ru
    z, specs = load_fixture()
    spec = specs[name]
    objects, sprites, _, st, who = project_scene(spec)
    assert np.array_equal(ru.bits([float(o.weight) for o in objects]), ru.bits(z[name + "/weight0"]))
    ps.clear_redraw(objects)
    return z, spec, objects, sprites, st, who
