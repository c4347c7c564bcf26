"""The flags of the multi-tick run at their limits (tests/golden/run_flags.npz, tests/golden/make_run_flags.py,
tests/physics_flags_scene.py): 1100 bodies that stand at a distance from the camera equal to dist_move or to dist_max +
max(half extent), one double below it or one double above it, where visibility and sleep hang on the last bit of math.dist and
the plain square root gives the other flag for a fifth of them.  Without a GPU: the file is what it says, and the host path
(world.run) gives the recorded flags.  On the device (DeviceWorld.run, vrt_physics_run): the same flags from a camera passed in,
from the camera the device derives from a followed body, and at a second tick."""
import math

import numpy as np
import pytest

import physics_flags_scene as fl
import physics_run_util as ru
import physics_scenes as ps
from python_raytracer_amd import _native as nat
from python_raytracer_amd import world
from python_raytracer_amd.lib import vec2, vec3

gpu = pytest.mark.gpu
FAR = (1e6, 1e6, 1e6)


def flags_scene(follower=False):
    """(the file's arrays, the objects, the settings store[, the followed body with its camera attached])."""
    z, pos = fl.load()
    objects, _, _, st = ps.project_scene(fl.spec_of(pos, follower))
    if not follower:
        return z, objects, st
    who = objects[-1]
    who.set_camera(vec2(0, fl.UP))
    assert who.cam_pos.tuple() == tuple(fl.CAM) and not who.sprite
    return z, objects, st, who


def assert_flags(row, z, what):
    n = len(z["pos"])
    assert np.array_equal(row["visible"][:n] != 0, z["visible"]), (what, np.flatnonzero((row["visible"][:n] != 0) != z["visible"]))
    assert np.array_equal(row["awake"][:n] != 0, z["awake"]), (what, np.flatnonzero((row["awake"][:n] != 0) != z["awake"]))
    assert np.array_equal(ru.bits(row["pos"][:n]), ru.bits(z["pos"])) and not row["moved"].any(), what


# ---- without a GPU -----------------------------------------------------------------------------------------------------------
def test_the_file_is_what_it_says():
    z, pos = fl.load()
    n = fl.N
    assert z["pos"].shape == (n, 3) and n > 1024 and z["cam"].tolist() == fl.CAM and (fl.CAM[1] - fl.UP) + fl.UP == fl.CAM[1]
    seen = set()
    for i, p in enumerate(pos):
        kind = fl.KINDS[i % 3]
        limit = float(fl.DIST_MAX + fl.HALF[kind]) if kind and (i // 9) % 2 else float(fl.DIST_MOVE)
        want = (limit, math.nextafter(limit, 0.0), math.nextafter(limit, math.inf))[(i // 3) % 3]
        assert math.dist(p, fl.CAM) == want, i                                  # (this interpreter's math.dist is the generating one's)
        assert bool(z["visible"][i]) == (bool(kind) and want <= fl.DIST_MAX + fl.HALF[kind]) and bool(z["awake"][i]) == (want <= fl.DIST_MOVE)
        dx, dy, dz = (a - b for a, b in zip(p, fl.CAM))
        plain = math.sqrt(dx * dx + dy * dy + dz * dz)
        other = (bool(kind) and plain <= fl.DIST_MAX + fl.HALF[kind], plain <= fl.DIST_MOVE) != (bool(z["visible"][i]), bool(z["awake"][i]))
        assert other == bool(z["naive"][i]), i
        seen.add((kind, (i // 3) % 3, limit, i >= 1024))
    assert len(seen) == 2 * 3 * (2 + 2 + 1)                                     # every kind, outcome and limit on both sides of 1024
    assert z["naive"].sum() * 10 >= n                                           # the share make_kat_dist.py demands
    for flag in ("visible", "awake"):
        assert 0 < z[flag][:1024].sum() < 1024 and 0 < z[flag][1024:].sum() < n - 1024
    # a distance computed as a plain `<` for `<=` fails at every body that stands on its limit
    on = np.array([(i // 3) % 3 == 0 for i in range(n)])
    assert (z["awake"] | z["visible"])[on].all() and on.sum() > n // 4


def test_host_run_gives_the_recorded_flags():
    z, objects, st = flags_scene()
    counters, trace = world.run(objects, vec3(*fl.CAM), st, 2, trace=True)
    for t in range(2):
        assert_flags(trace[t], z, ("host", t))
        assert (counters[t]["status"] == world.PHYSICS_SKIPPED).all()
    assert [bool(o.visible) for o in objects] == z["visible"].tolist()
    # followed: the camera is the body's cam_pos
    z, objects, st, who = flags_scene(follower=True)
    counters, trace = world.run(objects, vec3(*FAR), st, 1, follow=who, trace=True)
    assert_flags(trace[0], z, "host, followed")
    assert trace[0]["awake"][-1] and not trace[0]["visible"][-1]


# ---- on the device -----------------------------------------------------------------------------------------------------------
def assert_nothing_ran(r, n):
    assert int(r.stats[nat.S_PHYSICS_REFUSED]) == 0 and int(r.stats[nat.S_PHYSICS_BODIES]) == 0 and int(r.stats[nat.S_PHYSICS_STEPS]) == 0
    assert (r.trace["status"] == nat.BODY_SKIPPED).all() and r.moved == [] and r.trace.shape[1] == n
    assert not r.stats[:5].any() and r.stats[7] == 0


@gpu
def test_device_run_gives_the_recorded_flags():
    from python_raytracer_amd.world import DeviceWorld
    z, objects, st = flags_scene()
    r = DeviceWorld(8).run(objects, vec3(*fl.CAM), st, 1, trace=True)
    assert r.ticks_run == 1 and r.launches == 1
    assert_flags(r.trace[0], z, "device")
    assert_nothing_ran(r, fl.N)
    assert [bool(o.visible) for o in objects] == z["visible"].tolist()
    assert [bool(o.redraw) for o in objects if o.sprite] == [True] * sum(bool(o.sprite) for o in objects)   # (nothing cleared it)


@gpu
def test_device_run_gives_them_from_the_camera_it_follows():
    """The followed body stands at CAM - (0, UP, 0) and its attachment is (0, UP): pos + offset is CAM exactly.  pos_cam as passed
    is far away -- from there every body is asleep and out of sight, as the run without `follow` shows -- so the flags come from
    the camera the device worked out itself."""
    from python_raytracer_amd.world import DeviceWorld
    z, objects, st, who = flags_scene(follower=True)
    r = DeviceWorld(8).run(objects, vec3(*FAR), st, 1, follow=who, trace=True)
    assert_flags(r.trace[0], z, "device, followed")
    assert_nothing_ran(r, fl.N + 1)
    assert r.trace[0]["awake"][-1] and not r.trace[0]["visible"][-1]
    z, objects, st, who = flags_scene(follower=True)
    r = DeviceWorld(8).run(objects, vec3(*FAR), st, 1, trace=True)
    assert not r.trace[0]["awake"].any() and not r.trace[0]["visible"].any()


@gpu
def test_a_second_tick_leaves_every_flag_as_it_was():
    from python_raytracer_amd.world import DeviceWorld
    z, objects, st = flags_scene()
    ps.clear_redraw(objects)
    r = DeviceWorld(8).run(objects, vec3(*fl.CAM), st, 2, trace=True)
    assert r.ticks_run == 2
    for t in range(2):
        assert_flags(r.trace[t], z, ("device", t))
    assert_nothing_ran(r, fl.N)
    rec = r.records
    assert np.array_equal(rec["visible_before"], rec["visible_now"]) and np.array_equal(rec["visible_now"] != 0, z["visible"])
    # the "ever flipped" bit is the first tick's (every object came in with visible = False): the second tick set none
    assert np.array_equal(rec["pad"][:, 0], np.where(z["visible"], nat.BODY_EVER_FLIPPED, 0))
    assert [bool(o.redraw) for o in objects] == [bool(v) or not o.sprite for o, v in zip(objects, z["visible"])]
