"""Many physics ticks in one device call (DeviceWorld.run, vrt_physics_run): every recorded run of the real reference
(tests/golden/physics_*.npz) in segments between the scripts' ticks, every tick of the trace bit for bit, side by side with a
twin stepped by DeviceWorld.tick and one stepped by world.tick; the camera that follows a body (tests/golden/physics_follow.npz);
launches cut short by the work budget; bodies the device comes to refuse in the middle of a run; the run between the existing
passes (edit -> run -> update -> render, owners); fractional solidity; and a run of one tick against tick()."""
import json

import numpy as np
import pytest

import physics_follow_scenes as fs
import physics_run_util as ru
import physics_scenes as ps
from python_raytracer_amd import _native as nat
from python_raytracer_amd import make_settings, world
from python_raytracer_amd.lib import material, quaternion, rgb, vec2, vec3
from python_raytracer_amd.world import DeviceWorld, build_world

gpu = pytest.mark.gpu
WORDS = ("BODIES", "REFUSED", "STEPS", "BLOCKED", "CONTACTS", "TRANSFERS", "CAPPED")
COUNTERS = [f for f, _ in world.PHYSICS_COUNTER_FIELDS]


def totals(stats):
    return {w: int(stats[getattr(nat, "S_PHYSICS_" + w)]) for w in WORDS}


def same_state(a, b):
    sa, sb = ps.state(a), ps.state(b)
    return all(sa[f].tobytes() == sb[f].tobytes() for f in sa)


def assert_tick_is_trace_row(row, objects, counters, what):
    """One row of a run's trace against the objects a tick() loop has just stepped, and that tick's counters."""
    st = ps.state(objects)
    for f in ("pos", "vel"):
        assert np.array_equal(ru.bits(row[f]), ru.bits(st[f])), (what, f, row[f], st[f])
    assert np.array_equal(row["mins"], st["mins"]) and np.array_equal(row["maxs"], st["maxs"]), what
    assert np.array_equal(row["visible"] != 0, st["visible"]), what
    for f in COUNTERS:
        assert np.array_equal(row[f], counters[f]), (what, f, row[f], counters[f])


# ---- 1. the recorded runs ----------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", ps.DEVICE_SCENES)
def test_device_run_is_the_references(name):
    z, spec = ps.load_fixture(name)
    dev, _, _, st = ps.project_scene(spec)
    twin, _, _, _ = ps.project_scene(spec)
    host, _, _, _ = ps.project_scene(spec)
    has_sprite = np.array([bool(o.sprite) for o in dev])
    dw, dw_twin = DeviceWorld(16), DeviceWorld(16)
    cam = spec["cam"]
    for first, last in ru.segments(spec):
        for objects in (dev, twin, host):
            ps.clear_redraw(objects)
            at = ps.apply_script(spec, first, objects, vec3, cam)
        cam = at
        entry = ps.state(dev)
        r = dw.run(dev, vec3(*cam), st, last - first, trace=True)
        assert r.ticks_run == last - first and r.launches >= 1 and r.trace.shape == (last - first, len(dev))
        ru.assert_segment(z, first, r.trace, entry, has_sprite, name + " (run)")
        summed = dict.fromkeys(WORDS, 0)
        moved = np.zeros(len(dev), bool)
        for k in range(first, last):
            t = dw_twin.tick(twin, vec3(*cam), st)
            want = world.tick(host, vec3(*cam), st)
            assert np.array_equal(t.counters, want), (name, k)
            assert_tick_is_trace_row(r.trace[k - first], twin, want, (name, k))
            asleep = t.records["awake"] == 0
            assert np.array_equal(r.trace[k - first]["awake"] == 0, asleep), (name, k)
            for w, v in totals(t.stats).items():
                summed[w] += v
            moved |= want["moved"] != 0
        assert totals(r.stats) == summed, (name, first)
        assert int(r.stats[nat.S_PHYSICS_TICKS]) == last - first and int(r.stats[nat.S_PHYSICS_WORK]) >= (last - first) * len(dev)
        assert not r.stats[:5].any() and r.stats[7] == 0 and r.stats[15] == 0
        assert same_state(dev, twin) and same_state(dev, host), (name, first)       # redraw included: set where any tick would
        assert r.moved == [o for o, m in zip(dev, moved) if m]
        assert np.array_equal(r.counters, want)                                      # the records' `out` words are the last tick's


# ---- 2. the camera that follows ----------------------------------------------------------------------------------------------
def follow_scene():
    z = np.load(fs.PATH)
    spec = json.loads(bytes(z["spec"]).decode())
    objects, _, _, st = ps.project_scene(spec)
    who = fs.attach(objects, vec2)
    ps.clear_redraw(objects)
    return z, spec, objects, st, who


@gpu
def test_run_follows_the_body_that_carries_the_camera():
    z, spec, dev, st, who = follow_scene()
    _, _, host, _, who_host = follow_scene()
    has_sprite = np.array([bool(o.sprite) for o in dev])
    entry = ps.state(dev)
    far = vec3(1e6, 1e6, 1e6)                                  # not used: the followed body is never refused
    r = DeviceWorld(8).run(dev, far, st, spec["ticks"], follow=who, trace=True)
    ru.assert_segment(z, 0, r.trace, entry, has_sprite, "follow (run)")
    counters, trace = world.run(host, far, st, spec["ticks"], follow=who_host, trace=True)
    assert ru.same_records(r.trace, trace)
    assert same_state(dev, host) and np.array_equal(r.counters, counters[-1])
    assert np.array_equal(ru.bits(who.cam_pos.tuple()), ru.bits(z["cam_pos"][-1])) and who in r.moved
    assert r.ticks_run == spec["ticks"]
    # held where it started, the same scene ends elsewhere: the device's camera did move
    z, spec, dev, st, who = follow_scene()
    DeviceWorld(8).run(dev, who.cam_pos, st, spec["ticks"])
    assert np.array_equal(ru.bits(ps.state(dev)["pos"]), ru.bits(z["fixed_final_pos"]))
    # an attachment that is out of date is refused, not guessed at
    z, spec, dev, st, who = follow_scene()
    who.cam_pos = vec3(0, 0, 0)
    with pytest.raises(ValueError, match="set_camera_pos"):
        DeviceWorld(8).run(dev, far, st, 2, follow=who)
    with pytest.raises(ValueError, match="not one of"):
        DeviceWorld(8).run(dev[:2], far, st, 2, follow=who)


# ---- 3. the work budget ------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", ["default", "pile"])
def test_launches_cut_short_by_the_budget_change_nothing(name):
    _, spec = ps.load_fixture(name)
    ticks = spec["ticks"]
    runs = []
    for budget in (None, 1, "part"):
        objects, _, _, st = ps.project_scene(spec)
        if budget == "part":
            budget = int(runs[0].stats[nat.S_PHYSICS_WORK]) // 3       # a launch ends about three times in the run
        r = DeviceWorld(16).run(objects, vec3(*spec["cam"]), st, ticks, trace=True, budget=budget)
        assert r.ticks_run == ticks == int(r.stats[nat.S_PHYSICS_TICKS])
        runs.append(r)
    whole, single, part = runs
    assert single.launches == ticks and 1 < part.launches < ticks and whole.launches >= 1
    assert whole.launches == 1 or nat.PHYSICS_RUN_BUDGET < int(whole.stats[nat.S_PHYSICS_WORK])
    for other in (single, part):
        assert ru.same_records(whole.records, other.records) and ru.same_records(whole.trace, other.trace)
        assert np.array_equal(whole.stats, other.stats)
    assert (whole.records["pad"][:, 0] & nat.BODY_EVER_MOVED).any()


@gpu
def test_no_bodies_and_bad_arguments():
    st = make_settings(dist_move=24, dist_max=40)
    r = DeviceWorld(8).run([], vec3(0, 0, 0), st, 5, trace=True)
    assert r.ticks_run == 5 and r.launches == 1 and r.trace is None and r.moved == [] and not r.stats[7:].any()
    for kw in (dict(ticks=0), dict(ticks=3, budget=0)):
        with pytest.raises(ValueError):
            DeviceWorld(8).run([], vec3(0, 0, 0), st, **kw)


# ---- 4. refusal in the middle of a run ---------------------------------------------------------------------------------------
def _refusal_scene(kind):
    big = 10 ** 6
    if kind == "vel":
        # a 2^3 body of weight 0.5 under gravity 1200: -600 after one tick, -1200 after two -- beyond VRT_PHYSICS_MAX_VEL = 1024,
        # which max_velocity = 2048 lets through
        return 1, ps.scene({"tiny": ps.full((2, 2, 2)), "slab": ps.full((16, 2, 16)), "cube": ps.full((4, 4, 4), 3)},
                           [ps.obj("slab", (0, 0, 0), physics=False), ps.obj("tiny", (100, 0, 0)), ps.obj("cube", (0, 3, 0), vel=(0.5, 0, 0)),   # (the cube: weight 0.25)
                            ps.obj("cube", (40, 10, 0), vel=(0, 0, 0.25), physics=False)], 5,
                           gravity=1200.0, friction_air=0.0, min_velocity=0.0, max_velocity=2048.0, dist_move=big, dist_max=big)
    # a body that flies across |x| = 2^28 in its second tick
    edge = float(2 ** 28)
    return 1, ps.scene({"tiny": ps.full((2, 2, 2)), "slab": ps.full((16, 2, 16)), "cube": ps.full((4, 4, 4), 1)},
                       [ps.obj("slab", (edge - 40, 0, 0), physics=False), ps.obj("tiny", (edge - 3, 20, 0), vel=(2, 0, 0)),
                        ps.obj("cube", (edge - 40, 3, 0), vel=(0.5, 0, 0)), ps.obj("tiny", (edge - 20, 20, 0), physics=False)], 5,
                       cam=(edge, 0.0, 0.0), gravity=0.0, friction_air=0.0, min_velocity=0.0, max_velocity=2048.0, dist_move=big, dist_max=big)


@gpu
@pytest.mark.parametrize("kind", ["vel", "pos"])
def test_a_body_refused_in_the_middle_of_a_run(kind):
    """The run validates every body anew at every tick: the tick at which a fresh tick() refuses the body is the tick at which
    the run does -- status -3, position and velocity untouched from then on -- and the other bodies do what they do in the tick()
    loop."""
    bad, spec = _refusal_scene(kind)
    dev, _, _, st = ps.project_scene(spec)
    twin, _, _, _ = ps.project_scene(spec)
    cam = vec3(*spec["cam"])
    r = DeviceWorld(8).run(dev, cam, st, spec["ticks"], trace=True)
    dw = DeviceWorld(8)
    status, refused = [], 0
    for k in range(spec["ticks"]):
        t = dw.tick(twin, cam, st)
        assert_tick_is_trace_row(r.trace[k], twin, t.counters, (kind, k))
        status.append(int(t.counters[bad]["status"]))
        refused += int(t.stats[nat.S_PHYSICS_REFUSED])
    assert status == [0, 0, -3, -3, -3], status
    assert r.trace[:, bad]["status"].tolist() == status and int(r.stats[nat.S_PHYSICS_REFUSED]) == refused == 3
    for k in (2, 3, 4):
        assert ru.bits(r.trace[k, bad]["vel"]).tolist() == ru.bits(r.trace[1, bad]["vel"]).tolist()
        assert ru.bits(r.trace[k, bad]["pos"]).tolist() == ru.bits(r.trace[1, bad]["pos"]).tolist()
    if kind == "vel":
        assert r.trace[1, bad]["vel"][1] == -1200.0
    else:
        assert r.trace[1, bad]["pos"][0] >= 2.0 ** 28
    assert (r.trace[:, [0, 2, 3]]["status"] != nat.BODY_REFUSED).all() and (r.trace[:, 2]["status"] == 0).all()
    assert same_state(dev, twin)
    assert int(r.counters[bad]["status"]) == nat.BODY_REFUSED and dev[bad] in r.moved


@gpu
def test_a_followed_body_that_is_refused_hands_the_camera_back():
    """From the tick that refuses the followed body on, the camera is pos_cam as passed: here far away, so that everything falls
    asleep and out of sight at exactly that tick."""
    bad, spec = _refusal_scene("vel")
    spec["settings"].update(dist_move=200, dist_max=300)
    dev, _, _, st = ps.project_scene(spec)
    dev[bad].set_camera(vec2(0, 2))
    r = DeviceWorld(8).run(dev, vec3(1e5, 0, 0), st, spec["ticks"], follow=dev[bad], trace=True)
    assert r.trace[:, bad]["status"].tolist() == [0, 0, -3, -3, -3]
    assert (r.trace[:2, 2]["awake"] != 0).all() and (r.trace[:2, [0, 2, 3]]["visible"] != 0).all()
    assert not r.trace[2:]["awake"].any() and not r.trace[2:]["visible"].any()
    assert (r.trace[2:, 2]["status"] == nat.BODY_SKIPPED).all()
    assert all(o.redraw for o in dev if o.sprite) and not any(o.visible for o in dev)


# ---- 5. between the existing passes ------------------------------------------------------------------------------------------
def _camera(st, scene, pos):
    from python_raytracer_amd import Camera
    cam = Camera(settings=st)
    cam.pos = vec3(*[float(v) for v in pos])
    cam.rot = quaternion(0.0, 0.0, 0.0, 1.0)
    cam.set_world_scene(scene)
    cam.chunk_update(None)
    return cam


@gpu
def test_dig_run_update_render_and_owners():
    """A cube at rest on a slab; the slab under it is dug out with Sprite.set_voxels_area; run(ticks=8) lets it fall through
    without invalidate(); update(objects) voxelises the hole and the cube where it is now; the frame of a camera on the updated
    world equals the frame over a fresh build_world of the same objects, and owners() still resolves."""
    import torch
    spec = ps.scene({"cube": ps.full((4, 4, 4)), "slab": ps.full((16, 4, 16), 1), "floor": ps.full((16, 2, 16), 1)},
                    [ps.obj("floor", (0, -12, 0), physics=False), ps.obj("slab", (0, 0, 0), physics=False), ps.obj("cube", (0, 5, 0))], 0)
    props = lambda i: dict(function=material, albedo=rgb(200, 100, 50), roughness=0.0, absorption=1.0, ior=0.0, energy=0.0)  # noqa: E731
    dev, dsprites, _, st = ps.project_scene(spec, props)
    host, hsprites, _, _ = ps.project_scene(spec)
    dw = DeviceWorld(8)
    cam = vec3(0, 0, 0)
    r = dw.run(dev, cam, st, 12)
    counters, _ = world.run(host, cam, st, 12)
    rest = dev[2].pos.y
    assert np.array_equal(r.counters, counters[-1]) and r.counters[2]["blocked_steps"] == 1 and same_state(dev, host)
    scene, rebuilt = dw.update(dev)
    assert rebuilt > 0 and not any(o.redraw for o in dev)
    ps.clear_redraw(host)                                              # (what update() has just done for the device's objects)
    for sprites in (dsprites, hsprites):
        sprites["slab"].set_voxels_area(0, vec3(5, 0, 5), vec3(10, 3, 10), None, True)
    r = dw.run(dev, cam, st, 8)
    counters, _ = world.run(host, cam, st, 8)
    assert np.array_equal(r.counters, counters[-1]) and same_state(dev, host)
    assert dev[2].pos.y < rest - 4 and dev[2] in r.moved and dev[2].redraw and not dev[0].redraw
    assert not dw.model(dsprites["slab"])[0][5:11, :, 5:11].any()       # the journal was replayed on the resident model
    scene, rebuilt = dw.update(dev)
    assert rebuilt > 0 and not any(o.redraw for o in dw.order)
    rs = make_settings(width=64, height=48, samples=1, chunk_size=8, dist_max=96, chunk_lod=0, max_bounces=1.0)
    rs.culling = False
    pos = [0.0, 1.0, -24.0]
    a = _camera(rs, scene, pos)
    b = _camera(rs, build_world(list(dw.order), 8).packed(), pos)
    fa, fb = a.render(0), b.render(0)
    assert torch.equal(fa.rgba_f32, fb.rgba_f32) and float(fa.rgba_f32.abs().sum()) > 0
    own = dw.owners(a.first_hit(), a)
    assert int(own.stats[nat.S_OWNER_ORPHANS]) == 0 and int(own.stats[nat.S_OWNER_RESOLVED]) > 0


# ---- 6. what the run does not do, and the run of one tick --------------------------------------------------------------------
@gpu
def test_fractional_solidity_raises():
    _, spec = ps.load_fixture("fraction")
    objects, _, _, st = ps.project_scene(spec)
    before = ps.state(objects)
    with pytest.raises(ValueError, match="fractional solidity"):
        DeviceWorld(8).run(objects, vec3(*spec["cam"]), st, 4)
    after = ps.state(objects)
    assert all(np.array_equal(before[k], after[k]) for k in before)


@gpu
def test_a_run_of_one_tick_is_tick():
    _, spec = ps.load_fixture("pile")
    a, _, _, st = ps.project_scene(spec)
    b, _, _, _ = ps.project_scene(spec)
    dwa, dwb = DeviceWorld(16), DeviceWorld(16)
    cam = vec3(*spec["cam"])
    for k in range(6):
        r = dwa.run(a, cam, st, 1)
        t = dwb.tick(b, cam, st)
        assert r.launches == 1 and r.ticks_run == 1 and r.trace is None
        x, y = r.records.copy(), t.records.copy()
        x["pad"] = y["pad"] = 0                                 # (the run's "ever moved, ever flipped" bits)
        assert x.tobytes() == y.tobytes(), k                    # flags worked out on the device included
        assert np.array_equal(r.counters, t.counters) and totals(r.stats) == totals(t.stats)
        assert r.moved == [a[i] for i, o in enumerate(b) if o in t.moved] and same_state(a, b)
        assert np.array_equal(r.records["pad"][:, 0] & 1, t.records["moved"])
