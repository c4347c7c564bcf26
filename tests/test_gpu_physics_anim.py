"""Sprites animated during a device physics run (DeviceWorld.run(clock=), vrt_physics_run_anim): every tick of every scene of
tests/golden/physics_anim.npz, recorded from the real reference under a scripted clock, bit for bit -- positions, velocities,
boxes, visibility, weights and frames -- side by side with the host path (world.run(clock=)); one of the scenes under a camera
that follows a body; launches cut short by the work budget; the crowd, whose switching body and sharers lie on both sides of the
1024 bodies the device walks at a time; the run between the existing passes (run -> update -> first_hit, an edited frame); and
the C ABI itself with schedules, sprite indices and frame rows that are out of range."""
import ctypes as C

import numpy as np
import pytest

import physics_anim_scenes as an
import physics_run_util as ru
import physics_scenes as ps
from python_raytracer_amd import _native as nat
from python_raytracer_amd import make_settings, world
from python_raytracer_amd.lib import material, quaternion, rgb, vec3
from python_raytracer_amd.world import DeviceWorld

gpu = pytest.mark.gpu
WORDS = ("BODIES", "REFUSED", "STEPS", "BLOCKED", "CONTACTS", "TRANSFERS", "CAPPED")


def totals(stats):
    return {w: int(stats[getattr(nat, "S_PHYSICS_" + w)]) for w in WORDS}


def same_state(a, b):
    sa, sb = ps.state(a), ps.state(b)
    return all(sa[f].tobytes() == sb[f].tobytes() for f in sa)


# ---- 1. the recorded runs: `wake` follows a body, `crowd` has more bodies than the device walks at a time ------------------
@gpu
@pytest.mark.parametrize("name", list(an.SCENES))
def test_device_run_with_a_clock_is_the_references(name):
    z, spec, dev, sprites, st, who = an.fresh(name)
    _, _, host, host_sprites, _, who_host = an.fresh(name)
    assert (who is not None) == (name == "wake")
    cam, clock = vec3(*spec["cam"]), tuple(spec["clock"])
    r = DeviceWorld(8).run(dev, cam, st, spec["ticks"], follow=who, trace=True, clock=clock)
    assert r.ticks_run == spec["ticks"] and r.trace.shape == r.anim.shape == (spec["ticks"], len(dev))
    an.assert_ticks(z, name, spec, dev, sprites, r.trace, r.anim, name + " (device)")
    counters, trace, anim = world.run(host, cam, st, spec["ticks"], follow=who_host, trace=True, clock=clock)
    assert ru.same_records(r.trace, trace) and ru.same_records(r.anim, anim)                 # the counters of every tick included
    assert np.array_equal(r.counters, counters[-1])
    assert same_state(dev, host)                                                             # `redraw` included: a switch sets it
    assert [float(o.weight) for o in dev] == [float(o.weight) for o in host]
    assert r.frames == {sprites[s]: host_sprites[s].frame for s in sprites if sprites[s].animated} and len(r.frames) == 1
    switched = (anim["switched"] != 0).any(axis=0)
    assert np.array_equal((r.records["pad"][:, 0] & nat.BODY_EVER_SWITCHED) != 0, switched) and switched.any()
    assert int(r.stats[nat.S_PHYSICS_BODIES]) == int((counters["status"] == 0).sum()) and int(r.stats[nat.S_PHYSICS_REFUSED]) == 0
    if name == "crowd":
        R = an.CROWD_ROLES
        assert np.nonzero(switched)[0].tolist() == [R["switcher"]] and len(dev) > an.TILE
        assert (r.anim["frame"][:, [R["blink_low"], R["switcher"], R["blink_high"]]] == z["crowd/frame"][:, [1]]).all()


@gpu
def test_without_a_clock_the_run_is_what_it_was():
    z, spec, dev, sprites, st, who = an.fresh("platform")
    r = DeviceWorld(8).run(dev, vec3(*spec["cam"]), st, spec["ticks"], trace=True)
    assert r.frames is None and r.anim is None and all(s.frame == 0 for s in sprites.values())
    assert np.array_equal(ru.bits(r.trace["pos"]), ru.bits(z["platform/held_pos"]))
    assert np.array_equal(ru.bits(r.trace["vel"]), ru.bits(z["platform/held_vel"]))
    assert not (r.records["pad"][:, 0] & nat.BODY_EVER_SWITCHED).any()


@gpu
def test_a_run_with_a_clock_refuses_what_the_host_path_refuses():
    z, spec, dev, sprites, st, who = an.fresh("platform")
    before = ps.state(dev)
    sprites["plat"].anim_set(0, 2, 0.2)
    with pytest.raises(ValueError, match="frame_start"):
        DeviceWorld(8).run(dev, vec3(*spec["cam"]), st, 2, clock=(0, 50))
    sprites["plat"].anim_set(0, 1, 0.2)
    for clock in ((-1, 50), (0, 0.5), (1,)):
        with pytest.raises(ValueError, match="clock"):
            DeviceWorld(8).run(dev, vec3(*spec["cam"]), st, 2, clock=clock)
    after = ps.state(dev)
    assert all(before[f].tobytes() == after[f].tobytes() for f in before)


# ---- 2. the work budget ------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", ["platform", "weights"])
def test_launches_cut_short_by_the_budget_change_nothing(name):
    runs = []
    for budget in (None, 1, "part"):
        z, spec, objects, sprites, st, who = an.fresh(name)
        if budget == "part":
            budget = int(runs[0].stats[nat.S_PHYSICS_WORK]) // 3       # a launch ends about three times in the run
        r = DeviceWorld(8).run(objects, vec3(*spec["cam"]), st, spec["ticks"], trace=True, budget=budget, clock=tuple(spec["clock"]))
        assert r.ticks_run == spec["ticks"] == int(r.stats[nat.S_PHYSICS_TICKS])
        runs.append(r)
    whole, single, part = runs
    assert whole.launches == 1 and single.launches == spec["ticks"] and 1 < part.launches < spec["ticks"]
    for other in (single, part):
        assert ru.same_records(whole.records, other.records) and ru.same_records(whole.trace, other.trace)
        assert ru.same_records(whole.anim, other.anim) and np.array_equal(whole.stats, other.stats)
        assert list(whole.frames.values()) == list(other.frames.values())
    assert (whole.records["pad"][:, 0] & nat.BODY_EVER_SWITCHED).any() and (whole.anim["switched"] != 0).sum() >= 2


# ---- 3. between the existing passes ------------------------------------------------------------------------------------------
def _camera(st, scene, pos):
    from python_raytracer_amd import Camera
    cam = Camera(settings=st)
    cam.pos = vec3(*[float(v) for v in pos])
    cam.rot = quaternion(0.0, 0.0, 0.0, 1.0)
    cam.set_world_scene(scene)
    cam.chunk_update(None)
    return cam


PROPS = lambda i: dict(function=material, albedo=rgb(200, 100, 50), roughness=0.0, absorption=1.0, ior=0.0, energy=0.0)  # noqa: E731


@gpu
def test_run_update_first_hit_is_a_fresh_build():
    """The platform blinks during the run; update(objects) re-voxelises what shows the changed frame and what fell, and a 32 x 32
    first_hit over the updated world equals the one over a fresh DeviceWorld.build of the same objects."""
    import torch
    _, specs = an.load_fixture()
    spec = specs["platform"]
    dev, sprites, _, st, _ = an.project_scene(spec, PROPS)
    cam = vec3(*spec["cam"])
    dw = DeviceWorld(8)
    dw.run(dev, cam, st, 1, clock=(0, 0))                              # everything comes into view; the clock stands at frame 0
    scene, _ = dw.update(dev)
    assert sprites["plat"].frame == 0 and not any(o.redraw for o in dev)
    r = dw.run(dev, cam, st, 6, clock=(50, 50))                        # ticks 1..6 of the fixture's clock: the switch is at 200 ms
    assert r.frames == {sprites["plat"]: 1} and dev[1].redraw and dev[1] not in r.moved
    scene, rebuilt = dw.update(dev)
    assert rebuilt > 0 and not any(o.redraw for o in dev)
    rs = make_settings(width=32, height=32, samples=1, chunk_size=8, dist_max=96, chunk_lod=0, max_bounces=1.0)
    rs.culling = False
    pos = [0.0, 6.0, -24.0]
    fresh_world = DeviceWorld(8)
    a, b = _camera(rs, scene, pos), _camera(rs, fresh_world.build(dev), pos)
    ha, hb = a.first_hit(), b.first_hit()
    assert torch.equal(ha.records, hb.records)
    mats = ha.records.cpu().numpy().view(np.dtype(nat.HIT_FIELDS))["material"]
    assert (mats > 0).any() and (mats <= 0).any()                      # the frame that is left and the sky where the platform was
    # ... and the frame before the switch looked otherwise
    sprites["plat"].frame = 0
    c = _camera(rs, DeviceWorld(8).build(dev), pos)
    assert not torch.equal(c.first_hit().records, ha.records)


@gpu
def test_an_edited_frame_of_an_animated_sprite():
    """Frame 1 of the platform, resident since the first run but not shown, is filled in with Sprite.set_voxels_area; the next
    run replays the journal on the resident model and the cubes stay up when the platform blinks, as on the host."""
    _, specs = an.load_fixture()
    spec = specs["platform"]
    dev, dsprites, _, st, _ = an.project_scene(spec)
    host, hsprites, _, _, _ = an.project_scene(spec)
    cam = vec3(*spec["cam"])
    dw = DeviceWorld(8)
    r = dw.run(dev, cam, st, 3, clock=(0, 50))
    counters, _, _ = world.run(host, cam, st, 3, clock=(0, 50))
    assert np.array_equal(r.counters, counters[-1]) and same_state(dev, host) and dsprites["plat"].frame == 0
    z, _ = an.load_fixture()
    held = z["platform/held_pos"][7]                                   # where 8 ticks leave the bodies if the platform never blinks
    for sprites in (dsprites, hsprites):
        sprites["plat"].set_voxels_area(1, vec3(0, 0, 0), vec3(11, 1, 11), sprites["plat"].get_frame(0).get_voxel(vec3(0, 0, 0)), True)
    r = dw.run(dev, cam, st, 5, trace=True, clock=(150, 50))           # the switch comes at 200 ms
    counters, trace, anim = world.run(host, cam, st, 5, trace=True, clock=(150, 50))
    assert ru.same_records(r.trace, trace) and ru.same_records(r.anim, anim) and same_state(dev, host)
    assert dsprites["plat"].frame == 1 and (anim["switched"][:, 1] != 0).sum() == 1
    assert np.array_equal(ru.bits(ps.state(dev)["pos"]), ru.bits(held))                            # the filled frame holds them
    assert dw.model(dsprites["plat"], 1)[0].all() and dw.edit_calls["edit"] >= 1
    # the unedited scene lets them fall in those ticks
    plain, _, _, _, _ = an.project_scene(spec)
    DeviceWorld(8).run(plain, cam, st, 8, clock=(0, 50))
    assert plain[0].pos.y < held[0][1] and plain[2].pos.y < held[2][1]


# ---- 4. straight through the C ABI -------------------------------------------------------------------------------------------
class Abi:
    """The platform scene as DeviceWorld.run(clock=) packs it, for direct calls of vrt_physics_run and vrt_physics_run_anim."""

    def __init__(self):
        import torch
        self.torch = torch
        _, self.spec, self.objects, self.sprites, self.st, _ = an.fresh("platform")
        self.dw = DeviceWorld(8)
        plat = self.sprites["plat"]
        rows = {}
        flags = [(False, False, False)] * len(self.objects)
        self.bodies, remap, mats, matphys = self.dw._pack_bodies(self.objects, flags, [True] * len(self.objects), False, "test",
                                                                 [(plat, 0), (plat, 1)], rows)
        self.dw._flush_models()
        self.models = self.dw._model_dev
        dev = self.dw.device
        self.remap = torch.from_numpy(np.array(remap, np.uint8)).to(dev)
        self.matphys = torch.from_numpy(matphys.reshape(-1)).to(dev)
        self.n_materials = len(mats)
        self.ticks = self.spec["ticks"]
        self.body_sprite = np.array([-1, 0, -1], np.int32)
        self.sprite_tab = np.array([(0, 2, 0, 0)], np.dtype(nat.ANIM_SPRITE_FIELDS))
        self.frame_tab = np.array([rows[(id(plat), f)][:3] + (0, rows[(id(plat), f)][3]) for f in (0, 1)], np.dtype(nat.ANIM_FRAME_FIELDS))
        start, step = self.spec["clock"]
        self.schedule = np.array([[plat.frame_at(start + k * step)] for k in range(self.ticks)], np.int32)
        assert self.schedule.min() == 0 and self.schedule.max() == 1

    def call(self, anim=True, n_sprites=1, body_sprite=None, sprite_tab=None, frame_tab=None, schedule=None):
        """(status, bodies, trace, anim trace, stats, sprite table) after one launch of all ticks."""
        torch, dev = self.torch, self.dw.device
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)  # noqa: E731
        n = len(self.bodies)
        d_bodies = up(self.bodies)
        d_trace = torch.zeros(self.ticks * n * nat.BODY_SAMPLE_BYTES, dtype=torch.uint8, device=dev)
        d_anim = torch.zeros(self.ticks * n * nat.ANIM_SAMPLE_BYTES, dtype=torch.uint8, device=dev)
        stats = torch.zeros(nat.NSTATS, dtype=torch.int64, device=dev)
        st = self.st
        params = nat.VrtPhysicsParams(float(st.gravity), float(st.friction), float(st.friction_air), float(st.min_velocity), float(st.max_velocity))
        rp = nat.VrtPhysicsRunParams((C.c_double * 3)(*self.spec["cam"]), (C.c_double * 3)(0.0, 0.0, 0.0), float(st.dist_max), float(st.dist_move),
                                     1 << 40, self.ticks, -1)
        common = (d_bodies.data_ptr(), n, self.models.data_ptr(), self.models.numel(), self.remap.data_ptr(), self.remap.numel(),
                  self.matphys.data_ptr(), self.n_materials, C.byref(params), C.byref(rp), d_trace.data_ptr(), stats.data_ptr(),
                  torch.cuda.current_stream().cuda_stream)
        d_sprites = None
        if not anim:
            status = nat.lib().vrt_physics_run(*common)
        elif n_sprites == 0:
            status = nat.lib().vrt_physics_run_anim(*common, None, None, 0, None, 0, None, d_anim.data_ptr())
        else:
            d_body_sprite = up(self.body_sprite if body_sprite is None else body_sprite)
            d_sprites = up(self.sprite_tab if sprite_tab is None else sprite_tab)
            d_frames = up(self.frame_tab if frame_tab is None else frame_tab)
            d_schedule = up(self.schedule if schedule is None else schedule)
            status = nat.lib().vrt_physics_run_anim(*common, d_body_sprite.data_ptr(), d_sprites.data_ptr(), n_sprites, d_frames.data_ptr(),
                                                    len(self.frame_tab), d_schedule.data_ptr(), d_anim.data_ptr())
        torch.cuda.synchronize()
        return (status, d_bodies.cpu().numpy().view(np.dtype(nat.BODY_FIELDS)),
                d_trace.cpu().numpy().view(np.dtype(nat.BODY_SAMPLE_FIELDS)).reshape(self.ticks, n),
                d_anim.cpu().numpy().view(np.dtype(nat.ANIM_SAMPLE_FIELDS)).reshape(self.ticks, n), stats.cpu().numpy(),
                d_sprites.cpu().numpy().view(np.dtype(nat.ANIM_SPRITE_FIELDS)) if d_sprites is not None else None)


@gpu
def test_the_abi_ignores_what_is_out_of_range_and_refuses_a_frame_outside_the_models():
    abi = Abi()
    z, _ = an.load_fixture()
    status, plain_bodies, plain_trace, _, plain_stats, _ = abi.call(anim=False)
    assert status == 0 and np.array_equal(ru.bits(plain_trace["pos"]), ru.bits(z["platform/held_pos"]))
    # the tables as DeviceWorld.run packs them: the reference's run
    status, bodies, trace, anim, stats, left = abi.call()
    assert status == 0 and np.array_equal(ru.bits(trace["pos"]), ru.bits(z["platform/pos"])) and left["frame"].tolist() == [z["platform/frame"][-1, 0]]
    assert np.array_equal(anim["frame"][:, 1], z["platform/frame"][:, 0]) and (anim["frame"][:, [0, 2]] == -1).all()
    assert int(stats[nat.S_PHYSICS_WORK]) > int(plain_stats[nat.S_PHYSICS_WORK])             # a switch costs a unit

    def is_plain(result, frame=0):
        status, b, t, a, s, left = result
        assert status == 0 and b.tobytes() == plain_bodies.tobytes() and t.tobytes() == plain_trace.tobytes()
        assert np.array_equal(s, plain_stats) and not a["switched"].any()
        assert left is None or left["frame"].tolist() == [frame]

    # no sprites: vrt_physics_run's bytes
    is_plain(abi.call(n_sprites=0))
    # schedule values out of range change nothing: -1, below it, n_frames and beyond
    for bad in (-1, -7, 2, 1 << 30):
        is_plain(abi.call(schedule=np.where(abi.schedule == 1, bad, 0).astype(np.int32)))
    # a body's sprite index out of range: it shows no animated sprite
    for bad in (-1, -9, 1, 1 << 30):
        result = abi.call(body_sprite=np.array([-1, bad, -1], np.int32))
        is_plain(result)
        assert (result[3]["frame"] == -1).all()
    # a sprite whose rows leave the frame table is never switched
    for first_row, n_frames in ((1, 2), (-1, 2), (0, 3), (0, -1), (1 << 30, 2)):
        is_plain(abi.call(sprite_tab=np.array([(0, n_frames, first_row, 0)], np.dtype(nat.ANIM_SPRITE_FIELDS))))
    # a frame row whose model, rim or remap base leaves the buffers: the platform is refused from the tick of the switch on -- met
    # by nobody, so both cubes fall -- and, being the only body that shows the sprite, never switches back; the call returns,
    # nothing is read out of bounds
    first = int(np.nonzero(abi.schedule[:, 0] == 1)[0][0])
    assert 0 < first < abi.ticks - 2 and (abi.schedule[first:, 0] == 0).any()
    for field, value in (("model", abi.models.numel() - 1), ("model", -1), ("model", 1 << 40), ("rim", abi.models.numel()),
                         ("remap", abi.remap.numel() + 1), ("remap", -1)):
        table = abi.frame_tab.copy()
        table[1][field] = value
        status, b, t, a, s, left = abi.call(frame_tab=table)
        assert status == 0 and t[:first].tobytes() == trace[:first].tobytes(), (field, value)
        assert (t[first:, 1]["status"] == nat.BODY_REFUSED).all() and (t[:first, 1]["status"] != nat.BODY_REFUSED).all()
        assert int(s[nat.S_PHYSICS_REFUSED]) == abi.ticks - first                            # once per tick, the tick of the switch included
        assert a[first, 1]["switched"] == 1 and a["switched"].sum() == 1 and left["frame"].tolist() == [1]
        assert (t[first:, [0, 2]]["status"] == 0).all()
        assert all((np.diff(t[first:, k]["pos"][:, 1]) < 0).all() for k in (0, 2))           # nothing is under them any more
