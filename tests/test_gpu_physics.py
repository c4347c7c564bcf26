"""Object physics on the device (DeviceWorld.tick, vrt_physics_tick): every recorded run of the real reference
(tests/golden/physics_*.npz) tick by tick and bit for bit, side by side with the host path (world.tick) including the per-body
counts and the statistics; the tick between the existing passes (edit -> tick -> update -> render, owners); the kernel's model
lookup through all 64 quarter-turn triples against the host world; what the device refuses, and that it touches nothing else --
also in the second tile of 1024 bodies, and at each limit's own value (the recorded scene `crowd` has 1100 bodies)."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle_lib as ol
import physics_scenes as ps
from python_raytracer_amd import _native as nat
from python_raytracer_amd import Material, make_settings, world
from python_raytracer_amd.lib import material, quaternion, rgb, vec3
from python_raytracer_amd.world import DeviceWorld, Object, Sprite, build_world

gpu = pytest.mark.gpu
WORDS = ("BODIES", "REFUSED", "STEPS", "BLOCKED", "CONTACTS", "TRANSFERS", "CAPPED")


def run_both(name, extra=None, hook=None, chunk_size=16):
    """The fixture's scene twice -- DeviceWorld.tick on one set of objects, world.tick on a twin -- with both held to the
    record after every tick and to each other in the counts.  hook(k, dw, objects, st) runs after tick k."""
    z, spec = ps.load_fixture(name)
    dev, _, _, st = ps.project_scene(spec, extra)
    host, _, _, _ = ps.project_scene(spec, extra)
    dw = DeviceWorld(chunk_size)
    cam_d = cam_h = spec["cam"]
    for k in range(spec["ticks"]):
        ps.clear_redraw(dev), ps.clear_redraw(host)
        cam_d, cam_h = ps.apply_script(spec, k, dev, vec3, cam_d), ps.apply_script(spec, k, host, vec3, cam_h)
        r = dw.tick(dev, vec3(*cam_d), st)
        want = world.tick(host, vec3(*cam_h), st)
        ps.assert_tick(z, k, dev, name + " (device)")
        ps.assert_tick(z, k, host, name + " (host)")
        assert np.array_equal(r.counters, want), (name, k, r.counters, want)
        ran = want[want["status"] == 0]
        totals = dict(BODIES=len(ran), REFUSED=0, STEPS=ran["steps"].sum(), BLOCKED=ran["blocked_steps"].sum(),
                      CONTACTS=ran["contacts"].sum(), TRANSFERS=ran["transfers"].sum(), CAPPED=0)
        stats = r.stats
        assert {w: int(stats[getattr(nat, "S_PHYSICS_" + w)]) for w in WORDS} == {w: int(v) for w, v in totals.items()}, (name, k)
        assert not stats[:8].any() and stats[15] == 0
        assert r.moved == [o for o, m in zip(dev, want["moved"]) if m]
        if hook:
            hook(k, dw, dev, st)
    return z, spec


# ---- 1. the recorded runs ----------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", [n for n in ps.DEVICE_SCENES if n != "default"])
def test_device_tick_is_the_references(name):
    run_both(name)


def _render_props():
    sc = ol.default_scene()
    rows = dict(zip(list(sc.names), sc.materials))

    def extra(i):
        row = rows[list(ps.DEFAULT_MATS)[i]]
        return dict(function=material, albedo=rgb(*[int(v) for v in row[:3]]), roughness=row[3], absorption=row[4], ior=row[5], energy=row[6])
    return extra, sc


def _camera(st, scene, pos):
    from python_raytracer_amd import Camera
    cam = Camera(settings=st)
    cam.pos = vec3(*[float(v) for v in pos])
    cam.rot = quaternion(0.0, 0.0, 0.0, 1.0)
    cam.set_world_scene(scene)
    cam.chunk_update(None)
    return cam


# ---- 2. between the existing passes ------------------------------------------------------------------------------------------
@gpu
def test_default_mod_ticks_update_render_and_owners():
    """The default mod's 40 ticks against the record; after ticks 1, 5 and the last: update(objects), and the frame of a camera
    on the updated world equals the frame over a fresh build_world of the same objects; owners() still resolves."""
    import torch
    extra, sc = _render_props()
    seen = []

    def hook(k, dw, objects, st):
        if k not in (1, 5, 39):
            return
        rs = make_settings(width=64, height=48, samples=1, chunk_size=16, dist_max=192, chunk_lod=0, max_bounces=1.0)
        rs.culling = False
        scene, rebuilt = dw.update(objects)
        assert (rebuilt > 0 or k == 39) and not any(o.redraw for o in dw.order)    # (at rest since tick 9: nothing to rebuild)
        pos = [float(v) for v in sc.cam_pos]
        cam = _camera(rs, scene, pos)
        other = _camera(rs, build_world(list(dw.order), 16).packed(), pos)
        a, b = cam.render(0), other.render(0)
        assert torch.equal(a.rgba_f32, b.rgba_f32) and float(a.rgba_f32.abs().sum()) > 0
        hit = cam.first_hit()
        own = dw.owners(hit, cam)
        assert int(own.stats[nat.S_OWNER_ORPHANS]) == 0 and int(own.stats[nat.S_OWNER_RESOLVED]) > 0
        seen.append((k, tuple(o.pos.tuple() for o in objects)))

    run_both("default", extra=extra, hook=hook)
    assert [k for k, _ in seen] == [1, 5, 39] and seen[0][1] != seen[1][1] != seen[2][1]


@gpu
def test_digging_the_floor_away_lets_the_cube_fall():
    """A cube at rest on a slab; the slab under it is dug out with Sprite.set_voxels_area; the next tick it falls -- on the
    device as on the host, without invalidate() -- and update() afterwards voxelises the hole."""
    spec = ps.scene({"cube": ps.full((4, 4, 4)), "slab": ps.full((16, 4, 16), 1)},
                    [ps.obj("slab", (0, 0, 0), physics=False), ps.obj("cube", (0, 5, 0))], 0)
    dev, dsprites, _, st = ps.project_scene(spec, lambda i: dict(function=material, albedo=rgb(200, 100, 50), roughness=0.0,
                                                                  absorption=1.0, ior=0.0, energy=0.0))
    host, hsprites, _, _ = ps.project_scene(spec)
    dw = DeviceWorld(8)
    cam = vec3(0, 0, 0)
    for k in range(12):
        r = dw.tick(dev, cam, st)
        assert np.array_equal(r.counters, world.tick(host, cam, st))
    rest = dev[1].pos.y
    assert r.counters[1]["blocked_steps"] == 1 and not r.moved and rest == host[1].pos.y
    scene, _ = dw.update(dev)
    assert dw.model(dsprites["slab"])[0][6:10, :, 6:10].all()
    for sprites in (dsprites, hsprites):
        sprites["slab"].set_voxels_area(0, vec3(5, 0, 5), vec3(10, 3, 10), None, True)
    for k in range(3):
        r = dw.tick(dev, cam, st)
        assert np.array_equal(r.counters, world.tick(host, cam, st))
        assert ps.state(dev)["pos"].tobytes() == ps.state(host)["pos"].tobytes() and ps.state(dev)["vel"].tobytes() == ps.state(host)["vel"].tobytes()
    assert dev[1].pos.y < rest - 1 and dev[1] in r.moved and dev[1].redraw
    assert not dw.model(dsprites["slab"])[0][5:11, :, 5:11].any()       # the journal was replayed on the resident model
    _, rebuilt = dw.update(dev)                                            # ... and the world still learns of the hole
    assert rebuilt > 0
    assert int(np.count_nonzero(build_world(list(dw.order), 8).grid)) == int(np.count_nonzero(dw._voxels.cpu().numpy()))


@gpu
def test_voxels_at_the_rim_block_until_the_sprite_is_cleared():
    """Voxels at model x = size.x -- where the import's mirrored x puts a file's x = 0 column -- are outside the model the
    renderer reads and inside the box the physics tests: a body moving towards them is blocked on the device as on the host;
    after Sprite.clear, which removes them from the Frame, it passes, without invalidate()."""
    spec = ps.scene({"cube": ps.full((4, 4, 4)), "post": dict(size=[4, 4, 4], lod=0, boxes=[[[4, 0, 0], [4, 3, 3], 1], [[0, 0, 0], [0, 0, 0], 0]])},
                    [ps.obj("post", (0, 0, 0), physics=False), ps.obj("cube", (8, 0, 0), vel=(-1.5, 0, 0))], 0, gravity=0.0)
    dev, dsprites, _, st = ps.project_scene(spec)
    host, hsprites, _, _ = ps.project_scene(spec)
    assert not dsprites["post"].dense()[0][1:].any() and dsprites["post"].get_voxel(None, vec3(4, 1, 1), vec3(0, 0, 0)) is not None
    dw = DeviceWorld(8)
    cam = vec3(0, 0, 0)

    def ticks(n, push):
        blocked = 0
        for k in range(n):
            for objs in (dev, host):
                objs[1].vel = vec3(*push)
            r = dw.tick(dev, cam, st)
            assert np.array_equal(r.counters, world.tick(host, cam, st))
            assert ps.state(dev)["pos"].tobytes() == ps.state(host)["pos"].tobytes() and ps.state(dev)["vel"].tobytes() == ps.state(host)["vel"].tobytes()
            blocked += int(r.counters[1]["blocked_steps"])
        return blocked

    assert ticks(4, (-1.5, 0, 0)) == 2 and dev[1].mins.x == 3          # it stands against the plane at world x = -2 + 4
    for sprites in (dsprites, hsprites):
        sprites["post"].clear(0)
    assert ticks(3, (-1.5, 0, 0)) == 0 and dev[1].pos.x < 2


# ---- 3. the model lookup -----------------------------------------------------------------------------------------------------
@gpu
def test_lookup_through_every_quarter_turn_triple():
    """The 64 objects of tests/golden/world_random.npz -- every quarter-turn triple, turns the size rule ignores, sprites of lod
    1 -- each pushed one cell towards a solid probe block, in all six directions: the contacts the device counts are the
    voxels of the object's facing layer in the host world (build_world, which the suite holds to vrt_voxelize and to the
    reference), and equal the host path's."""
    z = np.load(os.path.join(ol.GOLDEN, "world_random.npz"))
    mat = Material(solidity=1, weight=2.0 ** -10, friction=0.5, elasticity=0.25, function=material, albedo=rgb(9, 9, 9), roughness=0.0,
                   absorption=1.0, ior=0.0, energy=0.0)
    num = lambda v: float(v) if v % 1 else int(v)  # noqa: E731
    sprites = []
    for k, (size, lod) in enumerate(zip(z["spec_size"], z["spec_lod"])):
        spr = Sprite(size=vec3(*[num(v) for v in size]), frames=1, lod=int(lod))
        rows = z["vox"][int(z["vox_start"][k]):int(z["vox_start"][k + 1])]
        spr.get_frame(0).set_voxels({(int(x), int(y), int(c)): mat for x, y, c, m in rows}, True)
        sprites.append(spr)
    probe = Sprite(size=vec3(16, 16, 16), frames=1, lod=0)
    probe.get_frame(0).set_voxels({(x, y, c): mat for x in range(16) for y in range(16) for c in range(16)}, True)
    st = make_settings(gravity=0.0, friction=1.0, friction_air=0.0, min_velocity=0.0, max_velocity=8.0, dist_move=10 ** 6, dist_max=10 ** 6)
    dw = DeviceWorld(8)
    cam = vec3(0, 0, 0)
    layers = 0
    for axis in range(3):
        for sign in (-1, 1):
            objects, expect = [], []
            for i, spr in enumerate(sprites):
                base = [40 * i, 0, 0]
                vel = [0.0, 0.0, 0.0]
                vel[axis] = float(sign)
                ob = Object(pos=vec3(*base), rot=vec3(*[num(v) for v in z["spec_rot"][i]]), sprite=spr, vel=vec3(*vel), physics=True)
                half = [int(ob.size.x), int(ob.size.y), int(ob.size.z)]
                at = list(base)
                at[axis] += sign * (half[axis] + 8)
                objects.append(ob)
                ob.visible = True
                grid = build_world([ob], 8)
                lo = np.array([ob.mins.x, ob.mins.y, ob.mins.z]) - grid.origin
                hi = np.array([ob.maxs.x, ob.maxs.y, ob.maxs.z]) - grid.origin
                box = grid.grid[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]]
                expect.append(int(np.count_nonzero(np.take(box, 0 if sign < 0 else box.shape[axis] - 1, axis=axis))))
                objects.append(Object(pos=vec3(*at), rot=vec3(0, 0, 0), sprite=probe, physics=False))
                objects[-1].visible = True       # (it comes after its object in the order: last tick's flag is what counts)
            twins = [Object(pos=vec3(*o.pos.tuple()), rot=o.rot, sprite=o.sprite, vel=vec3(*o.vel.tuple()), physics=o.physics) for o in objects]
            for t in twins:
                t.visible = True
            r = dw.tick(objects, cam, st)
            want = world.tick(twins, cam, st)
            assert np.array_equal(r.counters, want), (axis, sign)
            got = r.counters[0::2]
            assert got["contacts"].tolist() == expect, (axis, sign, got["contacts"].tolist(), expect)
            assert (got["steps"] == 1).all() and (got["blocked_steps"] == (np.array(expect) > 0)).all()
            assert (r.counters[1::2]["status"] == nat.BODY_SKIPPED).all()
            layers += sum(e > 0 for e in expect)
    assert layers >= 300          # nearly every object shows a voxel on every side


# ---- 4. bounds and refusals --------------------------------------------------------------------------------------------------
def _raw_tick(bodies, models, remap, matphys, n_materials, params=(0.0, 1.0, 0.0, 0.0, 8.0)):
    """vrt_physics_tick on hand-made records: (records after the call, the statistics)."""
    import torch
    dev = torch.device("cuda", torch.cuda.current_device())
    d_b = torch.from_numpy(bodies.view(np.uint8).reshape(-1).copy()).to(dev) if len(bodies) else torch.zeros(8, dtype=torch.uint8, device=dev)
    d_m, d_r = torch.from_numpy(models).to(dev), torch.from_numpy(remap).to(dev)
    d_p = torch.from_numpy(np.ascontiguousarray(matphys, np.float64).reshape(-1)).to(dev)
    stats = torch.full((nat.NSTATS,), 77, dtype=torch.int64, device=dev)
    p = nat.VrtPhysicsParams(*params)
    rc = nat.lib().vrt_physics_tick(d_b.data_ptr() if len(bodies) else None, len(bodies), d_m.data_ptr(), d_m.numel(), d_r.data_ptr(), d_r.numel(),
                                    d_p.data_ptr(), n_materials, C.byref(p), stats.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    out = d_b.cpu().numpy()[: len(bodies) * nat.BODY_BYTES].view(np.dtype(nat.BODY_FIELDS)) if len(bodies) else bodies
    return out, stats.cpu().numpy()


def _body(pos, half, size, model, vel=(0, 0, 0), physics=1):
    """A vrt_body record by hand: visible, awake, with a sprite, its box as Object.move leaves it."""
    b = np.zeros((), np.dtype(nat.BODY_FIELDS))
    b["pos"], b["vel"], b["weight"], b["half"] = pos, vel, 0.5, half
    b["object"]["mins"] = [int(np.ceil(p)) - h for p, h in zip(pos, half)]
    b["object"]["maxs"] = [int(np.floor(p)) + h for p, h in zip(pos, half)]
    b["object"]["size"], b["object"]["model"], b["object"]["remap"] = size, model, 0
    b["visible_before"] = b["visible_now"] = b["awake"] = b["has_sprite"] = 1
    b["physics"], b["rim"] = physics, -1
    return b


def _hand_scene():
    """A 8 x 2 x 8 slab at the origin, a 2^3 cube one cell above it moving down, another flying free: the records, by hand."""
    models = np.ones(8 * 2 * 8 + 8, np.uint8)
    remap = np.array([0, 1], np.uint8)
    matphys = np.array([[0, 0, 0, 0], [1, 0.5, 0.25, 0]], np.float64)
    body = _body
    slab = body((0, 0, 0), (4, 1, 4), (8, 2, 8), 0, physics=0)
    cube = body((0, 3, 0), (1, 1, 1), (2, 2, 2), 128, vel=(0, -1.5, 0))
    free = body((20, 0.5, 0), (1, 1, 1), (2, 2, 2), 128, vel=(0.75, 0, 0.75))
    return models, remap, matphys, slab, cube, free


@gpu
def test_no_body_and_one_body():
    models, remap, matphys, slab, cube, free = _hand_scene()
    out, stats = _raw_tick(np.zeros(0, np.dtype(nat.BODY_FIELDS)), models, remap, matphys, 1)
    assert not stats.any()                                   # n = 0 only zeroes the statistics
    out, stats = _raw_tick(np.array([free]), models, remap, matphys, 1)
    assert out[0]["status"] == 0 and out[0]["steps"] == 1 and out[0]["moved"] == 1 and out[0]["pos"].tolist() == [20.75, 0.5, 0.75]
    assert out[0]["object"]["mins"].tolist() == [20, 0, 0] and out[0]["object"]["maxs"].tolist() == [21, 1, 1]
    assert out[0]["vel"].tolist() == [0.75, 0.0, 0.75] and stats[nat.S_PHYSICS_BODIES] == 1 and stats[nat.S_PHYSICS_STEPS] == 1


@gpu
def test_refused_bodies_are_counted_and_untouched_and_their_neighbours_unaffected():
    models, remap, matphys, slab, cube, free = _hand_scene()
    clean, clean_stats = _raw_tick(np.array([slab, cube, free]), models, remap, matphys, 1)
    # the cube moves one cell down, then the slab blocks it: 2 x 2 voxels meet
    assert clean[1]["steps"] == 2 and clean[1]["blocked_steps"] == 1 and clean[1]["contacts"] == 4 and clean[1]["pos"].tolist() == [0, 2, 0]
    assert clean[0]["status"] == nat.BODY_SKIPPED and clean_stats[nat.S_PHYSICS_CONTACTS] == 4

    def bad(**change):
        # each stands where the cube is going and would block it, were it met
        b = cube.copy()
        b["pos"], b["vel"], b["physics"] = (0, 2, 0), (0, 0, 0), 1
        b["object"]["mins"], b["object"]["maxs"] = [-1, 1, -1], [1, 3, 1]
        for k, v in change.items():
            if k in ("model", "size"):
                b["object"][k] = v
            else:
                b[k] = v
        return b

    bads = [bad(pos=(float("nan"), 2, 0)), bad(vel=(0, float("inf"), 0)), bad(pos=(float(2 ** 28), 2, 0)), bad(vel=(0, 0, -2000.0)),
            bad(model=len(models) - 7), bad(model=-1), bad(half=(1, -1, 1)), bad(size=(2, 2, 1 << 20)), bad(rim=len(models) - 3),
            bad(pos=(0, float("-inf"), 0)), bad(weight=float("nan"))]
    mixed = np.array([bads[0], slab, bads[1], bads[2], cube, bads[3], bads[4], bads[5], free] + bads[6:])
    out, stats = _raw_tick(mixed, models, remap, matphys, 1)
    valid = [1, 4, 8]
    for k in range(len(mixed)):
        if k in valid:
            continue
        assert out[k]["status"] == nat.BODY_REFUSED, k
        a, b = out[k].copy(), mixed[k].copy()
        for f in ("steps", "blocked_steps", "contacts", "transfers", "moved", "status"):
            a[f] = b[f] = 0
        assert a.tobytes() == b.tobytes(), k              # but for the `out` words not a byte of a refused body changed
        assert not (out[k]["steps"] or out[k]["moved"] or out[k]["transfers"])
    assert out[valid].tobytes() == clean.tobytes()        # the neighbours did what they do without them
    assert stats[nat.S_PHYSICS_REFUSED] == len(bads) and stats[nat.S_PHYSICS_BODIES] == 2 and stats[nat.S_PHYSICS_CAPPED] == 0
    assert np.array_equal(np.delete(stats, nat.S_PHYSICS_REFUSED), np.delete(clean_stats, nat.S_PHYSICS_REFUSED))


@gpu
def test_refused_bodies_in_the_second_tile_of_the_walk():
    """1030 records: the validation loop and the walk over the other bodies both take a second trip of 1024.  Refused bodies
    at 1023, 1024 and 1029 (the last) stand where the cube at 1026 is going: they are untouched, counted and met by none, and the
    valid bodies do exactly what they do in the same array without them."""
    models, remap, matphys, slab, cube, free = _hand_scene()
    n = 1030
    far = [_body((1000 + 10 * i, 0, 0), (1, 1, 1), (2, 2, 2), 128, physics=0) for i in range(n)]
    blocker = cube.copy()
    blocker["pos"], blocker["vel"] = (0, 2, 0), (0, 0, 0)
    blocker["object"]["mins"], blocker["object"]["maxs"] = [-1, 1, -1], [1, 3, 1]
    bads = {1023: blocker.copy(), 1024: blocker.copy(), n - 1: blocker.copy()}
    bads[1023]["pos"][0] = float("nan")
    bads[1024]["vel"][2] = -2000.0
    bads[n - 1]["object"]["model"] = -1
    mixed = np.array(far)
    mixed[0], mixed[2], mixed[1026] = slab, free, cube
    for k, b in bads.items():
        mixed[k] = b
    valid = np.array([k for k in range(n) if k not in bads])
    clean, clean_stats = _raw_tick(mixed[valid], models, remap, matphys, 1)
    at = int(np.flatnonzero(valid == 1026)[0])
    assert clean[at]["steps"] == 2 and clean[at]["blocked_steps"] == 1 and clean[at]["contacts"] == 4 and clean[at]["pos"].tolist() == [0, 2, 0]
    assert clean_stats[nat.S_PHYSICS_BODIES] == 2 and clean_stats[nat.S_PHYSICS_REFUSED] == 0 and (clean["status"] != nat.BODY_REFUSED).all()
    out, stats = _raw_tick(mixed, models, remap, matphys, 1)
    for k in bads:
        assert out[k]["status"] == nat.BODY_REFUSED, k
        a, b = out[k].copy(), mixed[k].copy()
        for f in ("steps", "blocked_steps", "contacts", "transfers", "moved", "status"):
            assert f == "status" or out[k][f] == 0, (k, f)
            a[f] = b[f] = 0
        assert a.tobytes() == b.tobytes(), k              # but for the `out` words not a byte of a refused body changed
    assert out[valid].tobytes() == clean.tobytes()
    assert stats[nat.S_PHYSICS_REFUSED] == 3 and stats[nat.S_PHYSICS_CAPPED] == 0
    assert np.array_equal(np.delete(stats, nat.S_PHYSICS_REFUSED), np.delete(clean_stats, nat.S_PHYSICS_REFUSED))
    # were the blocker met it would stop the cube a step early: the same record, valid, at 1024
    mixed[1024] = blocker
    met, _ = _raw_tick(mixed, models, remap, matphys, 1)
    assert met[1024]["status"] == nat.BODY_OK and met[1026]["pos"].tolist() == [0, 3, 0] and met[1026]["blocked_steps"] == 1


def _header_define(name):
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    return int(re.search(r"^#define %s (\d+)\b" % name, open(os.path.join(root, "include", "vrt.h")).read(), re.M).group(1))


@gpu
def test_limits_accept_the_value_and_refuse_the_next():
    """include/vrt.h's refusal limits, each at its value (accepted: skipped, as these bodies are not physical) and just beyond it
    (refused): |vel| <= 1024, half <= 1024 with thin models of 2048 voxels along x and along y, a box extent <= 2049,
    |pos| < 2^28."""
    max_vel, max_half = _header_define("VRT_PHYSICS_MAX_VEL"), _header_define("VRT_PHYSICS_MAX_HALF")
    assert (max_vel, max_half) == (1024, 1024)
    models = np.ones(2 * max_half * 2 * 2, np.uint8)
    remap = np.array([0, 1], np.uint8)
    matphys = np.array([[0, 0, 0, 0], [1, 0.5, 0.25, 0]], np.float64)
    cases = []                                                      # (what, the record at the limit, the record beyond it)

    def pair(what, x, change_at, change_beyond, half=(1, 1, 1), size=(2, 2, 2)):
        a, b = (_body((x, 0, 0), half, size, 0, physics=0) for _ in range(2))
        change_at(a), change_beyond(b)
        cases.append((what, a, b))

    def setter(field, value, sub=None):
        def apply(b):
            (b["object"] if sub else b)[field] = value
        return apply

    for sign in (1.0, -1.0):
        pair("vel %+d" % sign, 0, setter("vel", (0, sign * max_vel, 0)), setter("vel", (0, sign * np.nextafter(float(max_vel), np.inf), 0)))
        pair("pos %+d" % sign, 10000, setter("pos", (sign * np.nextafter(2.0 ** 28, 0), 0, 0)), setter("pos", (sign * 2.0 ** 28, 0, 0)))
    thin_x, thin_y = (max_half, 1, 1), (1, max_half, 1)
    pair("half x", 20000, lambda b: None, setter("half", (max_half + 1, 1, 1)), half=thin_x, size=(2 * max_half, 2, 2))
    pair("half y", 30000, lambda b: None, setter("half", (1, max_half + 1, 1)), half=thin_y, size=(2, 2 * max_half, 2))
    pair("extent", 40000, setter("maxs", (40000 + max_half + 1, 1, 1), True), setter("maxs", (40000 + max_half + 2, 1, 1), True),
         half=thin_x, size=(2 * max_half, 2, 2))
    at_limit = np.array([a for _, a, _ in cases])
    beyond = np.array([b for _, _, b in cases])
    ext = at_limit["object"]["maxs"] - at_limit["object"]["mins"]
    assert ext[4:6].max() == 2 * max_half and ext[6, 0] == 2 * max_half + 1
    assert (beyond["object"]["maxs"] - beyond["object"]["mins"])[6, 0] == 2 * max_half + 2
    both = np.concatenate([at_limit, beyond])
    out, stats = _raw_tick(both, models, remap, matphys, 1)
    for k, (what, _, _) in enumerate(cases):
        assert out[k]["status"] == nat.BODY_SKIPPED, what
        assert out[len(cases) + k]["status"] == nat.BODY_REFUSED, what
    assert stats[nat.S_PHYSICS_REFUSED] == len(cases) and stats[nat.S_PHYSICS_BODIES] == 0
    for f in ("pos", "vel", "half", "object"):
        assert out[f].tobytes() == both[f].tobytes(), f


@gpu
def test_a_body_at_the_velocity_limit_takes_its_full_step_loop():
    """|vel| = max_velocity = 1024 = VRT_PHYSICS_MAX_VEL: accepted; the body takes more than 1000 unit steps in one tick, far below
    VRT_PHYSICS_STEP_CAP (3078, which accepted input cannot reach: 1024 steps of at most one unit each), and ends blocked on a
    wall -- on the device as on the host, in position, velocity, counts and CAPPED = 0."""
    spec = ps.scene({"cube": ps.full((2, 2, 2)), "wall": ps.full((2, 8, 8), 1)},
                    [ps.obj("wall", (1010, 0, 0), physics=False), ps.obj("cube", (0, 0, 0), vel=(1024.0, 0, 0))], 0,
                    gravity=0.0, friction_air=0.0, min_velocity=0.0, max_velocity=1024.0, dist_move=10 ** 6, dist_max=10 ** 6)
    dev, _, _, st = ps.project_scene(spec)
    host, _, _, _ = ps.project_scene(spec)
    dw = DeviceWorld(8)
    cam = vec3(0, 0, 0)
    for k in range(2):
        r = dw.tick(dev, cam, st)
        want = world.tick(host, cam, st)
        assert np.array_equal(r.counters, want), (k, r.counters, want)
        assert ps.state(dev)["pos"].tobytes() == ps.state(host)["pos"].tobytes() and ps.state(dev)["vel"].tobytes() == ps.state(host)["vel"].tobytes()
        assert int(r.stats[nat.S_PHYSICS_CAPPED]) == 0 and int(r.stats[nat.S_PHYSICS_REFUSED]) == 0
        if k == 0:
            # (the cube's leading layer, at model x = 1, meets the wall's first layer at world x = 1009 from pos.x = 1008)
            assert 1000 < want[1]["steps"] < nat.PHYSICS_STEP_CAP // 2 and want[1]["blocked_steps"] == 1 and want[1]["contacts"] == 4
            assert int(r.stats[nat.S_PHYSICS_STEPS]) == want[1]["steps"] and dev[1].pos.x == host[1].pos.x == 1008.0 and dev[1] in r.moved


@gpu
def test_fractional_solidity_is_the_host_paths():
    _, spec = ps.load_fixture("fraction")
    objects, _, _, st = ps.project_scene(spec)
    before = ps.state(objects)
    with pytest.raises(ValueError, match="world.tick"):
        DeviceWorld(8).tick(objects, vec3(*spec["cam"]), st)
    after = ps.state(objects)
    assert all(np.array_equal(before[k], after[k]) for k in before)


@gpu
def test_bad_host_arguments_are_refused_before_any_launch():
    import torch
    L = nat.lib()
    buf = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    stats = torch.full((nat.NSTATS,), 5, dtype=torch.int64, device="cuda")
    p = nat.VrtPhysicsParams(1.0, 1.0, 0.1, 0.01, 10.0)
    ptr = buf.data_ptr()

    def call(bodies=ptr, n=2, models=ptr, nbytes=64, remap=ptr, rbytes=8, mp=ptr, nm=1, params=p, st=stats.data_ptr()):
        return L.vrt_physics_tick(bodies, n, models, nbytes, remap, rbytes, mp, nm, C.byref(params) if params is not None else None, st, None)

    bad = nat.VrtPhysicsParams(1.0, float("nan"), 0.1, 0.01, 10.0)
    for kw in (dict(st=None), dict(params=None), dict(n=-1), dict(bodies=None), dict(bodies=ptr + 4), dict(mp=None), dict(models=None),
               dict(remap=None), dict(nbytes=-1), dict(nm=256), dict(params=bad)):
        assert call(**kw) == -1, kw
    torch.cuda.synchronize()
    assert (stats.cpu().numpy() == 5).all() and not buf.cpu().numpy().any()      # nothing ran
