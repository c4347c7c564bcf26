"""Many what-if runs in one device call (DeviceWorld.run_many, vrt_physics_run_batch): every recorded scene as a batch of the
world as it stands and five altered variants, each variant byte for byte DeviceWorld.run on a hand-made twin and world.run on a host
twin; the camera that follows; launches cut short by the budget where the runs' work differs widely; more runs than workgroups are
resident at once; a variant the device refuses next to ones it does not; a batch of one against run(); the caller's objects left
alone until apply(); the entry point through ctypes; fractional solidity."""
import ctypes as C
import json

import numpy as np
import pytest

import physics_batch_util as bu
import physics_follow_scenes as fs
import physics_run_util as ru
import physics_scenes as ps
from python_raytracer_amd import _native as nat
from python_raytracer_amd import world
from python_raytracer_amd.lib import material, rgb, vec2, vec3
from python_raytracer_amd.world import DeviceWorld

gpu = pytest.mark.gpu
WORDS = ("BODIES", "REFUSED", "STEPS", "BLOCKED", "CONTACTS", "TRANSFERS", "CAPPED", "TICKS")


def totals(stats):
    return {w: int(stats[getattr(nat, "S_PHYSICS_" + w)]) for w in WORDS}


def same_state(a, b):
    sa, sb = ps.state(a), ps.state(b)
    return all(sa[f].tobytes() == sb[f].tobytes() for f in sa)


def unchanged(before, objects):
    after = ps.state(objects)
    return all(before[f].tobytes() == after[f].tobytes() for f in before)


def tiny():
    """Scene `tiny` (2 bodies, 10 ticks), its settings and camera, and eight distinct variants of it."""
    _, spec = ps.load_fixture("edges_tiny")
    objects, _, _, st = ps.project_scene(spec)
    ps.clear_redraw(objects)
    eight = [{}, {1: dict(vel=(0.5, 0, 0))}, {1: dict(vel=(0, -3.25, 0.5))}, {1: dict(pos=(3, 7.5, -2))}, {1: dict(pos=(40, 5, 0))},
             {1: dict(pos=(-1, 9, 1), vel=(0.25, 1, 0))}, {0: dict(pos=(0, -2, 0))}, {0: dict(pos=(1, 0, 0)), 1: dict(vel=(-2, 0, 0))}]
    return spec, objects, st, vec3(*spec["cam"]), eight


# ---- 1. the recorded runs ----------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", ps.DEVICE_SCENES)
def test_every_variant_is_the_run_of_its_twin(name):
    z, spec = ps.load_fixture(name)
    objects, _, _, st = ps.project_scene(spec)
    has_sprite = np.array([bool(o.sprite) for o in objects])
    first, last = ru.segments(spec)[0]
    ps.clear_redraw(objects)
    cam = vec3(*ps.apply_script(spec, first, objects, vec3, spec["cam"]))
    entry = ps.state(objects)
    changes = bu.changes(objects, cam.tuple())
    assert len(changes) == 6 and changes[0] == {}
    r = DeviceWorld(16).run_many(objects, cam, st, last, [bu.mapping(objects, c) for c in changes], trace=True)
    assert unchanged(entry, objects)                                                  # nothing is written until apply()
    assert r.records.shape == (6, len(objects)) and r.trace.shape == (6, last, len(objects)) and r.stats.shape == (6, nat.NSTATS)
    assert r.ticks_run.tolist() == [last] * 6 and r.launches >= 1 and len(r.records) == 6
    ru.assert_segment(z, first, r.trace[0], entry, has_sprite, name + " (run_many, {})")
    dw = DeviceWorld(16)
    finals = set()
    for k, change in enumerate(changes):
        twin, host = bu.altered(objects, change), bu.altered(objects, change)
        t = dw.run(twin, cam, st, last, trace=True)
        counters, states = world.run(host, cam, st, last, trace=True)
        assert ru.same_records(r.records[k], t.records), (name, k)
        assert ru.same_records(r.trace[k], t.trace) and ru.same_records(r.trace[k], states), (name, k)
        assert np.array_equal(r.counters[k], counters[-1]) and np.array_equal(r.stats[k], t.stats), (name, k, r.stats[k], t.stats)
        pos, vel = r.final(k)
        assert np.array_equal(ru.bits(pos), ru.bits(states[-1]["pos"])) and np.array_equal(ru.bits(vel), ru.bits(states[-1]["vel"]))
        finals.add(r.trace[k].tobytes())
    assert len(finals) == 6, name                                                     # six different futures
    assert unchanged(entry, objects)


# ---- 2. the camera that follows ----------------------------------------------------------------------------------------------
@gpu
def test_every_variant_follows_its_own_copy_of_the_body():
    z = np.load(fs.PATH)
    spec = json.loads(bytes(z["spec"]).decode())
    objects, _, _, st = ps.project_scene(spec)
    who = fs.attach(objects, vec2)
    ps.clear_redraw(objects)
    entry = ps.state(objects)
    has_sprite = np.array([bool(o.sprite) for o in objects])
    far = vec3(1e6, 1e6, 1e6)                                  # not used: the followed body is never refused
    changes = [{}, {fs.FOLLOW: dict(vel=(0, 0, 1.5))}, {fs.FOLLOW: dict(pos=(40, 40, 0))}]
    r = DeviceWorld(8).run_many(objects, far, st, spec["ticks"], [bu.mapping(objects, c) for c in changes], follow=who, trace=True)
    ru.assert_segment(z, 0, r.trace[0], entry, has_sprite, "follow (run_many)")
    dw = DeviceWorld(8)
    for k, change in enumerate(changes):
        twin = bu.altered(objects, change)
        t = dw.run(twin, far, st, spec["ticks"], follow=twin[fs.FOLLOW], trace=True)
        assert ru.same_records(r.records[k], t.records) and ru.same_records(r.trace[k], t.trace), k
        mine = bu.twins(objects)
        r.apply(k, mine)
        assert same_state(mine, twin) and np.array_equal(ru.bits(mine[fs.FOLLOW].cam_pos.tuple()), ru.bits(twin[fs.FOLLOW].cam_pos.tuple()))
        if k == 0:
            assert np.array_equal(ru.bits(mine[fs.FOLLOW].cam_pos.tuple()), ru.bits(z["cam_pos"][-1]))
    # carried out of dist_move of the ball, the camera never wakes it
    assert r.trace[0][:, 1]["awake"].any() and not r.trace[2][:, 1]["awake"].any()
    assert unchanged(entry, objects) and np.array_equal(ru.bits(who.cam_pos.tuple()), ru.bits(z["cam_start"]))
    with pytest.raises(ValueError, match="not one of"):
        DeviceWorld(8).run_many(objects[:2], far, st, 2, [{}], follow=who)


# ---- 3. the work budget, with runs whose work differs widely -----------------------------------------------------------------
@gpu
def test_launches_cut_short_by_the_budget_change_nothing():
    _, spec = ps.load_fixture("pile")
    objects, _, _, st = ps.project_scene(spec)
    ticks, cam = spec["ticks"], vec3(*spec["cam"])
    movers = [k for k, o in enumerate(objects) if o.physics]
    # as recorded; one body falling at max_velocity; every body carried out of dist_move, where nothing wakes: a world at rest
    changes = [{}, {movers[0]: dict(vel=(0, -st.max_velocity, 0))}, {k: dict(pos=(objects[k].pos.x, 1000 + 8 * k, objects[k].pos.z)) for k in movers}]
    variants = [bu.mapping(objects, c) for c in changes]
    dw = DeviceWorld(16)
    whole = dw.run_many(objects, cam, st, ticks, variants, trace=True)
    cut = dw.run_many(objects, cam, st, ticks, variants, trace=True, budget=64)
    work = whole.stats[:, nat.S_PHYSICS_WORK]
    # (a body at rest costs its turn; one awake under gravity at least its turn, a step and the step's pass of box tests)
    assert work[2] == ticks * (1 + len(objects)) and work[0] > 2 * work[2] and not whole.stats[2, nat.S_PHYSICS_STEPS]
    assert cut.launches > 1 and cut.launches > whole.launches >= 1
    assert cut.ticks_run.tolist() == whole.ticks_run.tolist() == [ticks] * 3
    assert ru.same_records(whole.records, cut.records) and ru.same_records(whole.trace, cut.trace)
    for k in range(3):
        assert totals(whole.stats[k]) == totals(cut.stats[k]), k
        assert cut.stats[k, nat.S_PHYSICS_WORK] >= whole.stats[k, nat.S_PHYSICS_WORK]
    # a budget of one unit: a launch per tick, for every run at once
    single = dw.run_many(objects, cam, st, 4, variants, budget=1)
    assert single.launches == 4 and ru.same_records(single.records, dw.run_many(objects, cam, st, 4, variants).records)


# ---- 4. more runs than workgroups are resident at once -----------------------------------------------------------------------
@gpu
def test_six_hundred_runs_in_rounds():
    spec, objects, st, cam, eight = tiny()
    ticks = spec["ticks"]
    dw = DeviceWorld(8)
    variants = [bu.mapping(objects, eight[i % 8]) for i in range(600)]
    r = dw.run_many(objects, cam, st, ticks, variants, trace=True)
    assert r.ticks_run.tolist() == [ticks] * 600 and r.launches == 1
    for i in range(600):
        assert ru.same_records(r.records[i], r.records[i % 8]) and ru.same_records(r.trace[i], r.trace[i % 8]), i
        assert np.array_equal(r.stats[i], r.stats[i % 8]), i
    for k in range(8):
        t = dw.run(bu.altered(objects, eight[k]), cam, st, ticks, trace=True)
        assert ru.same_records(r.records[k], t.records) and ru.same_records(r.trace[k], t.trace) and np.array_equal(r.stats[k], t.stats), k
    assert len({r.trace[k].tobytes() for k in range(8)}) == 8
    # a permutation of the variants permutes the result
    order = np.random.default_rng(7).permutation(600)
    p = dw.run_many(objects, cam, st, ticks, [variants[i] for i in order], trace=True)
    assert ru.same_records(p.records, r.records[order]) and ru.same_records(p.trace, r.trace[order]) and np.array_equal(p.stats, r.stats[order])


# ---- 5. a run the device refuses stays alone ---------------------------------------------------------------------------------
@gpu
def test_a_refused_variant_touches_no_other_run():
    spec, objects, st, cam, eight = tiny()
    ticks = spec["ticks"]
    thrown = {1: dict(vel=(0, -1025.0, 0))}                     # beyond VRT_PHYSICS_MAX_VEL
    dw = DeviceWorld(8)
    r = dw.run_many(objects, cam, st, ticks, [bu.mapping(objects, c) for c in (eight[0], thrown, eight[1], eight[3])], trace=True)
    without = dw.run_many(objects, cam, st, ticks, [bu.mapping(objects, c) for c in (eight[0], eight[1], eight[3])], trace=True)
    assert r.trace[1][0][1]["status"] == nat.BODY_REFUSED and (r.trace[1][:, 1]["status"] == nat.BODY_REFUSED).all()
    assert r.stats[:, nat.S_PHYSICS_REFUSED].tolist() == [0, ticks, 0, 0]
    assert r.records[1][1]["vel"].tolist() == [0, -1025.0, 0] and r.records[1][1]["pos"].tolist() == list(objects[1].pos.tuple())
    keep = [0, 2, 3]
    assert ru.same_records(r.records[keep], without.records) and ru.same_records(r.trace[keep], without.trace)
    assert np.array_equal(r.stats[keep], without.stats)
    # ... as run() on a twin leaves it: the velocity the twin was given stays
    twin = bu.altered(objects, thrown)
    t = dw.run(twin, cam, st, ticks, trace=True)
    assert ru.same_records(r.records[1], t.records) and ru.same_records(r.trace[1], t.trace)
    mine = bu.twins(objects)
    r.apply(1, mine)
    assert same_state(mine, twin)


# ---- 6. a batch of one is run() ----------------------------------------------------------------------------------------------
@gpu
def test_a_batch_of_one_applied_is_run():
    props = lambda i: dict(function=material, albedo=rgb(200, 100, 50), roughness=0.0, absorption=1.0, ior=0.0, energy=0.0)  # noqa: E731
    spec = ps.scene({"slab": ps.full((32, 2, 32), 0), "ball": ps.full((4, 4, 4), 1), "cube": ps.full((4, 4, 4), 0)},
                    [ps.obj("slab", (0, 0, 0), physics=False), ps.obj("ball", (6, 10, 0)), ps.obj("cube", (0, 20, 0), rot=(0, 90, 0))], 10,
                    dist_move=24, dist_max=40)
    who = 2                                                    # the cube carries the camera, 3 forward and 4 up
    a, _, _, st = ps.project_scene(spec, props)
    b, _, _, _ = ps.project_scene(spec, props)
    far = vec3(1e6, 1e6, 1e6)
    dwa, dwb = DeviceWorld(8), DeviceWorld(8)
    for objects in (a, b):
        objects[who].set_camera(vec2(3, 4))
        ps.clear_redraw(objects)
    r = dwa.run_many(a, far, st, spec["ticks"], [{}], follow=a[who], trace=True)
    t = dwb.run(b, far, st, spec["ticks"], follow=b[who], trace=True)
    assert len(r.records) == 1 and ru.same_records(r.records[0], t.records) and ru.same_records(r.trace[0], t.trace)
    assert np.array_equal(r.stats[0], t.stats) and r.launches == t.launches and r.ticks_run.tolist() == [t.ticks_run]
    assert not same_state(a, b)                                # not yet
    moved = r.apply(0, a)
    assert same_state(a, b) and [a.index(o) for o in moved] == [b.index(o) for o in t.moved] and moved
    assert all(np.array_equal(ru.bits(x.cam_pos.tuple()), ru.bits(y.cam_pos.tuple())) for x, y in zip(a, b))
    assert [o.redraw for o in a] == [o.redraw for o in b] and any(o.redraw for o in a)
    # choose, commit, update: both worlds rebuild the same chunks
    (_, rebuilt_a), (_, rebuilt_b) = dwa.update(a), dwb.update(b)
    assert rebuilt_a == rebuilt_b > 0 and not any(o.redraw for o in a)


# ---- 7. untouched until applied ----------------------------------------------------------------------------------------------
@gpu
def test_the_callers_objects_are_untouched():
    _, spec = ps.load_fixture("pile")
    objects, _, _, st = ps.project_scene(spec)
    objects[3].redraw = False
    before = ps.state(objects)
    held = [(o.pos, o.vel, o.mins, o.maxs) for o in objects]
    r = DeviceWorld(16).run_many(objects, vec3(*spec["cam"]), st, 6, [{}, bu.mapping(objects, {3: dict(pos=(0, 30, 0), vel=(1, 0, 0))})], trace=True)
    assert (r.records["pad"][:, :, 0] & nat.BODY_EVER_MOVED).any() and r.trace is not None
    assert unchanged(before, objects) and not objects[3].redraw
    assert all(h[0] is o.pos and h[1] is o.vel and h[2] is o.mins and h[3] is o.maxs for h, o in zip(held, objects))
    with pytest.raises(ValueError):
        r.apply(0, objects[:3])
    for bad in (dict(ticks=0), dict(ticks=2, budget=0)):
        with pytest.raises(ValueError):
            DeviceWorld(16).run_many(objects, vec3(0, 0, 0), st, variants=[{}], **bad)
    with pytest.raises(ValueError):
        DeviceWorld(16).run_many(objects, vec3(0, 0, 0), st, 2, [])
    with pytest.raises(ValueError):
        DeviceWorld(16).run_many(objects, vec3(0, 0, 0), st, 2, [{}] * 4097)
    assert unchanged(before, objects)


# ---- 8. straight through the C ABI -------------------------------------------------------------------------------------------
class Abi:
    """Scene `tiny` as DeviceWorld.run_many packs it, for direct calls of vrt_physics_run_batch."""

    def __init__(self):
        import torch
        self.torch = torch
        self.spec, self.objects, self.st, _, _ = tiny()
        self.dw = DeviceWorld(8)
        flags = [(False, False, False)] * len(self.objects)
        self.bodies, remap, mats, matphys = self.dw._pack_bodies(self.objects, flags, [True] * len(self.objects), False, "test")
        self.dw._flush_models()
        self.models = self.dw._model_dev
        dev = self.dw.device
        self.remap = torch.from_numpy(np.array(remap, np.uint8)).to(dev)
        self.matphys = torch.from_numpy(matphys.reshape(-1)).to(dev)
        self.n_materials = len(mats)
        self.ticks = self.spec["ticks"]

    def call(self, runs, done, n=None, budget=1 << 40, trace=True):
        """(status, bodies [runs][n], trace [runs][ticks][n], stats [runs][16], ticks done [runs]) after one launch."""
        torch, dev = self.torch, self.dw.device
        n = len(self.bodies) if n is None else n
        start = np.tile(self.bodies[:n], (runs, 1))
        d_bodies = torch.from_numpy(start.view(np.uint8).reshape(-1).copy()).to(dev) if n else None
        d_trace = torch.full((runs * self.ticks * n * nat.BODY_SAMPLE_BYTES,), 0xAB, dtype=torch.uint8, device=dev) if trace and n else None
        d_done = torch.tensor(done, dtype=torch.int32, device=dev)
        stats = torch.full((runs * nat.NSTATS,), -1, dtype=torch.int64, device=dev)
        st = self.st
        params = nat.VrtPhysicsParams(float(st.gravity), float(st.friction), float(st.friction_air), float(st.min_velocity), float(st.max_velocity))
        rp = nat.VrtPhysicsRunParams((C.c_double * 3)(*self.spec["cam"]), (C.c_double * 3)(0.0, 0.0, 0.0), float(st.dist_max), float(st.dist_move),
                                     budget, self.ticks, -1)
        status = nat.lib().vrt_physics_run_batch(d_bodies.data_ptr() if n else None, runs, n, self.models.data_ptr(), self.models.numel(),
                                                 self.remap.data_ptr(), self.remap.numel(), self.matphys.data_ptr(), self.n_materials,
                                                 C.byref(params), C.byref(rp), d_done.data_ptr(), d_trace.data_ptr() if d_trace is not None else None,
                                                 stats.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return (status, d_bodies.cpu().numpy().view(np.dtype(nat.BODY_FIELDS)).reshape(runs, n) if n else start,
                d_trace.cpu().numpy().reshape(runs, -1) if d_trace is not None else None, stats.cpu().numpy().reshape(runs, nat.NSTATS),
                d_done.cpu().numpy())


@gpu
def test_the_abi_refuses_bad_arguments_and_leaves_bad_runs_alone():
    bu.assert_refusals(nat.lib())                      # VRT_ERR_ARG before any HIP call, with a device present as without
    abi = Abi()
    ticks, n = abi.ticks, len(abi.bodies)
    status, whole, whole_trace, whole_stats, done = abi.call(3, [0, 0, 0])
    assert status == 0 and done.tolist() == [ticks] * 3 and whole_stats[:, nat.S_PHYSICS_TICKS].tolist() == [ticks] * 3
    assert ru.same_records(whole[0], whole[1]) and (whole[0]["pad"][:, 0] & nat.BODY_EVER_MOVED).any()
    assert not whole_stats[:, nat.S_PHYSICS_BATCH_BADTICK].any() and not (whole_trace == 0xAB).all(axis=1).any()
    # no bodies: every run reports its ticks done
    status, _, _, stats, done = abi.call(3, [0, 4, ticks], n=0)
    assert status == 0 and done.tolist() == [ticks] * 3 and stats[:, nat.S_PHYSICS_TICKS].tolist() == [ticks, ticks - 4, 0]
    assert not np.delete(stats, nat.S_PHYSICS_TICKS, axis=1).any()
    # an entry of d_ticks_done outside [0, n_ticks]: that run is left alone and says so, the others complete; a run that is
    # done already writes zeroed statistics and touches nothing
    status, bodies, trace, stats, done = abi.call(5, [0, -1, ticks + 1, ticks, 0])
    assert status == 0 and done.tolist() == [ticks, -1, ticks + 1, ticks, ticks]
    assert stats[:, nat.S_PHYSICS_BATCH_BADTICK].tolist() == [0, 1, 1, 0, 0] and stats[:, nat.S_PHYSICS_TICKS].tolist() == [ticks, 0, 0, 0, ticks]
    for k in (1, 2, 3):
        assert bodies[k].tobytes() == abi.bodies.tobytes() and (trace[k] == 0xAB).all(), k
        assert not np.delete(stats[k], nat.S_PHYSICS_BATCH_BADTICK).any(), k
    for k in (0, 4):
        assert ru.same_records(bodies[k], whole[0]) and np.array_equal(trace[k], whole_trace[0]) and np.array_equal(stats[k], whole_stats[0]), k
    # a run picked up in the middle writes only the rows of the ticks it does
    status, _, trace, stats, done = abi.call(2, [0, 0], budget=1)
    assert status == 0 and done.tolist() == [1, 1] and stats[:, nat.S_PHYSICS_TICKS].tolist() == [1, 1]
    row = n * nat.BODY_SAMPLE_BYTES
    assert np.array_equal(trace[:, :row], whole_trace[:2, :row]) and (trace[:, row:] == 0xAB).all()


# ---- 9. what the batch does not do -------------------------------------------------------------------------------------------
@gpu
def test_fractional_solidity_raises():
    _, spec = ps.load_fixture("fraction")
    objects, _, _, st = ps.project_scene(spec)
    before = ps.state(objects)
    with pytest.raises(ValueError, match="fractional solidity"):
        DeviceWorld(8).run_many(objects, vec3(*spec["cam"]), st, 4, [{}, {}])
    assert unchanged(before, objects)
