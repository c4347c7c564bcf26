"""Many physics ticks in one device call with the reference's random draws (DeviceWorld.run(rng=), vrt_physics_run_draws): the
runs recorded from the real reference with seeded draws, in segments between the scripts' ticks, every tick bit for bit, each
tick's draws and the generator after every segment; `wade` (the camera rides on a body that falls into a pool) and `tide` (a
platform whose frames differ in solidity) of tests/golden/physics_run_draws.npz; a twin stepped tick by tick; launches cut short
by the work budget; generators that start at any index; host and device runs taking turns on one generator; the all-solid
scenes, whose draws decide nothing; what stays as it was without rng; and an index word out of range through the raw ABI.
Every comparison is bit for bit."""
import ctypes as C
import random

import numpy as np
import pytest

import physics_anim_scenes as an
import physics_draw_scenes  # noqa: F401  (the scenes the draw fixtures were recorded from)
import physics_run_draw_scenes as rd
import physics_run_util as ru
import physics_scenes as ps
from python_raytracer_amd import _native as nat
from python_raytracer_amd import world
from python_raytracer_amd.lib import vec3
from python_raytracer_amd.world import DeviceWorld

gpu = pytest.mark.gpu
WORDS = ("BODIES", "REFUSED", "STEPS", "BLOCKED", "CONTACTS", "TRANSFERS", "CAPPED", "DRAWS")
COUNTERS = [f for f, _ in world.PHYSICS_COUNTER_FIELDS]


def totals(stats):
    return {w: int(stats[getattr(nat, "S_PHYSICS_" + w)]) for w in WORDS}


def same_state(a, b):
    sa, sb = ps.state(a), ps.state(b)
    return all(sa[f].tobytes() == sb[f].tobytes() for f in sa)


def at_index(seed, index):
    """A generator whose next output is word `index` of its state (a fresh seed leaves 624)."""
    gen = random.Random(seed)
    if index != 624:
        for _ in range(index):
            gen.getrandbits(32)
    assert gen.getstate()[1][-1] == index
    return gen


def assert_row_is_objects(row, objects, counters, what):
    """One row of a run's trace against the objects a tick loop has just stepped, and that tick's counters."""
    st = ps.state(objects)
    for f in ("pos", "vel"):
        assert np.array_equal(ru.bits(row[f]), ru.bits(st[f])), (what, f, row[f], st[f])
    assert np.array_equal(row["mins"], st["mins"]) and np.array_equal(row["maxs"], st["maxs"]), what
    assert np.array_equal(row["visible"] != 0, st["visible"]), what
    for f in COUNTERS:
        assert np.array_equal(row[f], counters[f]), (what, f, row[f], counters[f])


def in_segments(name, gen_dev, gen_host, record=True, budget=None):
    """The fixture's scene in segments: DeviceWorld.run(rng=gen_dev) on one set of objects, world.run(rng=gen_host.random) on a
    twin, held to each other in every tick's records and in the generators after every segment, and (record) to the fixture.
    Returns (the RunResults, the draws of every tick)."""
    z, spec = ps.load_fixture(name)
    dev, _, _, st = ps.project_scene(spec)
    host, _, _, _ = ps.project_scene(spec)
    has_sprite = np.array([bool(o.sprite) for o in dev])
    dw = DeviceWorld(16)
    cam, results, draws = spec["cam"], [], []
    for first, last in ru.segments(spec):
        for objects in (dev, host):
            ps.clear_redraw(objects)
            at = ps.apply_script(spec, first, objects, vec3, cam)
        cam = at
        entry = ps.state(dev)
        r = dw.run(dev, vec3(*cam), st, last - first, trace=True, rng=gen_dev, budget=budget)
        assert r.ticks_run == last - first and r.trace.shape == (last - first, len(dev))
        assert r.draws_per_tick.dtype == np.uint64 and r.draws_per_tick.shape == (last - first,)
        assert r.draws == int(r.draws_per_tick.sum()) == int(r.stats[nat.S_PHYSICS_DRAWS]) and r.stats[nat.S_PHYSICS_RNG_INVALID] == 0
        if record:
            ru.assert_segment(z, first, r.trace, entry, has_sprite, name + " (run, rng)")
            if "draws" in z.files:
                assert r.draws_per_tick.tolist() == z["draws"][first:last].tolist(), (name, first)
        counters, trace = world.run(host, vec3(*cam), st, last - first, trace=True, rng=gen_host.random)
        assert ru.same_records(r.trace, trace), (name, first)
        assert gen_dev.getstate() == gen_host.getstate(), (name, first)
        assert same_state(dev, host) and np.array_equal(r.counters, counters[-1]), (name, first)
        results.append(r)
        draws += r.draws_per_tick.tolist()
    return results, draws


# ---- 1. the recorded runs --------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", ["fluid", "fraction", "brim", "classes", "crowd_fluid"])
def test_device_run_makes_the_references_draws(name):
    _, spec = ps.load_fixture(name)
    _, draws = in_segments(name, random.Random(spec["seed"]), random.Random(spec["seed"]))
    assert sum(draws) > 0 and (name != "fluid" or 2 * sum(draws) > 3 * 624)


@gpu
@pytest.mark.parametrize("name", list(rd.SCENES))
def test_follow_clock_and_rng_together_are_the_references(name):
    z, spec, dev, sprites, st, who = rd.fresh(name)
    gen = random.Random(spec["seed"])
    r = DeviceWorld(8).run(dev, vec3(*spec["cam"]), st, spec["ticks"], follow=who, trace=True, clock=tuple(spec["clock"]), rng=gen)
    assert r.ticks_run == spec["ticks"] and r.trace.shape == r.anim.shape == (spec["ticks"], len(dev))
    an.assert_ticks(z, name, spec, dev, sprites, r.trace, r.anim, name + " (device)")
    assert r.draws_per_tick.tolist() == z[name + "/draws"].tolist() and r.draws == int(z[name + "/draws"].sum())
    assert np.array_equal(rd.state_words(gen), z[name + "/state"])
    # side by side with the host path: the counters of every tick and `switched` included
    _, _, host, host_sprites, _, who_host = rd.fresh(name)
    twin = random.Random(spec["seed"])
    counters, trace, anim = world.run(host, vec3(*spec["cam"]), st, spec["ticks"], follow=who_host, trace=True, clock=tuple(spec["clock"]),
                                      rng=twin.random)
    assert ru.same_records(r.trace, trace) and ru.same_records(r.anim, anim) and same_state(dev, host)
    assert gen.getstate() == twin.getstate() and np.array_equal(r.counters, counters[-1])
    assert [float(o.weight) for o in dev] == [float(o.weight) for o in host]
    if name == "tide":
        assert r.frames == {sprites["plat"]: host_sprites["plat"].frame} and (anim["switched"][:, 1] != 0).sum() >= 4
        assert not anim["switched"][:, [0, 2, 3]].any()            # the first platform makes every switch, for both
    else:
        assert who in r.moved and r.trace["awake"][0][2] == 0 and r.trace["awake"][-1][2] == 1                # the sleeper wakes


# ---- 2. against the loop of ticks ------------------------------------------------------------------------------------------
@gpu
def test_the_run_is_the_loop_of_device_ticks_with_rng():
    z, spec = ps.load_fixture("fluid")
    dev, _, _, st = ps.project_scene(spec)
    twin, _, _, _ = ps.project_scene(spec)
    gen, gen_twin = random.Random(spec["seed"]), random.Random(spec["seed"])
    cam = vec3(*spec["cam"])
    r = DeviceWorld(16).run(dev, cam, st, spec["ticks"], trace=True, rng=gen)
    dw, summed = DeviceWorld(16), dict.fromkeys(WORDS, 0)
    for k in range(spec["ticks"]):
        t = dw.tick(twin, cam, st, rng=gen_twin)
        assert_row_is_objects(r.trace[k], twin, t.counters, ("fluid", k))
        assert int(r.draws_per_tick[k]) == t.draws, k
        for w, v in totals(t.stats).items():
            summed[w] += v
    assert totals(r.stats) == summed and gen.getstate() == gen_twin.getstate() and same_state(dev, twin)
    assert int(r.stats[nat.S_PHYSICS_TICKS]) == spec["ticks"] and not r.stats[:5].any()


@gpu
def test_the_run_is_the_loop_of_host_ticks_with_a_clock_and_rng():
    z, spec, dev, sprites, st, _ = rd.fresh("tide")
    _, _, twin, twin_sprites, _, _ = rd.fresh("tide")
    gen, gen_twin = random.Random(spec["seed"]), random.Random(spec["seed"])
    cam = vec3(*spec["cam"])
    start, step = spec["clock"]
    r = DeviceWorld(8).run(dev, cam, st, spec["ticks"], trace=True, clock=(start, step), rng=gen)
    summed = dict.fromkeys(WORDS, 0)
    for k in range(spec["ticks"]):
        made = [0]

        def draw():
            made[0] += 1
            return gen_twin.random()
        want = world.tick(twin, cam, st, rng=draw, now=start + k * step)
        assert_row_is_objects(r.trace[k], twin, want, ("tide", k))
        assert int(r.draws_per_tick[k]) == made[0], k
        assert [bool(o.last_switched) for o in twin] == (r.anim[k]["switched"] != 0).tolist()
        assert np.array_equal(ru.bits(r.anim[k]["weight"]), ru.bits([float(o.weight) for o in twin]))
        ran = want[want["status"] == 0]
        for w, v in dict(BODIES=len(ran), REFUSED=0, STEPS=ran["steps"].sum(), BLOCKED=ran["blocked_steps"].sum(),
                         CONTACTS=ran["contacts"].sum(), TRANSFERS=ran["transfers"].sum(), CAPPED=0, DRAWS=made[0]).items():
            summed[w] += int(v)
    assert totals(r.stats) == summed and gen.getstate() == gen_twin.getstate()
    assert sprites["plat"].frame == twin_sprites["plat"].frame


# ---- 3. chained launches ----------------------------------------------------------------------------------------------------
def _one_run(name, budget):
    if name == "fluid":
        z, spec = ps.load_fixture(name)
        objects, _, _, st = ps.project_scene(spec)
        who, clock = None, None
    else:
        z, spec, objects, _, st, who = rd.fresh(name)
        clock = tuple(spec["clock"])
    gen = random.Random(spec["seed"])
    r = DeviceWorld(16).run(objects, vec3(*spec["cam"]), st, spec["ticks"], follow=who, trace=True, budget=budget, clock=clock, rng=gen)
    assert r.ticks_run == spec["ticks"] == int(r.stats[nat.S_PHYSICS_TICKS])
    return r, gen, spec


@gpu
@pytest.mark.parametrize("name", ["fluid", "wade"])
def test_launches_cut_short_by_the_budget_change_nothing(name):
    whole, gen_whole, spec = _one_run(name, None)
    single, gen_single, _ = _one_run(name, 1)
    part, gen_part, _ = _one_run(name, int(whole.stats[nat.S_PHYSICS_WORK]) // 3)       # a launch ends about three times in the run
    assert whole.launches == 1 or int(whole.stats[nat.S_PHYSICS_WORK]) >= nat.PHYSICS_RUN_DRAWS_BUDGET
    assert single.launches == spec["ticks"] and whole.launches < part.launches < spec["ticks"]
    for other, gen in ((single, gen_single), (part, gen_part)):
        assert ru.same_records(whole.records, other.records) and ru.same_records(whole.trace, other.trace)
        assert np.array_equal(whole.draws_per_tick, other.draws_per_tick) and gen.getstate() == gen_whole.getstate()
        assert np.array_equal(whole.stats, other.stats)
        if name == "wade":
            assert ru.same_records(whole.anim, other.anim)
    assert 2 * whole.draws > 3 * 624                           # the state handed from launch to launch has been twisted


# ---- 4. any start index -----------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("index", [1, 2, 623, 624])
def test_generators_that_start_at_any_index(index):
    _, spec = ps.load_fixture("fraction")
    in_segments("fraction", at_index(spec["seed"], index), at_index(spec["seed"], index), record=index == 624)


@gpu
@pytest.mark.parametrize("index", [272, 273])
def test_brim_as_one_run_from_the_edge_of_the_eighth_state(index):
    """brim's first pass makes 2048 draws, 4096 outputs: from index 272 its last output is the last word of the seventh state after
    the current one and the generator is left untwisted at 624; from 273 it is word 0 of the eighth."""
    _, spec = ps.load_fixture("brim")
    assert not spec["script"] and spec["ticks"] == 3
    results, draws = in_segments("brim", at_index(spec["seed"], index), at_index(spec["seed"], index), record=False)
    assert len(results) == 1 and results[0].launches == 1 and max(draws) >= 2048


# ---- 5. host and device runs take turns -------------------------------------------------------------------------------------
@gpu
def test_host_and_device_runs_take_turns_on_one_generator():
    z, spec = ps.load_fixture("fluid")
    mixed, _, _, st = ps.project_scene(spec)
    host, _, _, _ = ps.project_scene(spec)
    gen, gen_host = random.Random(spec["seed"]), random.Random(spec["seed"])
    cam = vec3(*spec["cam"])
    dw = DeviceWorld(16)
    a, b = 5, 4
    r1 = dw.run(mixed, cam, st, a, rng=gen)
    world.run(mixed, cam, st, b, rng=gen.random)
    r2 = dw.run(mixed, cam, st, spec["ticks"] - a - b, rng=gen.random)             # (a bound method is the generator behind it)
    counters, _ = world.run(host, cam, st, spec["ticks"], rng=gen_host.random)
    assert same_state(mixed, host) and gen.getstate() == gen_host.getstate()
    assert np.array_equal(r2.counters, counters[-1]) and r1.draws + r2.draws > 0
    got = ps.state(mixed)                                      # (`redraw` accumulates over a run: the other fields)
    for f in ("pos", "vel", "mins", "maxs", "visible"):
        assert got[f].tobytes() == np.ascontiguousarray(z[f][-1]).tobytes(), f


# ---- 6. all-solid scenes: the draws decide nothing and are made all the same ------------------------------------------------
@gpu
@pytest.mark.parametrize("name", ["edges_face", "crowd", "default"])
def test_solid_scenes_draw_and_move_as_without_rng(name):
    results, draws = in_segments(name, random.Random(11), random.Random(11))
    assert sum(draws) > (2000 if name == "edges_face" else 0)
    # positions and velocities are those of the run without rng
    z, spec = ps.load_fixture(name)
    plain, _, _, st = ps.project_scene(spec)
    dw = DeviceWorld(16)
    cam = spec["cam"]
    for (first, last), r in zip(ru.segments(spec), results):
        ps.clear_redraw(plain)
        cam = ps.apply_script(spec, first, plain, vec3, cam)
        p = dw.run(plain, vec3(*cam), st, last - first, trace=True)
        assert p.draws is None and p.draws_per_tick is None and p.stats[nat.S_PHYSICS_DRAWS] == 0
        assert ru.same_records(p.trace, r.trace), (name, first)


@gpu
@pytest.mark.parametrize("name", ["weights", "wake"])
def test_animated_solid_scenes_draw_and_equal_their_record(name):
    """The animated scenes of tests/golden/physics_anim.npz are all solid: with a generator they move as recorded.  In `weights` the
    switching body is physical and collides AS its new frame in the tick of the switch: the switch comes before its draws."""
    z, spec, dev, sprites, st, who = an.fresh(name)
    _, _, host, _, _, who_host = an.fresh(name)
    gen, twin = random.Random(13), random.Random(13)
    cam, clock = vec3(*spec["cam"]), tuple(spec["clock"])
    r = DeviceWorld(8).run(dev, cam, st, spec["ticks"], follow=who, trace=True, clock=clock, rng=gen)
    an.assert_ticks(z, name, spec, dev, sprites, r.trace, r.anim, name + " (device, rng)")
    _, trace, anim = world.run(host, cam, st, spec["ticks"], follow=who_host, trace=True, clock=clock, rng=twin.random)
    assert ru.same_records(r.trace, trace) and ru.same_records(r.anim, anim) and gen.getstate() == twin.getstate() and r.draws > 0
    physical = np.array([o["physics"] for o in spec["objects"]])
    assert name != "weights" or (anim["switched"][:, physical] != 0).any()


# ---- 7. what stays as it was ------------------------------------------------------------------------------------------------
@gpu
def test_without_rng_nothing_changes(monkeypatch):
    _, spec = ps.load_fixture("fraction")
    objects, _, _, st = ps.project_scene(spec)
    before = ps.state(objects)
    dw = DeviceWorld(8)
    with pytest.raises(ValueError, match="fractional solidity"):
        dw.run(objects, vec3(*spec["cam"]), st, 3)
    for bad in (object(), 5, lambda: 0.5, "random"):
        with pytest.raises(TypeError, match="rng"):
            dw.run(objects, vec3(*spec["cam"]), st, 3, rng=bad)
    after = ps.state(objects)
    assert all(np.array_equal(before[k], after[k]) for k in before)
    # a run with a clock and without rng still launches vrt_physics_run_anim, one without either vrt_physics_run
    L = nat.lib()
    called = []

    def spy(name):
        real = getattr(L, name)

        def call(*args):
            called.append(name)
            return real(*args)
        monkeypatch.setattr(L, name, call)
    for name in ("vrt_physics_run", "vrt_physics_run_anim", "vrt_physics_run_draws"):
        spy(name)
    z, spec, dev, sprites, st, who = an.fresh("platform")
    r = DeviceWorld(8).run(dev, vec3(*spec["cam"]), st, spec["ticks"], trace=True, clock=tuple(spec["clock"]))
    assert called == ["vrt_physics_run_anim"] * r.launches and r.draws is None and r.draws_per_tick is None
    an.assert_ticks(z, "platform", spec, dev, sprites, r.trace, r.anim, "platform (no rng)")
    del called[:]
    z, spec, dev, sprites, st, who = an.fresh("platform")
    r = DeviceWorld(8).run(dev, vec3(*spec["cam"]), st, 2)
    assert called == ["vrt_physics_run"] * r.launches
    del called[:]
    z, spec, dev, sprites, st, who = an.fresh("platform")
    gen = random.Random(1)
    r = DeviceWorld(8).run(dev, vec3(*spec["cam"]), st, spec["ticks"], trace=True, clock=tuple(spec["clock"]), rng=gen)
    assert called == ["vrt_physics_run_draws"] * r.launches and r.draws > 0
    an.assert_ticks(z, "platform", spec, dev, sprites, r.trace, r.anim, "platform (all solid, rng)")     # the draws decide nothing


# ---- 8. the raw ABI: an index word out of range -----------------------------------------------------------------------------
@gpu
def test_an_index_out_of_range_ends_the_launch_before_its_first_tick():
    import torch
    from test_gpu_physics import _hand_scene
    models, remap, matphys, slab, cube, free = _hand_scene()
    bodies = np.array([slab, cube, free])
    bodies["steps"], bodies["moved"], bodies["status"] = 9, 9, 9        # not even the `out` words are written
    dev = torch.device("cuda", torch.cuda.current_device())
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)  # noqa: E731
    d_m, d_r, d_p = up(models), up(remap), up(matphys)
    words = np.array(random.Random(3).getstate()[1], np.uint32)
    p = nat.VrtPhysicsParams(1.0, 1.0, 0.125, 2.0 ** -7, 8.0)
    ticks = 2

    def call(index):
        words[624] = index
        d_b, d_rng = up(bodies), up(words)
        d_trace = torch.full((ticks * len(bodies) * nat.BODY_SAMPLE_BYTES,), 0x5A, dtype=torch.uint8, device=dev)
        d_draws = torch.full((ticks,), 77, dtype=torch.int64, device=dev)
        stats = torch.full((nat.NSTATS,), 77, dtype=torch.int64, device=dev)
        rp = nat.VrtPhysicsRunParams((C.c_double * 3)(0.0, 0.0, 0.0), (C.c_double * 3)(0.0, 0.0, 0.0), 96.0, 64.0, 1 << 40, ticks, -1)
        rc = nat.lib().vrt_physics_run_draws(d_b.data_ptr(), len(bodies), d_m.data_ptr(), d_m.numel(), d_r.data_ptr(), d_r.numel(),
                                             d_p.data_ptr(), 1, C.byref(p), C.byref(rp), d_trace.data_ptr(), stats.data_ptr(),
                                             torch.cuda.current_stream().cuda_stream, None, None, 0, None, 0, None, None,
                                             d_rng.data_ptr(), d_draws.data_ptr())
        assert rc == 0, rc
        torch.cuda.synchronize()
        return (d_b.cpu().numpy().view(np.dtype(nat.BODY_FIELDS)), stats.cpu().numpy(), d_rng.cpu().numpy().view(np.uint32),
                d_draws.cpu().numpy(), d_trace.cpu().numpy())

    for index in (625, 0xFFFFFFFF):
        out, st, after, draws, trace = call(index)
        assert out.tobytes() == bodies.tobytes()                 # not a byte of a body changed,
        assert np.array_equal(after, words)                      # nor a word of the generator,
        assert (draws == 77).all() and (trace == 0x5A).all()     # nor a draw count, nor the trace
        assert st[nat.S_PHYSICS_RNG_INVALID] == 1 and st[nat.S_PHYSICS_TICKS] == 0
        assert not np.delete(st, [nat.S_PHYSICS_RNG_INVALID]).any()
    # the same records with a legal index: the cube comes down on the slab, 4 x 2 + 5 draws at the first tick (as the tick's test)
    out, st, after, draws, trace = call(624)
    assert st[nat.S_PHYSICS_RNG_INVALID] == 0 and st[nat.S_PHYSICS_TICKS] == ticks and draws[0] == 13
    assert st[nat.S_PHYSICS_DRAWS] == draws.sum()
    gen = random.Random(3)
    for _ in range(int(draws.sum())):
        gen.random()
    assert np.array_equal(after, np.array(gen.getstate()[1], np.uint32))
    # DeviceWorld.run turns the refusal into VrtError and leaves the generator alone
    _, spec = ps.load_fixture("fraction")
    objects, _, _, s = ps.project_scene(spec)

    class Broken(random.Random):
        def getstate(self):
            version, state, gauss = super().getstate()
            return version, state[:-1] + (625,), gauss
    gen = Broken(5)
    before, state = ps.state(objects), random.Random.getstate(gen)
    with pytest.raises(nat.VrtError, match="index"):
        DeviceWorld(8).run(objects, vec3(*spec["cam"]), s, 2, rng=gen)
    assert random.Random.getstate(gen) == state
    after = ps.state(objects)
    assert all(np.array_equal(before[k], after[k]) for k in before)
