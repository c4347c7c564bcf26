"""Many what-if runs with the reference's random draws in one device call (DeviceWorld.run_many(rng=),
vrt_physics_run_batch_draws): every variant of a batch, under a generator of its own, byte for byte DeviceWorld.run(rng=) on a
hand-made twin and world.run(rng=) on a host twin -- records, trace, statistics, draws, the generator's final words; K seeds of one
variant as K different futures; launches cut short by the budget; more runs than workgroups are resident at once; an all-solid world;
runs whose device data is bad, through the C ABI; and apply() with the generator."""
import ctypes as C
import random

import numpy as np
import pytest

import physics_batch_util as bu
import physics_draw_scenes  # noqa: F401  (the scenes the draw fixtures were recorded from)
import physics_run_draw_scenes as rd
import physics_run_util as ru
import physics_scenes as ps
from python_raytracer_amd import _native as nat
from python_raytracer_amd import world
from python_raytracer_amd.lib import vec3
from python_raytracer_amd.world import DeviceWorld

gpu = pytest.mark.gpu


def copy_of(g):
    c = random.Random()
    c.setstate(g.getstate())
    return c


def at_index(seed, index):
    """A generator whose next output is word `index` of its state.  A fresh seed leaves 624; getrandbits(32) calls reach 1 .. 624
    (CPython regenerates at 624 and hands out word 0 in the same call, so no call ever leaves 0 behind); 0 is what setstate()
    accepts besides: the words a generator has after `seed`'s first call, with the index word set back to 0."""
    gen = random.Random(seed)
    if index == 0:
        gen.getrandbits(32)
        version, words, gauss = gen.getstate()
        gen.setstate((version, words[:-1] + (0,), gauss))
    elif index != 624:
        for _ in range(index):
            gen.getrandbits(32)
    assert gen.getstate()[1][-1] == index
    return gen


def six_generators(seed):
    """Six generators in different states, three of them at the index words 0, 623 (a draw's two outputs straddle a
    regeneration) and 624 (the first draw regenerates)."""
    gens = [at_index(seed, 624), at_index(seed + 1, 623), at_index(seed + 2, 0), at_index(seed + 3, 1), random.Random(seed + 4),
            random.Random(seed + 5)]
    for g, n in zip(gens[4:], (5000, 101)):
        for _ in range(n):
            g.random()
    assert [g.getstate()[1][-1] for g in gens[:4]] == [624, 623, 0, 1] and len({g.getstate() for g in gens}) == 6
    return gens


def same_state(a, b):
    sa, sb = ps.state(a), ps.state(b)
    return all(sa[f].tobytes() == sb[f].tobytes() for f in sa)


def unchanged(before, objects):
    after = ps.state(objects)
    return all(before[f].tobytes() == after[f].tobytes() for f in before)


def scene(name):
    """(objects, settings, camera, followed object or None, ticks, chunk size of the DeviceWorld): `wade` without its clock and with
    follow (undecided tests), `fluid` for half its ticks, `brim` for its three (a pass makes 2048 draws and regenerates the state
    several times)."""
    if name == "wade":
        _, spec, objects, _, st, who = rd.fresh("wade")
        return objects, st, vec3(*spec["cam"]), who, spec["ticks"], 8
    _, spec = ps.load_fixture(name)
    objects, _, _, st = ps.project_scene(spec)
    ps.clear_redraw(objects)
    return objects, st, vec3(*spec["cam"]), None, {"fluid": 12, "brim": 3}[name], 16


def small():
    """The smallest drawing world: a cube of solidity 0.5 resting on a bed of solidity 0.25, which holds it up one test in four."""
    spec = dict(settings=dict(rd.SETTINGS), cam=[0.0, 0.0, 0.0], materials=rd.MATS,
                sprites={"bed": ps.full((6, 2, 6), 1), "cube": ps.full((2, 2, 2), 2)},
                objects=[ps.obj("bed", (0, 0, 0), physics=False), ps.obj("cube", (0, 2, 0))], ticks=8, script={}, seed=None)
    objects, _, _, st = ps.project_scene(spec)
    ps.clear_redraw(objects)
    four = [{}, {1: dict(vel=(0.5, 0, 0))}, {1: dict(pos=(1, 2, -1))}, {1: dict(pos=(0, 4, 0), vel=(0, -2.5, 0.25))}]
    return objects, st, vec3(0.0, 0.0, 0.0), spec["ticks"], four


def assert_variant_is_run(r, k, dw, objects, change, cam, st, ticks, who, gen, host=True):
    """Variant k of the batch `r` against DeviceWorld.run(rng=) on a hand-made twin and (host) world.run(rng=) on another, each with
    a copy of `gen`: every byte of the records, the trace and the statistics, the draws and the generator's final state."""
    twin, g = bu.altered(objects, change), copy_of(gen)
    t = dw.run(twin, cam, st, ticks, follow=twin[objects.index(who)] if who is not None else None, trace=True, rng=g)
    assert ru.same_records(r.records[k], t.records) and ru.same_records(r.trace[k], t.trace), k
    assert np.array_equal(r.stats[k], t.stats), (k, r.stats[k], t.stats)
    assert int(r.draws[k]) == t.draws == int(r.stats[k][nat.S_PHYSICS_DRAWS]) and np.array_equal(r.draws_per_tick[k], t.draws_per_tick), k
    assert r.rng_state(k) == g.getstate(), k
    if host:
        other, h = bu.altered(objects, change), copy_of(gen)
        counters, states = world.run(other, cam, st, ticks, follow=other[objects.index(who)] if who is not None else None, trace=True, rng=h.random)
        assert ru.same_records(r.trace[k], states) and np.array_equal(r.counters[k], counters[-1]), k
        assert r.rng_state(k) == h.getstate(), k
    return t


# ---- 1. every variant is the run of its twin ---------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", ["wade", "fluid", "brim"])
def test_every_variant_is_the_run_of_its_twin(name):
    objects, st, cam, who, ticks, chunk = scene(name)
    entry = ps.state(objects)
    changes = bu.changes(objects, cam.tuple())
    assert len(changes) == 6 and changes[0] == {}
    gens = six_generators(977)
    before = [g.getstate() for g in gens]
    r = DeviceWorld(chunk).run_many(objects, cam, st, ticks, [bu.mapping(objects, c) for c in changes], follow=who, trace=True, rng=gens)
    assert unchanged(entry, objects) and [g.getstate() for g in gens] == before      # nothing of the caller's is touched
    assert r.records.shape == (6, len(objects)) and r.trace.shape == (6, ticks, len(objects)) and r.stats.shape == (6, nat.NSTATS)
    assert r.draws.shape == (6,) and r.draws_per_tick.shape == (6, ticks) and r.draws_per_tick.dtype == np.uint64
    assert r.ticks_run.tolist() == [ticks] * 6 and r.launches >= 1
    assert not r.stats[:, nat.S_PHYSICS_RNG_INVALID].any() and not r.stats[:, nat.S_PHYSICS_BATCH_BADTICK].any()
    dw = DeviceWorld(chunk)
    for k, change in enumerate(changes):
        assert_variant_is_run(r, k, dw, objects, change, cam, st, ticks, who, gens[k])
    assert r.draws.sum() > 0 and len({r.trace[k].tobytes() for k in range(6)}) == 6
    if name == "brim":
        assert r.draws_per_tick.max() >= 2 * 2048               # a step of two full passes: eight states behind one pass
    assert unchanged(entry, objects) and [g.getstate() for g in gens] == before


# ---- 2. K seeds of one variant -----------------------------------------------------------------------------------------------
@gpu
def test_sixty_four_seeds_of_one_variant_are_sixty_four_runs():
    """`wade` as it stands, without its clock, for its 20 ticks (tests/test_physics_batch_draws_host.py shows from world.run alone
    that its seeds end in different places)."""
    objects, st, cam, who, ticks, chunk = scene("wade")
    gens = [random.Random(seed) for seed in range(64)]
    r = DeviceWorld(chunk).run_many(objects, cam, st, ticks, [{}] * 64, follow=who, trace=True, rng=gens)
    dw = DeviceWorld(chunk)
    for k in range(64):
        assert_variant_is_run(r, k, dw, objects, {}, cam, st, ticks, who, gens[k])
    assert len({r.records[k].tobytes() for k in range(64)}) >= 2     # the generators are not shared between the workgroups
    assert len({r.rng_state(k) for k in range(64)}) == 64
    # one generator for all: 64 times the one future
    same = DeviceWorld(chunk).run_many(objects, cam, st, ticks, [{}] * 4, follow=who, trace=True, rng=gens[5])
    for k in range(4):
        assert ru.same_records(same.trace[k], r.trace[5]) and same.rng_state(k) == r.rng_state(5)
    assert gens[5].getstate() == random.Random(5).getstate()


# ---- 3. the work budget ------------------------------------------------------------------------------------------------------
@gpu
def test_launches_cut_short_by_the_budget_change_nothing():
    objects, st, cam, who, _, chunk = scene("fluid")
    ticks = 24                                                  # all of them: the raft reaches the pool at the fifth
    movers = [k for k, o in enumerate(objects) if o.physics]
    # as recorded; a body thrown; every physical body carried out of dist_move, where nothing wakes and nothing draws
    far = {k: dict(pos=(objects[k].pos.x, 1000 + 8 * k, objects[k].pos.z)) for k in movers}
    changes = [{}, {movers[1]: dict(vel=(0.5, -2.0, 0))}, far]
    variants = [bu.mapping(objects, c) for c in changes]
    gens = [at_index(31, 624), at_index(32, 623), at_index(33, 7)]
    before = [g.getstate() for g in gens]
    dw = DeviceWorld(chunk)
    whole = dw.run_many(objects, cam, st, ticks, variants, trace=True, rng=gens)
    work = whole.stats[:, nat.S_PHYSICS_WORK]
    assert work[2] == ticks * (1 + len(objects)) and work[0] > 2 * work[2]
    single = dw.run_many(objects, cam, st, ticks, variants, trace=True, rng=gens, budget=1)
    part = dw.run_many(objects, cam, st, ticks, variants, trace=True, rng=gens, budget=int(work[0]) // 2)
    assert single.launches == ticks and whole.launches < part.launches < ticks
    for other in (single, part):
        assert ru.same_records(whole.records, other.records) and ru.same_records(whole.trace, other.trace)
        assert np.array_equal(whole.stats, other.stats)           # launches differ and nothing else does: WORK and TICKS included
        assert np.array_equal(whole.draws, other.draws) and np.array_equal(whole.draws_per_tick, other.draws_per_tick)
        assert all(whole.rng_state(k) == other.rng_state(k) for k in range(3))
        assert other.ticks_run.tolist() == [ticks] * 3
    assert 2 * int(whole.draws[0]) > 3 * 624                     # the state handed from launch to launch has been twisted
    # the variant out of reach draws nothing, its generator comes back exactly as handed in, and it is done in one launch of the
    # budget that cuts the others
    assert whole.draws[2] == 0 and not whole.draws_per_tick[2].any() and whole.rng_state(2) == before[2]
    alone = dw.run_many(objects, cam, st, ticks, variants[2:], trace=True, rng=gens[2:], budget=int(work[0]) // 2)
    assert alone.launches == 1 < part.launches and ru.same_records(alone.trace[0], whole.trace[2]) and alone.rng_state(0) == before[2]
    assert [g.getstate() for g in gens] == before
    for k in (0, 1):
        assert_variant_is_run(whole, k, dw, objects, changes[k], cam, st, ticks, None, gens[k], host=False)


# ---- 4. more runs than workgroups are resident at once -----------------------------------------------------------------------
@gpu
def test_three_hundred_runs_in_rounds():
    objects, st, cam, ticks, four = small()
    gens = [random.Random(1000 + i) for i in range(300)]
    dw = DeviceWorld(8)
    r = dw.run_many(objects, cam, st, ticks, [bu.mapping(objects, four[i % 4]) for i in range(300)], trace=True, rng=gens)
    assert r.ticks_run.tolist() == [ticks] * 300 and r.launches == 1 and (r.draws > 0).all()
    for i in np.random.default_rng(7).permutation(300)[:12].tolist():
        assert_variant_is_run(r, i, dw, objects, four[i % 4], cam, st, ticks, None, gens[i])
    assert len({r.trace[i].tobytes() for i in range(0, 300, 4)}) >= 2      # 75 seeds of {}: more than one future


# ---- 5. a world with no fractional solidity ----------------------------------------------------------------------------------
@gpu
def test_an_all_solid_world_moves_as_without_rng_and_draws_all_the_same():
    _, spec = ps.load_fixture("edges_tiny")
    objects, _, _, st = ps.project_scene(spec)
    ps.clear_redraw(objects)
    cam, ticks = vec3(*spec["cam"]), spec["ticks"]
    changes = [{}, {1: dict(vel=(0.5, 0, 0))}, {1: dict(vel=(0, -3.25, 0.5))}, {1: dict(pos=(3, 7.5, -2))}]
    variants = [bu.mapping(objects, c) for c in changes]
    gens = [random.Random(70 + k) for k in range(4)]
    dw = DeviceWorld(8)
    r = dw.run_many(objects, cam, st, ticks, variants, trace=True, rng=gens)
    plain = dw.run_many(objects, cam, st, ticks, variants, trace=True)
    assert plain.draws is None and plain.draws_per_tick is None and plain.rng_state(0) is None
    assert ru.same_records(r.records, plain.records) and ru.same_records(r.trace, plain.trace)
    assert r.draws.sum() > 0                                     # the draws decide nothing and move the generators on
    for k, change in enumerate(changes):
        assert_variant_is_run(r, k, dw, objects, change, cam, st, ticks, None, gens[k])


# ---- 6. straight through the C ABI -------------------------------------------------------------------------------------------
class Abi:
    """The smallest drawing world as DeviceWorld.run_many(rng=) packs it, for direct calls of vrt_physics_run_batch_draws."""

    def __init__(self):
        import torch
        self.torch = torch
        self.objects, self.st, self.cam, self.ticks, _ = small()
        self.dw = DeviceWorld(8)
        flags = [(False, False, False)] * len(self.objects)
        self.bodies, remap, mats, matphys = self.dw._pack_bodies(self.objects, flags, [True] * len(self.objects), True, "test")
        self.dw._flush_models()
        self.models = self.dw._model_dev
        dev = self.dw.device
        self.remap = torch.from_numpy(np.array(remap, np.uint8)).to(dev)
        self.matphys = torch.from_numpy(matphys.reshape(-1)).to(dev)
        self.n_materials = len(mats)

    def call(self, words, done, n=None, budget=1 << 40):
        """(bodies [runs][n], trace [runs][bytes], stats [runs][16], ticks done [runs], generators [runs][625], draws [runs][ticks])
        after one launch on `words`, [runs][625] uint32."""
        torch, dev = self.torch, self.dw.device
        runs = len(words)
        n = len(self.bodies) if n is None else n
        start = np.tile(self.bodies[:n], (runs, 1))
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)  # noqa: E731
        d_bodies = up(start) if n else None
        d_trace = torch.full((max(runs * self.ticks * n * nat.BODY_SAMPLE_BYTES, 8),), 0xAB, dtype=torch.uint8, device=dev)
        d_done = torch.tensor(done, dtype=torch.int32, device=dev)
        d_rng = up(np.asarray(words, np.uint32))
        d_draws = torch.full((runs * self.ticks,), 77, dtype=torch.int64, device=dev)
        stats = torch.full((runs * nat.NSTATS,), -1, dtype=torch.int64, device=dev)
        st = self.st
        params = nat.VrtPhysicsParams(float(st.gravity), float(st.friction), float(st.friction_air), float(st.min_velocity), float(st.max_velocity))
        rp = nat.VrtPhysicsRunParams((C.c_double * 3)(*self.cam.tuple()), (C.c_double * 3)(0.0, 0.0, 0.0), float(st.dist_max), float(st.dist_move),
                                     budget, self.ticks, -1)
        status = nat.lib().vrt_physics_run_batch_draws(
            d_bodies.data_ptr() if n else None, runs, n, self.models.data_ptr(), self.models.numel(), self.remap.data_ptr(), self.remap.numel(),
            self.matphys.data_ptr(), self.n_materials, C.byref(params), C.byref(rp), d_done.data_ptr(), d_trace.data_ptr(), stats.data_ptr(),
            torch.cuda.current_stream().cuda_stream, d_rng.data_ptr(), d_draws.data_ptr())
        assert status == 0, status
        torch.cuda.synchronize()
        return (d_bodies.cpu().numpy().view(np.dtype(nat.BODY_FIELDS)).reshape(runs, n) if n else start,
                d_trace.cpu().numpy()[:runs * self.ticks * n * nat.BODY_SAMPLE_BYTES].reshape(runs, -1) if n else None, stats.cpu().numpy().reshape(runs, nat.NSTATS),
                d_done.cpu().numpy(), d_rng.cpu().numpy().view(np.uint32).reshape(runs, nat.RNG_WORDS), d_draws.cpu().numpy().reshape(runs, self.ticks))


@gpu
def test_the_abi_leaves_bad_runs_alone():
    """Bad device data the kernel must survive: both values are checked before anything is read or written through them."""
    abi = Abi()
    ticks = abi.ticks
    good = np.array([random.Random(s).getstate()[1] for s in (11, 12, 13)], np.uint32)
    bodies, trace, stats, done, rng, draws = abi.call(good, [0, 0, 0])
    assert done.tolist() == [ticks] * 3 and stats[:, nat.S_PHYSICS_TICKS].tolist() == [ticks] * 3 and (stats[:, nat.S_PHYSICS_DRAWS] > 0).all()
    assert np.array_equal(stats[:, nat.S_PHYSICS_DRAWS], draws.sum(axis=1)) and not (draws == 77).any() and not (trace == 0xAB).all(axis=1).any()
    assert not stats[:, [nat.S_PHYSICS_RNG_INVALID, nat.S_PHYSICS_BATCH_BADTICK]].any() and not (rng == good).all(axis=1).any()
    for k, seed in enumerate((11, 12, 13)):                     # each generator is its seed's after that run's draws
        g = random.Random(seed)
        for _ in range(int(draws[k].sum())):
            g.random()
        assert np.array_equal(rng[k], rd.state_words(g)), k
    # run 1's index word is 625 (and 2^32 - 1): runs 0 and 2 are as in the batch without the defect, run 1 is untouched and says so
    for index in (625, 0xFFFFFFFF):
        bad = good.copy()
        bad[1, 624] = index
        b2, t2, s2, d2, r2, w2 = abi.call(bad, [0, 0, 0])
        for k in (0, 2):
            assert b2[k].tobytes() == bodies[k].tobytes() and np.array_equal(t2[k], trace[k]) and np.array_equal(s2[k], stats[k]), k
            assert np.array_equal(r2[k], rng[k]) and np.array_equal(w2[k], draws[k]) and d2[k] == ticks, k
        assert b2[1].tobytes() == abi.bodies.tobytes() and (t2[1] == 0xAB).all() and np.array_equal(r2[1], bad[1])
        assert (w2[1] == 77).all() and d2[1] == 0
        assert s2[1][nat.S_PHYSICS_RNG_INVALID] == 1 and not np.delete(s2[1], nat.S_PHYSICS_RNG_INVALID).any()
    # d_ticks_done out of range: BADTICK, checked before the generator is looked at (its index word is bad as well); a run that
    # is done touches nothing, not its generator either, whatever its index word
    bad = good.copy()
    bad[1, 624] = bad[2, 624] = 999
    b2, t2, s2, d2, r2, w2 = abi.call(bad, [0, ticks + 1, ticks])
    assert d2.tolist() == [ticks, ticks + 1, ticks] and s2[:, nat.S_PHYSICS_BATCH_BADTICK].tolist() == [0, 1, 0]
    assert not s2[:, nat.S_PHYSICS_RNG_INVALID].any() and s2[:, nat.S_PHYSICS_TICKS].tolist() == [ticks, 0, 0]
    assert b2[0].tobytes() == bodies[0].tobytes() and np.array_equal(r2[0], rng[0]) and np.array_equal(s2[0], stats[0])
    for k in (1, 2):
        assert b2[k].tobytes() == abi.bodies.tobytes() and (t2[k] == 0xAB).all() and np.array_equal(r2[k], bad[k]) and (w2[k] == 77).all(), k
        assert not np.delete(s2[k], nat.S_PHYSICS_BATCH_BADTICK).any(), k
    b2, t2, s2, d2, r2, w2 = abi.call(good, [-1, 0, 0])
    assert s2[:, nat.S_PHYSICS_BATCH_BADTICK].tolist() == [1, 0, 0] and d2.tolist() == [-1, ticks, ticks] and np.array_equal(r2[0], good[0])
    # no bodies: every tick is done, none drew, the generators are untouched
    _, _, s2, d2, r2, w2 = abi.call(good, [0, 3, ticks], n=0)
    assert d2.tolist() == [ticks] * 3 and s2[:, nat.S_PHYSICS_TICKS].tolist() == [ticks, ticks - 3, 0]
    assert not np.delete(s2, nat.S_PHYSICS_TICKS, axis=1).any() and np.array_equal(r2, good)
    assert not w2[0].any() and (w2[1][:3] == 77).all() and not w2[1][3:].any() and (w2[2] == 77).all()
    # a launch that ends after one tick writes that tick's row, its draw count and the generator it stopped at; the next goes on
    b2, t2, s2, d2, r2, w2 = abi.call(good, [0, 0, 0], budget=1)
    row = len(abi.bodies) * nat.BODY_SAMPLE_BYTES
    assert d2.tolist() == [1, 1, 1] and np.array_equal(t2[:, :row], trace[:, :row]) and (t2[:, row:] == 0xAB).all()
    assert np.array_equal(w2[:, 0], draws[:, 0]) and (w2[:, 1:] == 77).all() and np.array_equal(s2[:, nat.S_PHYSICS_DRAWS], draws[:, 0])
    # DeviceWorld.run_many turns an index out of range into VrtError and touches nothing of the caller's

    class Broken(random.Random):
        def getstate(self):
            version, state, gauss = super().getstate()
            return version, state[:-1] + (625,), gauss
    gens = [random.Random(1), Broken(2)]
    before, states = ps.state(abi.objects), [random.Random.getstate(g) for g in gens]
    with pytest.raises(nat.VrtError, match="index"):
        abi.dw.run_many(abi.objects, abi.cam, abi.st, ticks, [{}, {}], rng=gens)
    assert unchanged(before, abi.objects) and [random.Random.getstate(g) for g in gens] == states


# ---- 7. what stays as it was, and apply() ------------------------------------------------------------------------------------
@gpu
def test_apply_commits_the_variant_and_its_generator():
    objects, st, cam, who, ticks, chunk = scene("wade")
    changes = bu.changes(objects, cam.tuple())
    gens = six_generators(55)
    entry, before = ps.state(objects), [g.getstate() for g in gens]
    dw = DeviceWorld(chunk)
    r = dw.run_many(objects, cam, st, ticks, [bu.mapping(objects, c) for c in changes], follow=who, rng=gens)
    assert r.trace is None and unchanged(entry, objects) and [g.getstate() for g in gens] == before      # nothing yet
    k = 5                                                      # the wader thrown down, the sleeper moved: position, velocity, draws
    twin, g = bu.altered(objects, changes[k]), copy_of(gens[k])
    t = dw.run(twin, cam, st, ticks, follow=twin[objects.index(who)], rng=g)
    moved = r.apply(k, objects, rng=gens[k])
    assert same_state(objects, twin) and gens[k].getstate() == g.getstate() != before[k]
    assert [objects.index(o) for o in moved] == [twin.index(o) for o in t.moved] and moved
    assert np.array_equal(ru.bits(who.cam_pos.tuple()), ru.bits(twin[objects.index(who)].cam_pos.tuple()))
    assert [o.redraw for o in objects] == [o.redraw for o in twin]
    assert [g.getstate() for i, g in enumerate(gens) if i != k] == [s for i, s in enumerate(before) if i != k]
    # without rng= a fractional solidity still raises, and anything that is no generator is a TypeError
    fresh, *_ = scene("wade")
    with pytest.raises(ValueError, match="fractional solidity"):
        dw.run_many(fresh, cam, st, 2, [{}, {}], follow=fresh[objects.index(who)])
    for bad in (5, gens[0].random, [gens[0], 5]):
        with pytest.raises(TypeError, match="rng"):
            dw.run_many(fresh, cam, st, 2, [{}, {}], follow=fresh[objects.index(who)], rng=bad)
    with pytest.raises(ValueError, match="generators"):
        dw.run_many(fresh, cam, st, 2, [{}, {}], follow=fresh[objects.index(who)], rng=gens[:3])
