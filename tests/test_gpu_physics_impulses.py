"""Scripted accelerations in device runs (DeviceWorld.run(impulses=), DeviceWorld.run_many(impulses=) and the "impulses" key of
a variant, vrt_physics_run_batch_impulses): the device's run bit for bit the host's (world.run(impulses=)), through
tests/golden/physics_impulses.npz the real reference's, and the loop of today's DeviceWorld.run() calls with Object.accelerate
between them, which uses none of the new code; a batch whose variants act at different ticks against its twins, with a contact
log and without; one tick per launch; more than 1024 entries before one tick; device data gone bad, through the C ABI; and a sum
that leaves the limits."""
import ctypes as C
import random

import numpy as np
import pytest

import physics_batch_util as bu
import physics_contacts_util as cu
import physics_impulse_scenes as sc
import physics_impulses_util as iu
import physics_scenes as ps
from python_raytracer_amd import _native as nat
from python_raytracer_amd import world
from python_raytracer_amd.lib import vec3
from python_raytracer_amd.world import Contacts, DeviceWorld

gpu = pytest.mark.gpu
VOXELS = Contacts(cu.ALL, "voxels")
COUNTED = [nat.S_PHYSICS_TICKS] + list(range(nat.S_PHYSICS_BODIES, nat.S_PHYSICS_DRAWS + 1))   # every word but WORK and the new two


def device_runner(dw):
    def runner(objects, cam, st, ticks, follow, gen, impulses):
        r = dw.run(objects, cam, st, ticks, follow=follow, trace=True, rng=gen, impulses=impulses)
        assert r.ticks_run == ticks and r.impulses_applied == len(impulses) and r.impulses_skipped == 0
        return r.trace, r.draws_per_tick, (r.stats.copy(), [objects.index(o) for o in r.moved], gen.getstate() if gen else None)
    return runner


def device_plain(dw):
    def plain(objects, cam, st, ticks, follow, gen):
        r = dw.run(objects, cam, st, ticks, follow=follow, trace=True, rng=gen)                  # today's call: no new code
        assert r.impulses_applied is None and r.impulses_skipped is None
        return r.trace, r.draws_per_tick, r.stats.copy()
    return plain


# ---- 1. device = host = reference = the loop it replaces ---------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("key", iu.RUNS)
def test_device_run_is_the_hosts_the_references_and_the_segment_loops(key):
    objects, states, draws, extras = iu.play(key, device_runner(DeviceWorld(8)))
    iu.assert_is_fixture(key, states, draws)                                                    # the reference, draws per tick too
    host, host_states, host_draws, _ = iu.play(key, iu.host_runner)
    assert iu.same_records(states, host_states) and iu.same_state(objects, host)               # the host: records, trace, objects
    assert draws is None or int(draws.sum()) == int(host_draws.sum())
    # the loop of DeviceWorld.run() calls with accelerate between them, on a twin world
    twins, loop_states, loop_draws, loop_extras = iu.play(key, iu.by_hand(device_plain(DeviceWorld(8))))
    assert iu.same_records(states, loop_states) and iu.same_state(objects, twins)
    assert draws is None or np.array_equal(draws, loop_draws)
    for (stats, moved, state), parts in zip(extras, loop_extras):
        assert np.array_equal(stats[COUNTED], np.sum(parts, axis=0)[COUNTED]), (key, stats, parts)
        assert stats[nat.S_PHYSICS_WORK] >= np.sum(parts, axis=0)[nat.S_PHYSICS_WORK]
    if draws is not None:
        # the generator handed back is where the host's run leaves its own
        spec, mine, st, follow, gen = iu.fresh(key)
        world.run(mine, vec3(*spec["cam"]), st, spec["ticks"], rng=gen.random, impulses=sc.impulses_of(spec, mine))
        assert extras[-1][2] == gen.getstate() and int(draws.sum()) > 0


# ---- 2. a batch whose variants act at different ticks ------------------------------------------------------------------------
def run_batch(dw, trace=True, **more):
    spec, objects, st, cam, variants, shared = iu.jump_batch()
    r = dw.run_many(objects, cam, st, spec["ticks"], [iu.variant_mapping(objects, v) for v in variants], trace=trace,
                    impulses=[(t, objects[k], vel) for t, k, vel in shared], **more)
    return spec, objects, st, cam, variants, shared, r


def own_entries(variants, shared):
    return [len(shared) + sum(len(c.get("impulses", ())) for c in v.values()) for v in variants]


@gpu
def test_every_variant_is_the_run_of_its_twin():
    dw = DeviceWorld(8)
    spec, objects, st, cam, variants, shared, r = run_batch(dw)
    ticks = spec["ticks"]
    entry = ps.state(objects)
    assert r.ticks_run.tolist() == [ticks] * 8
    assert r.impulses_applied.tolist() == own_entries(variants, shared) and not r.impulses_skipped.any()
    assert r.impulses_applied.dtype == np.uint64 and min(r.impulses_applied) == len(shared) and max(r.impulses_applied) == len(shared) + ticks
    finals = []
    for k, change in enumerate(variants):
        twin, impulses = iu.variant_twin(objects, change, shared)
        t = dw.run(twin, cam, st, ticks, trace=True, impulses=impulses)
        host_twin, host_impulses = iu.variant_twin(objects, change, shared)
        _, host_states = world.run(host_twin, cam, st, ticks, trace=True, impulses=host_impulses)
        assert iu.same_records(r.records[k], t.records) and iu.same_records(r.trace[k], t.trace), k
        assert iu.same_records(r.trace[k], host_states) and np.array_equal(r.stats[k], t.stats), k
        applied = bu.twins(objects)
        r.apply(k, applied)                                                                     # write-back needs nothing new
        assert iu.same_state(applied, twin) and iu.same_state(applied, host_twin), k
        finals.append(r.trace[k][-1].tobytes())
    assert len(set(finals)) == 8
    assert all(entry[f].tobytes() == ps.state(objects)[f].tobytes() for f in entry)           # nothing is written until apply()


@gpu
@pytest.mark.parametrize("mode", ["voxels", "pairs_of"])
def test_the_contact_log_of_every_variant_is_the_hosts(mode):
    dw = DeviceWorld(8)
    spec, objects, st, cam, variants, shared = iu.jump_batch()
    ticks = spec["ticks"]
    request = (lambda group: VOXELS) if mode == "voxels" else (lambda group: Contacts(cu.ALL, "pairs", of=[group[1]]))
    mappings, listed = [iu.variant_mapping(objects, v) for v in variants], [(t, objects[k], vel) for t, k, vel in shared]
    r = dw.run_many(objects, cam, st, ticks, mappings, trace=True, impulses=listed, contacts=request(objects))
    plain = dw.run_many(objects, cam, st, ticks, mappings, trace=True, impulses=listed)          # (the same sprites: the same models)
    assert iu.same_records(r.records, plain.records) and iu.same_records(r.trace, plain.trace) and np.array_equal(r.stats, plain.stats)
    totals = []
    for k, change in enumerate(variants):
        twin, impulses = iu.variant_twin(objects, change, shared)
        *_, want = world.run(twin, cam, st, ticks, impulses=impulses, contacts=request(twin))
        assert cu.same_log(r.contacts(k), want), k                                              # record for record
        totals.append(want.total)
    assert min(totals) > 0 and len(set(totals)) >= 3


@gpu
def test_an_empty_list_is_todays_batch_byte_for_byte(monkeypatch):
    L = nat.lib()
    called = []
    for name in ("vrt_physics_run_batch", "vrt_physics_run_batch_draws", "vrt_physics_run_batch_contacts", "vrt_physics_run_batch_impulses"):
        def spy(name=name, real=getattr(L, name)):
            def call(*args):
                called.append(name)
                return real(*args)
            monkeypatch.setattr(L, name, call)
        spy()
    spec, objects, st, cam, variants, shared = iu.jump_batch()
    plain_variants = [{k: {key: v for key, v in c.items() if key != "impulses"} for k, c in v.items()} for v in variants]
    variants = [bu.mapping(objects, v) for v in plain_variants]
    dw, ticks = DeviceWorld(8), spec["ticks"]
    for more in ({}, dict(contacts=VOXELS)):
        del called[:]
        today = dw.run_many(objects, cam, st, ticks, variants, trace=True, **more)
        # a call without impulses= launches exactly what it launched
        assert called == ["vrt_physics_run_batch_contacts" if more else "vrt_physics_run_batch"] * today.launches
        assert today.impulses_applied is None and today.impulses_skipped is None
        del called[:]
        r = dw.run_many(objects, cam, st, ticks, variants, trace=True, impulses=[], **more)
        assert called == ["vrt_physics_run_batch_impulses"] * r.launches
        assert iu.same_records(r.records, today.records) and iu.same_records(r.trace, today.trace)
        assert np.array_equal(r.stats, today.stats) and r.launches == today.launches and r.ticks_run.tolist() == today.ticks_run.tolist()
        assert not r.impulses_applied.any() and not r.impulses_skipped.any()
        if more:
            assert all(cu.same_log(r.contacts(k), today.contacts(k)) for k in range(8)) and np.array_equal(r.contacts_total, today.contacts_total)
    # ... and with draws: the seeded fluid scene, the log kept and not kept
    spec, objects, st, _, gen = iu.fresh("wade_thrust")
    cam = vec3(*spec["cam"])
    for more in ({}, dict(contacts=VOXELS)):
        del called[:]
        today = dw.run_many(objects, cam, st, 6, [{}, {}], trace=True, rng=[gen, random.Random(3)], **more)
        assert called == ["vrt_physics_run_batch_contacts" if more else "vrt_physics_run_batch_draws"] * today.launches
        r = dw.run_many(objects, cam, st, 6, [{}, {}], trace=True, rng=[gen, random.Random(3)], impulses=[], **more)
        assert iu.same_records(r.records, today.records) and iu.same_records(r.trace, today.trace) and np.array_equal(r.stats, today.stats)
        assert np.array_equal(r.draws_per_tick, today.draws_per_tick) and r.draws.min() > 0 and r.launches == today.launches
        assert all(r.rng_state(k) == today.rng_state(k) for k in range(2))
        if more:
            assert all(cu.same_log(r.contacts(k), today.contacts(k)) for k in range(2))
    # DeviceWorld.run without impulses= is the call it was
    del called[:]
    one = dw.run(bu.twins(iu.fresh("jump")[1]), vec3(0, 0, 0), iu.fresh("jump")[2], 3)
    assert "vrt_physics_run_batch_impulses" not in called and one.impulses_applied is None


# ---- 3. chaining: one tick per launch ------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("logged", [False, True])
def test_one_tick_per_launch_gives_the_same_batch(logged):
    dw = DeviceWorld(8)
    more = dict(contacts=VOXELS) if logged else {}
    spec, objects, st, cam, variants, shared = iu.jump_batch()
    ticks = spec["ticks"]
    mappings, listed = [iu.variant_mapping(objects, v) for v in variants], [(t, objects[k], vel) for t, k, vel in shared]
    whole = dw.run_many(objects, cam, st, ticks, mappings, trace=True, impulses=listed, **more)
    r = dw.run_many(objects, cam, st, ticks, mappings, trace=True, impulses=listed, budget=1, **more)
    assert r.launches == ticks and whole.launches == 1 and r.ticks_run.tolist() == [ticks] * 8
    assert iu.same_records(r.records, whole.records) and iu.same_records(r.trace, whole.trace)
    assert np.array_equal(r.stats, whole.stats)                                                 # the sums over the chain, WORK included
    assert r.impulses_applied.tolist() == own_entries(variants, shared) and not r.impulses_skipped.any()
    if logged:
        assert all(cu.same_log(r.contacts(k), whole.contacts(k)) for k in range(8))
    # ... and with draws: every thrust tick is the first tick of a launch
    spec, objects, st, _, gen = iu.fresh("wade_thrust")
    shared = sc.impulses_of(spec, objects)
    a = dw.run_many(objects, vec3(*spec["cam"]), st, spec["ticks"], [{}], trace=True, rng=gen, impulses=shared, **more)
    b = dw.run_many(objects, vec3(*spec["cam"]), st, spec["ticks"], [{}], trace=True, rng=gen, impulses=shared, budget=1, **more)
    assert b.launches == spec["ticks"] and iu.same_records(a.trace, b.trace) and np.array_equal(a.draws_per_tick, b.draws_per_tick)
    assert a.rng_state(0) == b.rng_state(0) and np.array_equal(a.stats, b.stats) and int(a.impulses_applied[0]) == len(shared)
    iu.assert_is_fixture("wade_thrust", b.trace[0], b.draws_per_tick[0])


# ---- 4. more than 1024 entries before one tick ---------------------------------------------------------------------------------
AWAKE = (0, 1023, 1029)
CROWD_N = 1030


def crowd():
    """1030 bodies of 2^3, no gravity, no air friction, no minimum velocity, each with velocity 2^-53 along x; all but three stand
    beyond dist_move.  Before tick 1 every body gets one impulse; bodies 0, 1022 (asleep: its two entries lie on both sides of
    the 1024th of the tick), 1023 and 1029 get two, in an order that shows: from 2^-53, + 2^-53 + 1.0 is 1 + 2^-52 and
    + 1.0 + 2^-53 is 1.0."""
    p = sc.P53
    objects = [ps.obj("dot", (100 + 6 * (i % 34), 0, 6 * (i // 34)), vel=(p, 0, 0)) for i in range(CROWD_N)]
    for at, i in enumerate(AWAKE):
        objects[i] = ps.obj("dot", (0, 8 * at, 0), vel=(p, 0, 0))
    spec = ps.scene({"dot": ps.full((2, 2, 2), 1)}, objects, 3, gravity=0.0, friction_air=0.0, min_velocity=0.0, dist_move=32, dist_max=1024)
    built, _, _, st = ps.project_scene(spec)
    ps.clear_redraw(built)
    first = {0: (p, 1.0), 1022: (p, 1.0), 1023: (1.0, p), 1029: (p, 1.0)}

    def impulses(group):
        out = []
        for i in range(CROWD_N):
            out += [(1, group[i], (x, 0.0, 0.0)) for x in first.get(i, (0.5,))]
        return out
    return spec, built, st, impulses


@gpu
def test_more_than_1024_entries_before_one_tick():
    spec, objects, st, impulses = crowd()
    twins = bu.twins(objects)
    cam = vec3(*spec["cam"])
    r = DeviceWorld(8).run(objects, cam, st, 3, trace=True, impulses=impulses(objects))
    _, states = world.run(twins, cam, st, 3, trace=True, impulses=impulses(twins))
    assert r.impulses_applied == CROWD_N + 4 and r.impulses_skipped == 0
    assert iu.same_records(r.trace, states) and iu.same_state(objects, twins)
    vel = r.trace["vel"][:, :, 0]
    assert vel[1, 0] == vel[1, 1029] == vel[1, 1022] == 1.0 + 2.0 ** -52 and vel[1, 1023] == 1.0          # the order shows
    asleep = np.setdiff1d(np.arange(CROWD_N), AWAKE + (1022,))
    assert (vel[0] == sc.P53).all() and (vel[1:, asleep] == 0.5 + sc.P53).all()                            # 2^-53 + 0.5, held
    assert (r.trace["awake"][:, asleep] == 0).all() and (r.trace["awake"][:, list(AWAKE)] != 0).all()
    assert (r.trace["pos"][2, list(AWAKE), 0] > 1.5).all() and (r.trace["pos"][:, asleep] == r.trace["pos"][0, asleep]).all()


# ---- 5. device data gone bad: through the C ABI --------------------------------------------------------------------------------
class Abi:
    """Scene `jump` as DeviceWorld.run_many packs it, for direct calls of vrt_physics_run_batch_impulses with hand-made lists."""

    def __init__(self):
        import torch
        self.torch = torch
        self.spec, self.objects, self.st, _, _ = iu.fresh("jump")
        self.dw = DeviceWorld(8)
        n = len(self.objects)
        self.bodies, remap, mats, matphys = self.dw._pack_bodies(self.objects, [(False, False, False)] * n, [True] * n, False, "test")
        self.dw._flush_models()
        self.models = self.dw._model_dev
        dev = self.dw.device
        self.remap = torch.from_numpy(np.array(remap, np.uint8)).to(dev)
        self.matphys = torch.from_numpy(matphys.reshape(-1)).to(dev)
        self.n_materials, self.ticks, self.n = len(mats), self.spec["ticks"], n

    def call(self, lists, first=None, budget=1 << 40, launches=1):
        """(status, statistics summed over the launches [runs][16], ticks done [runs], bodies [runs][n]) for the runs' lists of
        (tick, body, vel) rows, uploaded as they are: nothing is sorted or checked here.  first: d_first, if not the lists'."""
        torch, dev = self.torch, self.dw.device
        runs = len(lists)
        rows = np.array([tuple(e) for entries in lists for e in entries], np.dtype(nat.IMPULSE_FIELDS)).reshape(-1)
        bounds = np.cumsum([0] + [len(entries) for entries in lists]).astype(np.int32) if first is None else np.array(first, np.int32)
        assert len(bounds) == runs + 1
        d_rows = torch.from_numpy(rows.view(np.uint8).reshape(-1).copy()).to(dev) if len(rows) else None
        d_first = torch.from_numpy(bounds).to(dev)
        listed = nat.VrtImpulseList(d_rows.data_ptr() if d_rows is not None else None, d_first.data_ptr(), len(rows))
        d_bodies = torch.from_numpy(np.tile(self.bodies, (runs, 1)).view(np.uint8).reshape(-1).copy()).to(dev)
        d_done = torch.zeros(runs, dtype=torch.int32, device=dev)
        stats = torch.full((runs * nat.NSTATS,), -1, dtype=torch.int64, device=dev)
        total = np.zeros((runs, nat.NSTATS), np.int64)
        st = self.st
        params = nat.VrtPhysicsParams(float(st.gravity), float(st.friction), float(st.friction_air), float(st.min_velocity), float(st.max_velocity))
        rp = nat.VrtPhysicsRunParams((C.c_double * 3)(*self.spec["cam"]), (C.c_double * 3)(0.0, 0.0, 0.0), float(st.dist_max), float(st.dist_move),
                                     budget, self.ticks, -1)
        status = 0
        for _ in range(launches):
            status = nat.lib().vrt_physics_run_batch_impulses(
                d_bodies.data_ptr(), runs, self.n, self.models.data_ptr(), self.models.numel(), self.remap.data_ptr(), self.remap.numel(),
                self.matphys.data_ptr(), self.n_materials, C.byref(params), C.byref(rp), d_done.data_ptr(), None, stats.data_ptr(),
                torch.cuda.current_stream().cuda_stream, None, None, None, C.byref(listed))
            torch.cuda.synchronize()
            if status != 0:
                break
            total += stats.cpu().numpy().reshape(runs, nat.NSTATS)
        return status, total, d_done.cpu().numpy(), d_bodies.cpu().numpy().view(np.dtype(nat.BODY_FIELDS)).reshape(runs, self.n)


def applied_by_the_rule(entries, ticks, n):
    """The entries of a run's list that include/vrt.h says are applied, in order: an entry belongs to the largest tick in
    [0, ticks) among the entries up to it, and is applied iff its tick is that tick, its body is in [0, n) and no lower than the
    body of an earlier entry of that tick that passed these tests, and its components are finite."""
    kept, tick, body = [], -1, -1
    for t, b, vel in entries:
        if 0 <= t < ticks and t > tick:
            tick, body = t, -1
        if 0 <= t == tick and 0 <= b < n and b >= body:
            body = b
            if all(np.isfinite(vel)):
                kept.append((t, b, vel))
    return kept


@gpu
def test_bad_device_data_is_counted_and_never_applied():
    iu.assert_refusals(nat.lib())                      # VRT_ERR_ARG before any HIP call, with a device present as without
    abi = Abi()
    ticks, n = abi.ticks, abi.n
    nan = float("nan")
    jump, push, late = (3, 1, (0.75, 6.0, 0.0)), (5, 1, (0.5, 0.0, 0.25)), (8, 1, (0.0, 3.0, 0.0))
    good_a, good_b = [(1, 1, (0.0, 4.0, 0.0)), push], [(3, 0, (1.0, 0.0, 0.0)), jump, late]      # (sorted by tick, then body, as the host sorts)
    status, alone, done, want = abi.call([good_a, good_b])
    assert status == 0 and done.tolist() == [ticks] * 2 and alone[:, nat.S_PHYSICS_IMPULSES].tolist() == [2, 3]
    assert not alone[:, nat.S_PHYSICS_IMPULSES_BAD].any() and want[0].tobytes() != want[1].tobytes()
    # each bad list, the entries of it that are applied all the same, and how many are skipped
    cases = {"a body of -1 and one of n": ([jump, (3, -1, (9.0, 9.0, 9.0)), (3, n, (9.0, 9.0, 9.0)), push], [jump, push], 2),
             "ticks out of order": ([push, jump, (4, 1, (9.0, 0.0, 0.0)), late], [push, late], 2),
             "a tick of n_ticks, and a negative one": ([jump, (ticks, 1, (9.0, 9.0, 9.0)), (-1, 0, (9.0, 9.0, 9.0)), push], [jump, push], 2),
             "a NaN component": ([(3, 1, (0.75, nan, 0.0)), jump, (3, 1, (float("inf"), 0.0, 0.0)), push], [jump, push], 2),
             "bodies out of order within a tick": ([jump, (3, 0, (9.0, 0.0, 0.0)), (3, 1, (0.25, 0.0, 0.0)), push],
                                                   [jump, (3, 1, (0.25, 0.0, 0.0)), push], 1)}
    for what, (bad, kept, skipped) in cases.items():
        assert applied_by_the_rule(bad, ticks, n) == kept and len(bad) - len(kept) == skipped, what
        status, stats, done, got = abi.call([good_a, bad, good_b])
        assert status == 0 and done.tolist() == [ticks] * 3, what
        assert stats[1][nat.S_PHYSICS_IMPULSES] == len(kept) and stats[1][nat.S_PHYSICS_IMPULSES_BAD] == skipped, (what, stats[1])
        assert got[0].tobytes() == want[0].tobytes() and got[2].tobytes() == want[1].tobytes(), what     # the good runs beside it
        assert np.array_equal(stats[[0, 2]], alone), what
        _, _, _, only = abi.call([kept])
        assert got[1].tobytes() == only[0].tobytes(), what                                               # ... never applied
        # one tick per launch: the same entries are skipped, once each
        status, chained, done, again = abi.call([good_a, bad, good_b], budget=1, launches=ticks)
        assert status == 0 and done.tolist() == [ticks] * 3 and again.tobytes() == got.tobytes(), what
        assert np.array_equal(chained[:, :2], stats[:, :2]), (what, chained[:, :2])
    # a d_first row that decreases, is negative or passes `total`: that run's list is empty, and it says so once.  The rows
    # beside it read what their own bounds say (which here overlaps other runs' entries): the rule of the header, written out
    _, _, _, none = abi.call([[]])
    lists = [good_a, [jump, push], good_b[:1]]
    flat = [e for entries in lists for e in entries]
    for first in ([0, 4, 2, 5], [0, 2, 9, 5], [0, 2, -1, 5]):
        status, stats, done, got = abi.call(lists, first=first)
        assert status == 0 and done.tolist() == [ticks] * 3, first
        bad_rows = [r for r in range(3) if not 0 <= first[r] <= first[r + 1] <= len(flat)]
        assert len(bad_rows) >= 1
        for r in range(3):
            if r in bad_rows:
                assert stats[r][:2].tolist() == [0, 1] and got[r].tobytes() == none[0].tobytes(), (first, r)
                continue
            mine = flat[first[r]:first[r + 1]]
            kept = applied_by_the_rule(mine, ticks, n)
            assert stats[r][:2].tolist() == [len(kept), len(mine) - len(kept)], (first, r, stats[r][:2])
            assert got[r].tobytes() == abi.call([kept])[3][0].tobytes(), (first, r)
    assert first == [0, 2, -1, 5] and got[0].tobytes() == want[0].tobytes()                  # (row 0 is good_a, untouched)
    status, chained, done, again = abi.call(lists, first=[0, 4, 2, 5], budget=1, launches=ticks)
    status, stats, done, got = abi.call(lists, first=[0, 4, 2, 5])
    assert status == 0 and done.tolist() == [ticks] * 3 and np.array_equal(chained[:, :2], stats[:, :2]) and chained[1][:2].tolist() == [0, 1]
    assert again.tobytes() == got.tobytes()


# ---- 6. a sum that leaves the limits -------------------------------------------------------------------------------------------
@gpu
def test_an_impulse_past_the_limit_is_refused_by_the_tick_in_that_run_only():
    dw = DeviceWorld(8)
    spec, objects, st, cam, variants, shared = iu.jump_batch()
    ticks = spec["ticks"]
    mappings = [iu.variant_mapping(objects, v) for v in variants]
    listed = [(t, objects[k], vel) for t, k, vel in shared]
    without = dw.run_many(objects, cam, st, ticks, mappings, trace=True, impulses=listed)
    over = {objects[1]: dict(impulses=[(4, (0.0, 1000.0, 0.0)), (4, (0.0, 30.0, 0.0))])}            # 1030 > 1024 from tick 4 on
    r = dw.run_many(objects, cam, st, ticks, mappings[:3] + [over] + mappings[3:], trace=True, impulses=listed)
    others = [0, 1, 2, 4, 5, 6, 7, 8]
    assert iu.same_records(r.records[others], without.records) and iu.same_records(r.trace[others], without.trace)
    assert np.array_equal(r.stats[others], without.stats)
    status = r.trace[3]["status"][:, 1]
    assert (status[4:] == nat.BODY_REFUSED).all() and (status[:4] != nat.BODY_REFUSED).all()
    assert (r.trace[3]["status"][:, 0] != nat.BODY_REFUSED).all()                                    # the slab of that run goes on
    assert int(r.impulses_applied[3]) == len(shared) + 2 and int(r.stats[3][nat.S_PHYSICS_REFUSED]) == ticks - 4
    pos = r.trace[3]["pos"][:, 1]
    assert (pos[4:] == pos[3]).all() and r.trace[3]["vel"][-1, 1, 1] > 1024                          # it keeps the velocity, and stands
    # ValueErrors of the device path
    with pytest.raises(ValueError, match="clock"):
        dw.run(bu.twins(objects), cam, st, 2, clock=(0, 10), impulses=[])
    with pytest.raises(ValueError, match="not one of"):
        dw.run(objects, cam, st, 2, impulses=[(0, world.Object(), (0, 1, 0))])
    with pytest.raises(ValueError):
        dw.run_many(objects, cam, st, 2, [{objects[1]: dict(impulses=[(2, (0, 1, 0))])}])
    with pytest.raises(ValueError):
        dw.run_many(objects, cam, st, 2, [{}], impulses=[(0, objects[1], (0, float("nan"), 0))])
