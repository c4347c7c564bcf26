"""The contact log of device runs (DeviceWorld.run(contacts=), DeviceWorld.run_many(contacts=), vrt_physics_run_batch_contacts):
the device's log byte for byte the host's (world.run(contacts=)) and through tests/golden/physics_contacts.npz the real
reference's, with everything else in the result as the same call without contacts= gives it; a batch against its twins; the
drawing instance with one generator and with K; bodies at and past index 1024 and a met body whose slab takes three passes, in
PAIRS mode; the capacity and chained launches; the mask; and the entry point through ctypes."""
import ctypes as C
import random

import numpy as np
import pytest

import physics_batch_util as bu
import physics_contacts_util as cu
import physics_run_util as ru
import physics_scenes as ps
from python_raytracer_amd import _native as nat
from python_raytracer_amd import world
from python_raytracer_amd.lib import vec3
from python_raytracer_amd.world import Contacts, DeviceWorld

gpu = pytest.mark.gpu
VOXELS = Contacts(cu.ALL, "voxels")


def copy_of(g):
    c = random.Random()
    c.setstate(g.getstate())
    return c


def same_result(a, b):
    """Two RunResults agree in everything but the log: records, trace, statistics, ticks, launches, counters, draws."""
    assert ru.same_records(a.records, b.records) and ru.same_records(a.trace, b.trace)
    assert np.array_equal(a.stats, b.stats), (a.stats, b.stats)
    assert (a.ticks_run, a.launches) == (b.ticks_run, b.launches) and ru.same_records(a.counters, b.counters)
    assert a.draws == b.draws and (a.draws_per_tick is None) == (b.draws_per_tick is None)
    assert a.draws_per_tick is None or np.array_equal(a.draws_per_tick, b.draws_per_tick)
    assert a.frames is None and b.frames is None and a.anim is None and b.anim is None
    return True


def same_state(a, b):
    sa, sb = ps.state(a), ps.state(b)
    return all(sa[f].tobytes() == sb[f].tobytes() for f in sa)


def tiny():
    """Scene `tiny` (2 bodies, 10 ticks), its settings and camera, and eight distinct variants of it (tests/test_gpu_physics_batch.py)."""
    spec, objects, _, st, cam, _ = cu.fresh("edges_tiny")
    eight = [{}, {1: dict(vel=(0.5, 0, 0))}, {1: dict(vel=(0, -3.25, 0.5))}, {1: dict(pos=(3, 7.5, -2))}, {1: dict(pos=(40, 5, 0))},
             {1: dict(pos=(-1, 9, 1), vel=(0.25, 1, 0))}, {0: dict(pos=(0, -2, 0))}, {0: dict(pos=(1, 0, 0)), 1: dict(vel=(-2, 0, 0))}]
    return spec, objects, st, cam, eight


# ---- 1. device = host = reference --------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", ["edges_tiny", "edges_rot", "pile", "default"])
def test_device_log_is_the_hosts_and_the_references(name):
    spec, objects, mats, st, cam, _ = cu.fresh(name)
    ticks = spec["ticks"]
    r = DeviceWorld(16).run(objects, cam, st, ticks, trace=True, contacts=VOXELS)
    host = cu.host(name)
    log = r.contacts
    assert log.total == host[6].total > 0 and log.lost == 0 and log.records.dtype == host[6].records.dtype
    assert log.records.tobytes() == host[6].records.tobytes() and cu.same_log(log, host[6]), name    # the ids too: bytes
    want, _ = cu.fixture()[name]
    assert cu.in_scene_materials(log, mats).tobytes() == want.tobytes(), name                        # ... and the reference's
    assert same_state(objects, host[1])
    # everything else is the run without a log
    _, plain, _, _, _, _ = cu.fresh(name)
    p = DeviceWorld(16).run(plain, cam, st, ticks, trace=True)
    assert same_result(r, p) and p.contacts is None and same_state(objects, plain)
    assert [objects.index(o) for o in r.moved] == [plain.index(o) for o in p.moved]
    assert int(r.stats[nat.S_PHYSICS_CONTACTS]) == log.total


# ---- 2. a batch --------------------------------------------------------------------------------------------------------------
@gpu
def test_every_variants_log_is_the_log_of_its_twin():
    spec, objects, st, cam, eight = tiny()
    ticks = spec["ticks"]
    entry = ps.state(objects)
    variants = [bu.mapping(objects, c) for c in eight]
    r = DeviceWorld(8).run_many(objects, cam, st, ticks, variants, trace=True, contacts=VOXELS)
    plain = DeviceWorld(8).run_many(objects, cam, st, ticks, variants, trace=True)
    host = world.run_many(objects, cam, st, ticks, variants, trace=True, contacts=VOXELS)
    assert all(entry[f].tobytes() == ps.state(objects)[f].tobytes() for f in entry)                 # nothing is written until apply()
    assert ru.same_records(r.records, plain.records) and ru.same_records(r.trace, plain.trace) and np.array_equal(r.stats, plain.stats)
    assert r.ticks_run.tolist() == plain.ticks_run.tolist() == [ticks] * 8 and r.launches == plain.launches
    assert plain.contacts(0) is None and plain.contacts_total is None and plain.contacts_lost is None
    assert r.contacts_total.dtype == np.uint64 and r.contacts_total.shape == (8,) and not r.contacts_lost.any()
    dw = DeviceWorld(8)
    logs = []
    for k, change in enumerate(eight):
        twin = bu.altered(objects, change)
        t = dw.run(twin, cam, st, ticks, trace=True, contacts=VOXELS)
        mine = r.contacts(k)
        assert cu.same_log(mine, t.contacts) and cu.same_log(mine, host[k][3]), k
        assert int(r.contacts_total[k]) == mine.total == int(r.stats[k][nat.S_PHYSICS_CONTACTS]), k
        assert ru.same_records(r.records[k], t.records) and ru.same_records(r.trace[k], t.trace) and ru.same_records(r.trace[k], host[k][2]), k
        logs.append(mine.records.tobytes())
    assert len(set(logs)) >= 3 and b"" in logs and cu.same_log(r.contacts(0), cu.host("edges_tiny")[6])   # the scene has not gone quiet
    # apply() is unchanged
    a, b = bu.twins(objects), bu.twins(objects)
    r.apply(1, a), plain.apply(1, b)
    assert same_state(a, b)


# ---- 3. the drawing instance -------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("generators", ["one", "three"])
def test_with_draws_every_variants_log_is_the_hosts(generators):
    spec, objects, mats, st, cam, gen = cu.fresh("fluid")
    ticks = 12
    changes = [{}, {1: dict(vel=(0.5, -1.0, 0))}, {2: dict(pos=(-8, 9, 3))}]
    variants = [bu.mapping(objects, c) for c in changes]
    gens = gen if generators == "one" else [gen, random.Random(7), random.Random(8)]
    each = [gen] * 3 if generators == "one" else gens
    before = [g.getstate() for g in each]
    r = DeviceWorld(16).run_many(objects, cam, st, ticks, variants, trace=True, rng=gens, contacts=VOXELS)
    plain = DeviceWorld(16).run_many(objects, cam, st, ticks, variants, trace=True, rng=gens)
    assert [g.getstate() for g in each] == before
    assert ru.same_records(r.records, plain.records) and ru.same_records(r.trace, plain.trace) and np.array_equal(r.stats, plain.stats)
    assert np.array_equal(r.draws, plain.draws) and np.array_equal(r.draws_per_tick, plain.draws_per_tick) and r.launches == plain.launches
    assert r.draws.min() > 0 and not r.stats[:, nat.S_PHYSICS_RNG_INVALID].any()
    for k, change in enumerate(changes):
        assert r.rng_state(k) == plain.rng_state(k), k
        twin, g = bu.altered(objects, change), copy_of(each[k])
        *_, want = world.run(twin, cam, st, ticks, rng=g.random, contacts=VOXELS)
        assert want.total > 0 and cu.same_log(r.contacts(k), want), k
        assert r.rng_state(k) == g.getstate(), k
    assert len({r.contacts(k).records.tobytes() for k in range(3)}) == 3
    if generators == "one":
        # DeviceWorld.run(rng=, contacts=): the log, and the generator handed back where run(rng=) leaves it
        a, b, ga, gb = bu.twins(objects), bu.twins(objects), copy_of(gen), copy_of(gen)
        dw = DeviceWorld(16)
        t, p = dw.run(a, cam, st, ticks, trace=True, rng=ga, contacts=VOXELS), dw.run(b, cam, st, ticks, trace=True, rng=gb)
        assert same_result(t, p) and ga.getstate() == gb.getstate() == r.rng_state(0) and same_state(a, b)
        assert cu.same_log(t.contacts, r.contacts(0)) and t.draws > 0


# ---- 4. tile and pass borders ------------------------------------------------------------------------------------------------
@gpu
def test_bodies_at_and_past_index_1024_are_logged_as_the_host_logs_them():
    spec, objects, mats, st, cam, _ = cu.fresh("crowd")
    _, twins, _, _, _, _ = cu.fresh("crowd")
    dw = DeviceWorld(16)
    seen = []
    for first, last in ru.segments(spec):
        for group in (objects, twins):
            ps.clear_redraw(group)
            cam = vec3(*ps.apply_script(spec, first, group, vec3, cam.tuple()))
        r = dw.run(objects, cam, st, last - first, contacts=VOXELS)
        *_, want = world.run(twins, cam, st, last - first, contacts=VOXELS)
        assert cu.same_log(r.contacts, want), first
        seen.append(r.contacts.records)
    seen = np.concatenate(seen)
    assert (seen["other"] >= 1024).any() and (seen["mover"] >= 1024).any() and (seen["other"] < 1024).any()
    # one step that meets a body on either side of the tile border: the bar on block_low and block_high
    R = ps.CROWD_ROLES
    bar = seen[seen["mover"] == R["bar"]]
    assert {R["block_low"], R["block_high"]} <= set(bar["other"].tolist())


@gpu
def test_pairs_across_passes_is_one_record_per_touch():
    """`fluid`: the raft's slab on the 40 x 34 pool is 37 x 2 x 31 = 2294 tests, three passes of 1024 with contacts in each."""
    spec, objects, mats, st, cam, gen = cu.fresh("fluid")
    r = DeviceWorld(16).run(objects, cam, st, spec["ticks"], rng=gen, contacts=Contacts(cu.ALL, "pairs"))
    want, voxels = cu.host("fluid", "pairs")[6], cu.host("fluid")[6]
    assert cu.same_log(r.contacts, want)
    rec = r.contacts.records
    keys = list(zip(rec["tick"].tolist(), rec["mover"].tolist(), rec["step"].tolist(), rec["other"].tolist()))
    assert len(set(keys)) == len(keys) == len(voxels.pairs()) > 0                        # exactly one record per touch
    # ... and some touch's contacts do span passes: more than 1024 tests lie between its first and its last
    v, raft = voxels.records, 1
    touch = v[(v["mover"] == raft) & (v["other"] == 0)]
    first = touch[(touch["tick"] == touch["tick"][0]) & (touch["step"] == touch["step"][0])]
    ext_z, ext_y = 31, 2
    flat = ((first["voxel"][:, 0] - first["voxel"][:, 0].min()) * ext_y + (first["voxel"][:, 1] - first["voxel"][:, 1].min())) * ext_z
    assert flat.max() - flat.min() > 1024
    # the same without draws, on a scene whose floor takes three passes too: `face`
    spec, objects, mats, st, cam, _ = cu.fresh("edges_face")
    _, twins, _, _, _, _ = cu.fresh("edges_face")
    for mode in ("pairs", "voxels"):
        a, b = bu.twins(objects), bu.twins(twins)
        r = DeviceWorld(16).run(a, cam, st, spec["ticks"], contacts=Contacts(cu.ALL, mode))
        *_, want = world.run(b, cam, st, spec["ticks"], contacts=Contacts(cu.ALL, mode))
        assert cu.same_log(r.contacts, want) and want.total > 0, mode
    assert want.total >= 1360 and len(want.pairs()) < 10


# ---- 5. bounded and chained --------------------------------------------------------------------------------------------------
@gpu
def test_capacity_keeps_the_prefix_and_chained_launches_continue_the_log():
    spec, objects, mats, st, cam, _ = cu.fresh("pile")
    ticks = spec["ticks"]
    full = cu.host("pile")[6]
    total = full.total
    assert total > 100
    variants = [{}, bu.mapping(objects, {3: dict(vel=(0, -2.0, 0))})]
    dw = DeviceWorld(16)
    whole = dw.run_many(objects, cam, st, ticks, variants, contacts=VOXELS)
    assert cu.same_log(whole.contacts(0), full) and whole.contacts(1).total > 0
    for capacity in (total // 2, 0):
        r = dw.run_many(objects, cam, st, ticks, variants, contacts=Contacts(capacity, "voxels"))
        assert np.array_equal(r.contacts_total, whole.contacts_total)
        assert r.contacts_lost.tolist() == [max(0, int(t) - capacity) for t in whole.contacts_total]
        for k in range(2):
            got, want = r.contacts(k), whole.contacts(k)
            assert got.total == want.total and got.lost == max(0, want.total - capacity) and len(got.records) == min(capacity, want.total)
            assert got.records.tobytes() == want.records[:capacity].tobytes(), (capacity, k)
        assert ru.same_records(r.records, whole.records)
    # one tick per launch: the log goes on where it stood
    for capacity in (cu.ALL, total // 2):
        r = dw.run_many(objects, cam, st, ticks, variants, budget=1, contacts=Contacts(capacity, "voxels"))
        assert r.launches == ticks and np.array_equal(r.contacts_total, whole.contacts_total)
        for k in range(2):
            assert r.contacts(k).records.tobytes() == whole.contacts(k).records[:capacity].tobytes(), (capacity, k)
        assert ru.same_records(r.records, whole.records) and np.array_equal(r.stats[:, nat.S_PHYSICS_WORK], whole.stats[:, nat.S_PHYSICS_WORK])
    pairs = cu.host("pile", "pairs")[6]
    one = DeviceWorld(16).run(bu.twins(objects), cam, st, ticks, budget=1, contacts=Contacts(100, "pairs"))
    assert one.launches == ticks and one.contacts.records.tobytes() == pairs.records[:100].tobytes()
    assert one.contacts.total == pairs.total > 100 and one.contacts.lost == pairs.total - 100


# ---- 6. the mask -------------------------------------------------------------------------------------------------------------
@gpu
def test_of_gives_the_hosts_filtered_log():
    spec, objects, mats, st, cam, _ = cu.fresh("pile")
    _, twins, _, _, _, _ = cu.fresh("pile")
    for who in ([3], [0], [3, 17]):
        for mode in ("voxels", "pairs"):
            a, b = bu.twins(objects), bu.twins(twins)
            r = DeviceWorld(16).run(a, cam, st, spec["ticks"], contacts=Contacts(cu.ALL, mode, of=[a[k] for k in who]))
            *_, want = world.run(b, cam, st, spec["ticks"], contacts=Contacts(cu.ALL, mode, of=[b[k] for k in who]))
            assert cu.same_log(r.contacts, want) and 0 < want.total < cu.host("pile")[6].total, (who, mode)
    with pytest.raises(ValueError, match="not one of"):
        DeviceWorld(16).run(objects, cam, st, 2, contacts=Contacts(of=[twins[3]]))
    with pytest.raises(ValueError, match="clock"):
        DeviceWorld(16).run(objects, cam, st, 2, clock=(0, 10), contacts=Contacts())
    with pytest.raises(TypeError):
        DeviceWorld(16).run_many(objects, cam, st, 2, [{}], contacts="pairs")
    with pytest.raises(ValueError, match="2\\^31"):
        DeviceWorld(16).run_many(objects, cam, st, 2, [{}] * 3, contacts=Contacts(capacity=(1 << 31) // 3 + 1))


# ---- 7. straight through the C ABI -------------------------------------------------------------------------------------------
class Abi:
    """Scene `tiny` as DeviceWorld.run_many packs it, for direct calls of vrt_physics_run_batch_contacts."""

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

    def call(self, runs, done, counts, capacity, n=None, mask=None, mode=nat.CONTACTS_VOXELS, budget=1 << 40, launches=1, rng=None):
        """(status, stats [runs][16] of the last launch, ticks done [runs], counts [runs], records [runs][capacity] as bytes) after
        `launches` launches with the same pointers; the records start as 0xAB bytes.  rng: [runs][625] generator words: the
        drawing instance; self.rng_after then holds them as the launches left them."""
        torch, dev = self.torch, self.dw.device
        n = len(self.bodies) if n is None else n
        start = np.tile(self.bodies[:n], (runs, 1))
        d_bodies = torch.from_numpy(start.view(np.uint8).reshape(-1).copy()).to(dev) if n else None
        d_done = torch.tensor(done, dtype=torch.int32, device=dev)
        stats = torch.full((runs * nat.NSTATS,), -1, dtype=torch.int64, device=dev)
        d_counts = torch.tensor(counts, dtype=torch.int64, device=dev)
        d_records = torch.full((max(runs * capacity, 1) * nat.CONTACT_BYTES,), 0xAB, dtype=torch.uint8, device=dev)
        d_mask = torch.tensor(mask, dtype=torch.uint8, device=dev) if mask is not None else None
        st = self.st
        params = nat.VrtPhysicsParams(float(st.gravity), float(st.friction), float(st.friction_air), float(st.min_velocity), float(st.max_velocity))
        rp = nat.VrtPhysicsRunParams((C.c_double * 3)(*self.spec["cam"]), (C.c_double * 3)(0.0, 0.0, 0.0), float(st.dist_max), float(st.dist_move),
                                     budget, self.ticks, -1)
        log = nat.VrtContactLog(d_records.data_ptr(), d_counts.data_ptr(), d_mask.data_ptr() if d_mask is not None else None, capacity, mode)
        d_rng = torch.from_numpy(np.ascontiguousarray(rng, np.uint32).view(np.int32).reshape(-1)).to(dev) if rng is not None else None
        for _ in range(launches):
            status = nat.lib().vrt_physics_run_batch_contacts(
                d_bodies.data_ptr() if n else None, runs, n, self.models.data_ptr(), self.models.numel(), self.remap.data_ptr(),
                self.remap.numel(), self.matphys.data_ptr(), self.n_materials, C.byref(params), C.byref(rp), d_done.data_ptr(), None,
                stats.data_ptr(), torch.cuda.current_stream().cuda_stream, d_rng.data_ptr() if d_rng is not None else None, None, C.byref(log))
            torch.cuda.synchronize()
            if status != 0:
                break
        self.rng_after = d_rng.cpu().numpy().view(np.uint32).reshape(runs, -1) if d_rng is not None else None
        return (status, stats.cpu().numpy().reshape(runs, nat.NSTATS), d_done.cpu().numpy(), d_counts.cpu().numpy(),
                d_records.cpu().numpy()[:runs * capacity * nat.CONTACT_BYTES].reshape(runs, -1))


@gpu
def test_the_abi_refuses_bad_arguments_and_keeps_its_counts():
    cu.assert_refusals(nat.lib())                      # VRT_ERR_ARG before any HIP call, with a device present as without
    abi = Abi()
    ticks = abi.ticks
    want = cu.host("edges_tiny")[6]
    total, row = want.total, nat.CONTACT_BYTES
    assert total == 24
    status, stats, done, counts, records = abi.call(2, [0, 0], [0, 0], 32)
    assert status == 0 and done.tolist() == [ticks] * 2 and counts.tolist() == [total] * 2
    assert records[0][:total * row].tobytes() == want.records.tobytes() == records[1][:total * row].tobytes()
    assert (records[:, total * row:] == 0xAB).all()                                        # nothing past the count is written
    # a count preset at or past the capacity stores nothing and still counts; one preset below it goes on from there
    status, stats, done, counts, records = abi.call(3, [0, 0, 0], [8, 9, 5], 8)
    assert status == 0 and counts.tolist() == [8 + total, 9 + total, 5 + total]
    assert (records[0] == 0xAB).all() and (records[1] == 0xAB).all()
    assert (records[2][:5 * row] == 0xAB).all() and records[2][5 * row:].tobytes() == want.records[:3].tobytes()
    # a run with a bad d_ticks_done word, and one that is done, leave count and records untouched; the others complete
    status, stats, done, counts, records = abi.call(4, [0, -1, ticks + 1, ticks], [0, 3, 4, 5], 32)
    assert status == 0 and done.tolist() == [ticks, -1, ticks + 1, ticks] and counts.tolist() == [total, 3, 4, 5]
    assert stats[:, nat.S_PHYSICS_BATCH_BADTICK].tolist() == [0, 1, 1, 0] and (records[1:] == 0xAB).all()
    assert records[0][:total * row].tobytes() == want.records.tobytes()
    # no bodies: every tick is done, the log is left alone
    status, stats, done, counts, records = abi.call(2, [0, 4], [7, 0], 4, n=0)
    assert status == 0 and done.tolist() == [ticks] * 2 and counts.tolist() == [7, 0] and (records == 0xAB).all()
    assert stats[:, nat.S_PHYSICS_TICKS].tolist() == [ticks, ticks - 4]
    # only bits 0 and 1 of a mask byte are read: 0xFC logs nothing for that body, 0xFD logs it as the mover, 0xFE as the other
    for mask, logged in (([0xFC, 0xFC], 0), ([0xFC, 0xFD], total), ([0xFE, 0xFC], total), ([0xFD, 0xFE], 0), ([0x00, 0x03], total)):
        status, stats, done, counts, records = abi.call(1, [0], [0], 32, mask=mask)
        assert status == 0 and counts.tolist() == [logged] and int(stats[0][nat.S_PHYSICS_CONTACTS]) == total, mask
        assert records[0][:logged * row].tobytes() == want.records[:logged].tobytes() and (records[0][logged * row:] == 0xAB).all(), mask
    # PAIRS, in one launch and chained by the budget: one tick per launch, the counts carried from launch to launch in d_counts
    pairs = cu.host("edges_tiny", "pairs")[6]
    assert 0 < pairs.total < total
    for launches, budget in ((1, 1 << 40), (ticks, 1)):
        status, stats, done, counts, records = abi.call(2, [0, 0], [0, 0], 32, mode=nat.CONTACTS_PAIRS, budget=budget, launches=launches)
        assert status == 0 and done.tolist() == [ticks] * 2 and counts.tolist() == [pairs.total] * 2, launches
        assert stats[:, nat.S_PHYSICS_TICKS].tolist() == ([ticks] * 2 if launches == 1 else [1, 1])
        assert records[0][:pairs.total * row].tobytes() == pairs.records.tobytes() == records[1][:pairs.total * row].tobytes(), launches
        assert (records[:, pairs.total * row:] == 0xAB).all()
    # a run short of its ticks after the launches made: the log holds the ticks done so far
    status, stats, done, counts, records = abi.call(1, [0], [0], 32, budget=1, launches=ticks - 1)
    part = want.records[want.records["tick"] < ticks - 1]
    assert done.tolist() == [ticks - 1] and counts.tolist() == [len(part)] and records[0][:len(part) * row].tobytes() == part.tobytes()
    # the drawing instance (d_rng set): in this all-solid world every draw passes, so the log is the same; a run whose generator's
    # index word is above 624 is left alone -- its count, its records, its generator and its ticks -- and says so
    words = np.array([random.Random(s).getstate()[1] for s in (1, 2, 3)], np.uint32)
    words[1, 624] = 625
    status, stats, done, counts, records = abi.call(3, [0, 0, 0], [0, 6, 2], 32, rng=words)
    assert status == 0 and done.tolist() == [ticks, 0, ticks] and counts.tolist() == [total, 6, 2 + total]
    assert stats[:, nat.S_PHYSICS_RNG_INVALID].tolist() == [0, 1, 0] and (stats[[0, 2], nat.S_PHYSICS_DRAWS] > 0).all()
    assert records[0][:total * row].tobytes() == want.records.tobytes() and (records[0][total * row:] == 0xAB).all()
    assert (records[1] == 0xAB).all() and np.array_equal(abi.rng_after[1], words[1]) and not np.array_equal(abi.rng_after[0], words[0])
    assert (records[2][:2 * row] == 0xAB).all() and records[2][2 * row:(2 + total) * row].tobytes() == want.records.tobytes()
