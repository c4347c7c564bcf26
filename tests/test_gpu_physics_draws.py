"""Object physics on the device with the reference's random draws (DeviceWorld.tick(rng=), vrt_physics_tick_draws): the runs
recorded from the real reference with seeded draws -- `fluid` (tests/physics_draw_scenes.py: every class of test in one pass,
draws across the generator's states, slabs of three passes) and `fraction` -- tick by tick and bit for bit, with the generator
left in the state the host path (world.tick) leaves its own in; the all-solid recorded scenes, whose draws decide nothing and
still move the generator; generators that start at any index, odd ones included; host and device ticks taking turns on one
generator; an index word out of range through the raw ABI; and what `rng` may be."""
import ctypes as C
import random

import numpy as np
import pytest

import physics_draw_scenes  # noqa: F401  (the scene the fixture `fluid` was recorded from)
import physics_scenes as ps
from python_raytracer_amd import _native as nat
from python_raytracer_amd import world
from python_raytracer_amd.lib import vec3
from python_raytracer_amd.world import DeviceWorld

gpu = pytest.mark.gpu
WORDS = ("BODIES", "REFUSED", "STEPS", "BLOCKED", "CONTACTS", "TRANSFERS", "CAPPED")


def counted(gen):
    """gen.random, counting its calls: ([count], the function)."""
    made = [0]

    def draw():
        made[0] += 1
        return gen.random()
    return made, draw


def run_both(name, gen_dev, gen_host, record=True, device_turn=lambda k: True):
    """The fixture's scene twice -- DeviceWorld.tick(rng=gen_dev) on one set of objects, world.tick with gen_host's draws on a
    twin -- held to each other after every tick in every field, the counts, the statistics, the number of draws and the
    generators' states, and (record) to the fixture.  device_turn(k) False: tick k of the first set runs on the host as well,
    with gen_dev."""
    z, spec = ps.load_fixture(name)
    dev, _, _, st = ps.project_scene(spec)
    host, _, _, _ = ps.project_scene(spec)
    dw = DeviceWorld(16)
    cam_d = cam_h = spec["cam"]
    total = 0
    for k in range(spec["ticks"]):
        ps.clear_redraw(dev), ps.clear_redraw(host)
        cam_d, cam_h = ps.apply_script(spec, k, dev, vec3, cam_d), ps.apply_script(spec, k, host, vec3, cam_h)
        made, draw = counted(gen_host)
        want = world.tick(host, vec3(*cam_h), st, rng=draw)
        if device_turn(k):
            r = dw.tick(dev, vec3(*cam_d), st, rng=gen_dev)
            assert np.array_equal(r.counters, want), (name, k, r.counters, want)
            ran = want[want["status"] == 0]
            totals = dict(BODIES=len(ran), REFUSED=0, STEPS=ran["steps"].sum(), BLOCKED=ran["blocked_steps"].sum(),
                          CONTACTS=ran["contacts"].sum(), TRANSFERS=ran["transfers"].sum(), CAPPED=0)
            assert {w: int(r.stats[getattr(nat, "S_PHYSICS_" + w)]) for w in WORDS} == {w: int(v) for w, v in totals.items()}, (name, k)
            assert r.draws == made[0] == int(r.stats[nat.S_PHYSICS_DRAWS]), (name, k, r.draws, made[0])
            assert not r.stats[:8].any()
            assert r.moved == [o for o, m in zip(dev, want["moved"]) if m]
        else:
            world.tick(dev, vec3(*cam_d), st, rng=gen_dev.random)
        got, twin = ps.state(dev), ps.state(host)
        for f in got:
            assert got[f].tobytes() == twin[f].tobytes(), (name, k, f, got[f], twin[f])
        assert gen_dev.getstate() == gen_host.getstate(), (name, k)
        if record:
            ps.assert_tick(z, k, dev, name + " (device)")
            if "draws" in z.files:
                assert made[0] == int(z["draws"][k]), (name, k)
        total += made[0]
    return z, spec, total


# ---- 1. the recorded runs with fractional solidity -----------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", ["fluid", "fraction"])
def test_device_tick_makes_the_references_draws(name):
    _, spec = ps.load_fixture(name)
    _, _, total = run_both(name, random.Random(spec["seed"]), random.Random(spec["seed"]))
    assert total > 2 * 624 or name == "fraction"          # (fluid: the run goes through many states of the generator)


@gpu
def test_a_bound_method_and_the_modules_own_generator():
    """rng=random.Random(s).random is the generator behind it; rng=random.random the module's hidden instance."""
    _, spec = ps.load_fixture("fraction")
    objects, _, _, st = ps.project_scene(spec)
    twin, _, _, _ = ps.project_scene(spec)
    gen, ref = random.Random(7), random.Random(7)
    dw = DeviceWorld(8)
    for k in range(3):
        dw.tick(objects, vec3(*spec["cam"]), st, rng=gen.random)
        world.tick(twin, vec3(*spec["cam"]), st, rng=ref.random)
    assert gen.getstate() == ref.getstate() and ps.state(objects)["vel"].tobytes() == ps.state(twin)["vel"].tobytes()
    saved = random.getstate()
    try:
        random.seed(7)
        objects, _, _, st = ps.project_scene(spec)
        for k in range(3):
            dw.tick(objects, vec3(*spec["cam"]), st, rng=random.random)
        assert random.getstate() == ref.getstate() and ps.state(objects)["vel"].tobytes() == ps.state(twin)["vel"].tobytes()
    finally:
        random.setstate(saved)


# ---- 2. all-solid scenes: the draws decide nothing and are made all the same -----------------------------------------------------
@gpu
@pytest.mark.parametrize("name", ["edges_tiny", "edges_face", "edges_chain", "crowd"])
def test_solid_scenes_draw_and_still_equal_the_record(name):
    _, _, total = run_both(name, random.Random(11), random.Random(11))
    assert total > (2000 if name == "edges_face" else 0)


# ---- 3. any start index ----------------------------------------------------------------------------------------------------------
def _at_index(seed, index):
    """A generator whose next output is word `index` of its state (a fresh seed leaves 624)."""
    gen = random.Random(seed)
    if index != 624:
        for _ in range(index):
            gen.getrandbits(32)
    assert gen.getstate()[1][-1] == index
    return gen


@gpu
@pytest.mark.parametrize("index", [1, 2, 623, 624])
def test_generators_that_start_at_any_index(index):
    _, spec = ps.load_fixture("fraction")
    run_both("fraction", _at_index(spec["seed"], index), _at_index(spec["seed"], index), record=index == 624)


# ---- 4. host and device ticks take turns -------------------------------------------------------------------------------------------
@gpu
def test_host_and_device_ticks_interleave_on_one_generator():
    _, spec = ps.load_fixture("fluid")
    run_both("fluid", random.Random(spec["seed"]), random.Random(spec["seed"]), device_turn=lambda k: k % 2 == 1)


# ---- 5. the raw ABI: an index word out of range ------------------------------------------------------------------------------------
@gpu
def test_an_index_out_of_range_makes_the_tick_a_no_op():
    import torch
    from test_gpu_physics import _hand_scene
    models, remap, matphys, slab, cube, free = _hand_scene()
    bodies = np.array([slab, cube, free])
    bodies["steps"], bodies["moved"], bodies["status"] = 9, 9, 9        # the `out` words are written all the same
    dev = torch.device("cuda", torch.cuda.current_device())
    d_b = torch.from_numpy(bodies.view(np.uint8).reshape(-1).copy()).to(dev)
    d_m, d_r = torch.from_numpy(models).to(dev), torch.from_numpy(remap).to(dev)
    d_p = torch.from_numpy(matphys.reshape(-1)).to(dev)
    stats = torch.full((nat.NSTATS,), 77, dtype=torch.int64, device=dev)
    words = np.array(random.Random(3).getstate()[1], np.uint32)
    p = nat.VrtPhysicsParams(1.0, 1.0, 0.125, 2.0 ** -7, 8.0)

    def call(index):
        words[624] = index
        d_rng = torch.from_numpy(words.view(np.int32).copy()).to(dev)
        rc = nat.lib().vrt_physics_tick_draws(d_b.data_ptr(), len(bodies), d_m.data_ptr(), d_m.numel(), d_r.data_ptr(), d_r.numel(),
                                              d_p.data_ptr(), 1, C.byref(p), stats.data_ptr(), d_rng.data_ptr(),
                                              torch.cuda.current_stream().cuda_stream)
        assert rc == 0, rc
        torch.cuda.synchronize()
        return d_b.cpu().numpy().view(np.dtype(nat.BODY_FIELDS)), stats.cpu().numpy(), d_rng.cpu().numpy().view(np.uint32)

    for index in (625, 0xFFFFFFFF):
        out, st, after = call(index)
        assert (out["status"] == nat.BODY_REFUSED).all()
        a, b = out.copy(), bodies.copy()
        for f in ("steps", "blocked_steps", "contacts", "transfers", "moved", "status"):
            assert f == "status" or not out[f].any()
            a[f] = b[f] = 0
        assert a.tobytes() == b.tobytes()                    # but for the `out` words not a byte of a body changed
        assert np.array_equal(after, words)                  # nor a word of the generator
        assert st[nat.S_PHYSICS_RNG_INVALID] == 1 and st[nat.S_PHYSICS_REFUSED] == len(bodies)
        assert not np.delete(st, [nat.S_PHYSICS_RNG_INVALID, nat.S_PHYSICS_REFUSED]).any()
    # the same records with a legal index: the cube comes down on the slab.  Its second step tests 3 x 2 x 3 slab voxels (its
    # box is inclusive); 9 of them hold a voxel of the slab, 4 of those face a voxel of the cube: 4 x 2 + 5 draws
    out, st, after = call(624)
    assert out[1]["steps"] == 2 and out[1]["blocked_steps"] == 1 and out[1]["contacts"] == 4 and out[1]["pos"].tolist() == [0, 2, 0]
    assert st[nat.S_PHYSICS_RNG_INVALID] == 0 and st[nat.S_PHYSICS_DRAWS] == 13 and after[624] == 26
    gen = random.Random(3)
    for _ in range(13):
        gen.random()
    assert np.array_equal(after, np.array(gen.getstate()[1], np.uint32))


# ---- 6. what rng may be ------------------------------------------------------------------------------------------------------------
@gpu
def test_rng_argument_handling():
    _, spec = ps.load_fixture("fraction")
    objects, _, mats, st = ps.project_scene(spec)
    cam = vec3(*spec["cam"])
    before = ps.state(objects)
    dw = DeviceWorld(8)
    for bad in (object(), 5, lambda: 0.5, "random"):
        with pytest.raises(TypeError, match="rng"):
            dw.tick(objects, cam, st, rng=bad)
    with pytest.raises(ValueError, match="fractional solidity"):
        dw.tick(objects, cam, st, rng=None)
    after = ps.state(objects)
    assert all(np.array_equal(before[k], after[k]) for k in before)
    # a physical object whose material has no `weight`: raised before the launch, the generator is untouched
    gen = random.Random(5)
    gen.random()
    state = gen.getstate()
    objects[1].weight = None
    with pytest.raises(ValueError, match="weight"):
        dw.tick(objects, cam, st, rng=gen)
    assert gen.getstate() == state
    after = ps.state(objects)
    assert all(np.array_equal(before[k], after[k]) for k in before)
