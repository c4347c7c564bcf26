"""The physics tick that makes the reference's random draws, without a GPU: the host path (world.tick with a seeded generator)
against the run recorded from the real reference on the scene of fractional solidities (tests/golden/physics_fluid.npz,
tests/golden/make_physics_draws.py), what that run reached, the C ABI's new symbol and what vrt_physics_tick_draws refuses before
any HIP call, and the compiler's resource report of python_raytracer_amd/csrc/vrt_physics_draws.hip against the saved one."""
import ctypes as C
import json
import os
import random
import re

import numpy as np
import pytest

import kernel_report
import physics_draw_scenes as pds
import physics_draws_report
import physics_scenes as ps
from python_raytracer_amd import _native as nat
from python_raytracer_amd import world
from python_raytracer_amd.lib import vec3

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vrt.h")


def test_host_tick_with_the_seeded_generator_is_the_references():
    z, spec = ps.load_fixture("fluid")
    assert json.loads(json.dumps(pds.SCENES["fluid"])) == spec        # the file was made from the scene as it is described now
    objects, _, _, st = ps.project_scene(spec)
    gen = random.Random(spec["seed"])
    made = [0]

    def draw():
        made[0] += 1
        return gen.random()

    assert z["draws"].dtype == np.int64 and len(z["draws"]) == spec["ticks"] == len(z["pos"])
    for k in range(spec["ticks"]):
        ps.clear_redraw(objects)
        before = made[0]
        world.tick(objects, vec3(*spec["cam"]), st, rng=draw)
        ps.assert_tick(z, k, objects, "fluid")
        assert made[0] - before == z["draws"][k], k
    # the generator went through its states in step with the reference's: 624 outputs a state, two a draw
    twin = random.Random(spec["seed"])
    for _ in range(int(z["draws"].sum())):
        twin.random()
    assert gen.getstate() == twin.getstate() and z["draws"].sum() * 2 > 20 * 624


def test_the_recorded_run_reaches_what_it_is_for():
    """What make_physics_draws.py demanded of the reference's run before it wrote the file, from the file: (b) a pass of 1024
    tests with all four classes of test, (c) a pass whose draws come from two states of the generator, (d) a step of more than
    1024 tests with contacts beyond the first pass, (e) undecided tests that went each way, (f) a field another seed changes."""
    z, spec = ps.load_fixture("fluid")
    reached = json.loads(bytes(z["reached"]).decode())
    for key in ("passes_of_all_four_classes", "passes_across_a_regeneration", "slab_over_1024_contact_beyond", "open_passed",
                "open_failed", "fields_another_seed_changes", "blocked_steps"):
        assert reached[key] >= 1, (key, reached)
    assert reached["outside"] == 0 and reached["draws_max"] == z["draws"].max() > 1024
    solid = sorted(m["solidity"] for m in spec["materials"])
    assert solid == [-0.5, 0, 0.25, 0.5, 0.75, 1, 2.0]
    # another seed, another run
    objects, _, _, st = ps.project_scene(spec)
    other = random.Random(spec["seed"] + 1).random
    path = []
    for k in range(spec["ticks"]):
        world.tick(objects, vec3(*spec["cam"]), st, rng=other)
        path.append(ps.state(objects)["vel"])
    assert not np.array_equal(np.array(path), z["vel"])


def test_symbol_header_and_build():
    text = open(HEADER).read()
    assert re.search(r"int vrt_physics_tick_draws\(vrt_body\* d_bodies, int32_t n_bodies, const uint8_t\* d_models, int64_t models_bytes,\s+"
                     r"const uint8_t\* d_remap, int32_t remap_bytes, const double\* d_matphys, int32_t n_materials,\s+"
                     r"const vrt_physics_params\* params, uint64_t\* d_stats, uint32_t\* d_rng, void\* stream\);", text)
    for name, word in (("RNG_INVALID", 7), ("DRAWS", 15)):
        assert re.search(r"VRT_S_PHYSICS_%s = %d\b" % (name, word), text), name
        assert getattr(nat, "S_PHYSICS_" + name) == word
    assert "#define VRT_ABI_VERSION 9" in text and nat.ABI_VERSION == 9       # the change only adds a symbol
    L = nat.lib()
    assert L.vrt_abi_version() == 9 and L.vrt_physics_tick_draws is not None and "vrt_physics_tick_draws" in nat.EXPORTS
    assert nat.RNG_WORDS == 625 == len(random.Random(0).getstate()[1])
    assert [os.path.basename(u) for u in nat.PHYSICS_DRAWS_UNITS] == ["vrt_physics_draws.hip"]
    assert set(nat.PHYSICS_DRAWS_UNITS) <= set(nat.SOURCES) and not set(nat.PHYSICS_DRAWS_UNITS) & set(nat.UNITS + nat.PHYSICS_UNITS)
    assert os.path.join(nat.HERE, "csrc", "vrt_physics_common.h") in nat.SOURCES      # a change to the shared header rebuilds
    assert "csrc/vrt_physics_draws.hip" in open(os.path.join(ROOT, "tools", "build_variant.sh")).read()
    from python_raytracer_amd.results import PhysicsResult
    assert isinstance(PhysicsResult.draws, property)


def test_physics_tick_draws_rejects_bad_arguments_without_a_device():
    """Everything the entry point can refuse is refused before its first HIP call: these calls carry made-up device
    pointers, which nothing reads."""
    L = nat.lib()
    fake = 0x1000
    good = nat.VrtPhysicsParams(1.0, 1.0, 0.1, 0.01, 10.0)

    def call(bodies=fake, n=4, models=fake, models_bytes=64, remap=fake, remap_bytes=8, matphys=fake, n_materials=3, params=good, stats=fake,
             rng=fake):
        return L.vrt_physics_tick_draws(bodies, n, models, models_bytes, remap, remap_bytes, matphys, n_materials,
                                        C.byref(params) if params is not None else None, stats, rng, None)

    assert call(rng=None) == -1 and call(rng=None, n=0) == -1 and call(rng=fake + 1) == -1 and call(rng=fake + 2) == -1
    assert call(stats=None) == -1 and call(stats=None, n=0) == -1 and call(params=None) == -1 and call(stats=fake + 4) == -1
    assert call(n=-1) == -1 and call(n=(1 << 20) + 1) == -1
    assert call(bodies=None) == -1 and call(bodies=fake + 4) == -1 and call(matphys=None) == -1 and call(matphys=fake + 4) == -1
    assert call(models=None) == -1 and call(remap=None) == -1 and call(models_bytes=-1) == -1 and call(remap_bytes=-1) == -1
    assert call(n_materials=-1) == -1 and call(n_materials=256) == -1
    for field in ("gravity", "friction", "friction_air", "min_velocity", "max_velocity"):
        for value in (float("nan"), float("inf")):
            bad = nat.VrtPhysicsParams(1.0, 1.0, 0.1, 0.01, 10.0)
            setattr(bad, field, value)
            assert call(params=bad) == -1, field


def test_rng_must_be_a_generator():
    gen = random.Random(1)
    assert world._generator(gen) is gen and world._generator(gen.random) is gen and world._generator(gen.getrandbits) is gen
    assert world._generator(random.random) is random._inst
    for bad in (object(), 0.5, lambda: 0.5, np.random.default_rng(1).random):
        with pytest.raises(TypeError, match="rng"):
            world._generator(bad)


def test_physics_draws_report_is_the_saved_one():
    if not os.path.exists(kernel_report.HIPCC):
        pytest.skip("no hipcc")
    fresh = kernel_report.parse(physics_draws_report.compile_report())
    saved = physics_draws_report.saved()
    assert list(fresh) == list(saved) and fresh == saved
    names = [n for n in fresh if "physics_draws_kernel" in n]
    assert len(names) == 1 and len(fresh) == 1               # one kernel: one launch per tick
    fig = fresh[names[0]]
    assert fig["VGPRs Spill"] == 0 and fig["ScratchSize [bytes/lane]"] == 0 and fig["SGPRs Spill"] == 0, fig
    assert fig["VGPRs"] <= 128                               # 1024 threads are 4 waves per SIMD: 512 / 4 registers each
    assert fig["LDS Size [bytes/block]"] <= 65536            # static LDS of one workgroup
