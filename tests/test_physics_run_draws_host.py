"""Many physics ticks with the reference's random draws (DeviceWorld.run(rng=), vrt_physics_run_draws), without a GPU: the C
ABI's new symbol, what it refuses before its first HIP call, its place in the build; the fixture tests/golden/physics_run_draws.npz
(tests/golden/make_physics_run_draws.py, tests/physics_run_draw_scenes.py) is what it says it is, and the host path
(world.run(follow=, clock=, rng=)) reproduces it bit for bit, draws and generator included; the Python interface; and the
compiler's resource report of python_raytracer_amd/csrc/vrt_physics_run_draws.hip against the saved one."""
import ctypes as C
import inspect
import json
import os
import random
import re

import numpy as np
import pytest

import kernel_report
import physics_anim_scenes as an
import physics_run_draw_scenes as rd
import physics_run_draws_report
import physics_run_util as ru
from python_raytracer_amd import _native as nat
from python_raytracer_amd import world
from python_raytracer_amd.lib import vec3

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vrt.h")
REACH = ("held_camera_changes_end_and_draws", "asleep_would_have_drawn", "held_clock_changes_draws_from_switch",
         "earlier_twin_drew_against_old_frame", "tick_crosses_a_state", "open_both_ways_in_one_pass", "another_seed_changes_run")


# ---- 1. the C ABI -----------------------------------------------------------------------------------------------------------
def test_symbol_and_build():
    text = open(HEADER).read()
    assert re.search(r"int vrt_physics_run_draws\(vrt_body\* d_bodies, int32_t n_bodies, const uint8_t\* d_models, int64_t models_bytes,\s+"
                     r"const uint8_t\* d_remap, int32_t remap_bytes, const double\* d_matphys, int32_t n_materials,\s+"
                     r"const vrt_physics_params\* params, const vrt_physics_run_params\* run, vrt_body_sample\* d_trace,\s+"
                     r"uint64_t\* d_stats, void\* stream, const int32_t\* d_body_sprite, vrt_anim_sprite\* d_sprites,\s+"
                     r"int32_t n_sprites, const vrt_anim_frame\* d_frames, int32_t n_frame_rows, const int32_t\* d_schedule,\s+"
                     r"vrt_anim_sample\* d_anim_trace, uint32_t\* d_rng, uint64_t\* d_tick_draws\);", text)
    assert "#define VRT_ABI_VERSION 9" in text
    L = nat.lib()
    assert L.vrt_abi_version() == 9 and nat.ABI_VERSION == 9      # the change only adds a symbol
    assert L.vrt_physics_run_draws is not None
    assert nat.EXPORTS[-2:] == ["vrt_physics_run_draws", "vrt_physics_run_anim"] and nat.EXPORTS.count("vrt_physics_run_draws") == 1
    assert list(L.vrt_physics_run_draws.argtypes) == list(L.vrt_physics_run_anim.argtypes) + [C.c_void_p, C.c_void_p]
    # the build: a unit of its own in the one library, counted by needs_build(), and in the variant build
    assert [os.path.basename(u) for u in nat.PHYSICS_RUN_DRAWS_UNITS] == ["vrt_physics_run_draws.hip"]
    assert set(nat.PHYSICS_RUN_DRAWS_UNITS) <= set(nat.SOURCES)
    others = nat.UNITS + nat.PHYSICS_UNITS + nat.PHYSICS_DRAWS_UNITS + nat.PHYSICS_RUN_UNITS + nat.PHYSICS_ANIM_UNITS
    assert len(others) == 6 and not set(nat.PHYSICS_RUN_DRAWS_UNITS) & set(others)
    assert "csrc/vrt_physics_run_draws.hip" in open(os.path.join(ROOT, "tools", "build_variant.sh")).read()
    # the default budget of a run with draws: derived from the measured cost of a unit, a power of two
    assert "#define VRT_PHYSICS_RUN_DRAWS_BUDGET %d\n" % nat.PHYSICS_RUN_DRAWS_BUDGET in text
    assert nat.PHYSICS_RUN_DRAWS_BUDGET & (nat.PHYSICS_RUN_DRAWS_BUDGET - 1) == 0 and nat.PHYSICS_RUN_BUDGET == 8192
    bench = json.load(open(os.path.join(ROOT, "profiles", "physics_run_draws_bench.json")))["budget"]
    assert bench["shipped"] == nat.PHYSICS_RUN_DRAWS_BUDGET == bench["power_of_two"] <= bench["units_for_target"]
    assert nat.RNG_WORDS == 625 and (nat.S_PHYSICS_RNG_INVALID, nat.S_PHYSICS_DRAWS, nat.S_PHYSICS_TICKS) == (7, 15, 6)


def test_physics_run_draws_rejects_bad_arguments_without_a_device():
    """Everything the entry point can refuse is refused before its first HIP call: these calls carry made-up device
    pointers, which nothing reads."""
    L = nat.lib()
    fake = 0x1000
    good = nat.VrtPhysicsParams(1.0, 1.0, 0.1, 0.01, 10.0)

    def call(n=4, run_ticks=8, trace=fake, body_sprite=fake, sprites=fake, n_sprites=2, frames=fake, n_rows=4, schedule=fake, anim_trace=fake,
             stats=fake, rng=fake, tick_draws=fake, follow=2, budget=1 << 16, params=good, dist_max=40.0):
        rp = nat.VrtPhysicsRunParams((C.c_double * 3)(0.0, 4.0, 3.0), (C.c_double * 3)(0.0, 4.0, 3.0), dist_max, 24.0, budget, run_ticks, follow)
        return L.vrt_physics_run_draws(fake, n, fake, 64, fake, 8, fake, 3, C.byref(params) if params else None, C.byref(rp), trace, stats, None,
                                       body_sprite, sprites, n_sprites, frames, n_rows, schedule, anim_trace, rng, tick_draws)

    # vrt_physics_tick's and vrt_physics_run's refusals are this call's
    assert call(stats=None) == -1 and call(n=-1) == -1 and call(run_ticks=0) == -1 and call(trace=fake + 4) == -1
    assert call(stats=fake + 4) == -1 and call(params=None) == -1 and call(budget=0) == -1 and call(follow=4) == -1 and call(follow=-2) == -1
    assert call(dist_max=float("inf")) == -1 and call(params=nat.VrtPhysicsParams(float("nan"), 1.0, 0.1, 0.01, 10.0)) == -1
    # ... vrt_physics_run_anim's: negative counts, NULL or misaligned arrays while there are sprites
    assert call(n_sprites=-1) == -1 and call(n_rows=-1) == -1 and call(n_sprites=0, n_rows=-1) == -1
    assert call(sprites=None) == -1 and call(schedule=None) == -1 and call(body_sprite=None) == -1 and call(frames=None) == -1
    assert call(sprites=fake + 2) == -1 and call(schedule=fake + 1) == -1 and call(body_sprite=fake + 3) == -1
    assert call(frames=fake + 4) == -1 and call(anim_trace=fake + 4) == -1 and call(anim_trace=fake + 4, n_sprites=0) == -1
    # ... and its own: the generator's words and the per-tick counts
    assert call(rng=None) == -1 and call(rng=fake + 2) == -1 and call(tick_draws=fake + 4) == -1
    assert call(rng=None, n_sprites=0) == -1 and call(rng=fake + 1, tick_draws=None) == -1


# ---- 2. the fixture ---------------------------------------------------------------------------------------------------------
def test_the_fixture_is_what_it_says():
    z, specs, reached = rd.load_fixture()
    assert specs == json.loads(json.dumps(rd.SCENES)) and list(specs) == ["wade", "tide"]
    assert os.path.getsize(rd.PATH) < 200 * 1024
    assert set(reached) == set(REACH) and all(reached[k] >= 1 for k in REACH), reached
    for name, spec in specs.items():
        n, ticks = len(spec["objects"]), spec["ticks"]
        assert n <= 8 and ticks <= 24
        for f in ("pos", "vel", "held_pos", "held_vel"):
            assert z[name + "/" + f].shape == (ticks, n, 3) and z[name + "/" + f].dtype == np.float64
        for f in ("mins", "maxs"):
            assert z[name + "/" + f].shape == (ticks, n, 3)
        for f in ("visible", "redraw", "weight"):
            assert z[name + "/" + f].shape == (ticks, n)
        assert z[name + "/frame"].shape == (ticks, len(spec["sprites"])) and z[name + "/weight0"].shape == (n,)
        draws, state = z[name + "/draws"], z[name + "/state"]
        assert draws.shape == z[name + "/held_draws"].shape == (ticks,) and state.shape == (625,) and state.dtype == np.uint32
        # the recorded draws and the recorded final state belong together: random.Random(seed) advanced by that many draws
        gen = random.Random(spec["seed"])
        for _ in range(int(draws.sum())):
            gen.random()
        assert np.array_equal(rd.state_words(gen), state), name
        assert 2 * int(draws.sum()) > 3 * 624                      # more than three states of the generator
        # held, the scene ends elsewhere and draws differently
        assert (z[name + "/pos"][-1] != z[name + "/held_pos"][-1]).any() and (draws != z[name + "/held_draws"]).any()
    # wade: the camera rides on body 1; body 2 lies asleep at first and draws once it wakes
    wade = specs["wade"]
    assert wade["follow"] == 1 and any(m["solidity"] == 0.25 for m in wade["materials"])
    # tide: frames of solidity 1, 0.5 and none; the sprite is shown twice, rafts before and between
    tide = specs["tide"]
    frames = tide["sprites"]["plat"]["frames"]
    assert [tide["materials"][f[0][2]]["solidity"] if f else None for f in frames] == [1, 0.5, None]
    assert [o["sprite"] for o in tide["objects"]] == ["raft", "plat", "raft", "plat"]
    assert sorted(set(z["tide/frame"][:, 0].tolist())) == [0, 1, 2] and "anim" not in tide["sprites"]["raft"]


@pytest.mark.parametrize("name", list(rd.SCENES))
def test_host_run_with_follow_clock_and_rng_is_the_references(name):
    z, spec, objects, sprites, st, who = rd.fresh(name)
    assert (who is not None) == (name == "wade")
    gen = random.Random(spec["seed"])
    made = []

    def draw():
        made[-1] += 1
        return gen.random()

    # tick by tick, for the draws of every tick ...
    start, step = spec["clock"]
    rows, anims = [], []
    for k in range(spec["ticks"]):
        made.append(0)
        cam = who.cam_pos if who is not None else vec3(*spec["cam"])
        _, trace, anim = world.run(objects, cam, st, 1, trace=True, rng=draw, clock=(start + k * step, 0))
        rows.append(trace[0]), anims.append(anim[0])
    an.assert_ticks(z, name, spec, objects, sprites, np.array(rows), np.array(anims), name + " (host, tick by tick)")
    assert made == z[name + "/draws"].tolist()
    assert np.array_equal(rd.state_words(gen), z[name + "/state"])
    # ... and as one run, with the generator itself
    z, spec, objects, sprites, st, who = rd.fresh(name)
    gen = random.Random(spec["seed"])
    _, trace, anim = world.run(objects, vec3(*spec["cam"]), st, spec["ticks"], follow=who, trace=True, rng=gen.random, clock=tuple(spec["clock"]))
    an.assert_ticks(z, name, spec, objects, sprites, trace, anim, name + " (host)")
    assert np.array_equal(rd.state_words(gen), z[name + "/state"])
    # held: the camera where it stood (wade), the clock at 0 (tide)
    z, spec, objects, sprites, st, who = rd.fresh(name)
    gen = random.Random(spec["seed"])
    _, trace, _ = world.run(objects, vec3(*spec["cam"]), st, spec["ticks"], trace=True, rng=gen.random, clock=(0, 0))
    assert np.array_equal(ru.bits(trace["pos"]), ru.bits(z[name + "/held_pos"])) and np.array_equal(ru.bits(trace["vel"]), ru.bits(z[name + "/held_vel"]))


# ---- 3. the Python interface ------------------------------------------------------------------------------------------------
def test_run_takes_rng_and_the_result_has_the_draws():
    from python_raytracer_amd.results import RunResult
    sig = inspect.signature(world.DeviceWorld.run)
    assert list(sig.parameters) == ["self", "objects", "pos_cam", "settings", "ticks", "follow", "trace", "budget", "time_kernel", "clock", "rng"]
    assert sig.parameters["rng"].default is None
    records = np.zeros(2, np.dtype(nat.BODY_FIELDS))
    plain = RunResult(records, [], None, 3, 1, None, (3, 2))
    assert plain.draws is None and plain.draws_per_tick is None
    with_rng = RunResult(records, [], None, 3, 1, None, (3, 2), draws_per_tick=np.array([5, 0, 7], np.uint64))
    assert with_rng.draws == 12 and isinstance(with_rng.draws, int) and with_rng.draws_per_tick.dtype == np.uint64
    assert "rng" in world.DeviceWorld.run.__doc__ and "vrt_physics_run_draws" in world.DeviceWorld.run.__doc__


# ---- 4. the compiler's report of the new translation unit -------------------------------------------------------------------
def test_physics_run_draws_report_is_the_saved_one():
    if not os.path.exists(kernel_report.HIPCC):
        pytest.skip("no hipcc")
    fresh_report = kernel_report.parse(physics_run_draws_report.compile_report())
    saved = physics_run_draws_report.saved()
    assert list(fresh_report) == list(saved) and fresh_report == saved
    names = [n for n in fresh_report if "physics_run_draws_kernel" in n]
    assert len(names) == len(fresh_report) == 2                 # with and without the sprite tables
    for n in names:
        fig = fresh_report[n]
        assert fig["VGPRs"] <= 128                              # 1024 threads are 4 waves per SIMD: 512 / 4 registers each
        assert fig["Occupancy [waves/SIMD]"] >= 4               # ... or the workgroup does not launch
        assert 0 < fig["LDS Size [bytes/block]"] <= 64 * 1024   # within what every launch may ask for without opting in
        # recorded, not conditions: vector spills and scratch
        print(n, "VGPRs Spill", fig["VGPRs Spill"], "ScratchSize", fig["ScratchSize [bytes/lane]"], "SGPRs Spill", fig["SGPRs Spill"])
