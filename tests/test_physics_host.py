"""Object physics without a GPU: the host path (world.tick, Object.update_physics) against the runs recorded from the real
reference (tests/golden/physics_*.npz, tests/golden/make_physics.py) tick by tick and bit for bit, Object.set_weight against
the recorded weights, the [PHYSICS] settings, the C ABI's new record and symbol, what vrt_physics_tick refuses before any HIP
call, and the compiler's resource report of python_raytracer_amd/csrc/vrt_physics.hip against the saved one."""
import ctypes as C
import json
import os
import random
import re

import numpy as np
import pytest

import kernel_report
import physics_report
import physics_scenes as ps
from python_raytracer_amd import _native as nat
from python_raytracer_amd import load_settings, make_settings, world
from python_raytracer_amd.lib import vec3

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vrt.h")


# ---- 1. the host path is the reference's -------------------------------------------------------------------------------------
def replay(name, seeded=False):
    """world.tick over the fixture's scene, held to the record after every tick; returns the per-tick counters."""
    z, spec = ps.load_fixture(name)
    objects, _, _, st = ps.project_scene(spec)
    rng = random.Random(spec["seed"]).random if seeded else None
    cam, out = spec["cam"], []
    for k in range(spec["ticks"]):
        ps.clear_redraw(objects)
        cam = ps.apply_script(spec, k, objects, vec3, cam)
        out.append(world.tick(objects, vec3(*cam), st, rng=rng))
        ps.assert_tick(z, k, objects, name)
    return z, spec, out


@pytest.mark.parametrize("name", ps.DEVICE_SCENES)
def test_host_tick_is_the_references(name):
    z, spec, counters = replay(name)
    assert json.loads(json.dumps(ps.SCENES[name])) == spec            # the file was made from the scene as it is described now
    assert len(z["pos"]) == spec["ticks"] and (z["pos"][-1] != np.array([o["pos"] for o in spec["objects"]])).any()
    assert sum(int((c["status"] == 0).sum()) for c in counters) > 0


def test_the_recorded_runs_reach_what_they_are_for():
    """What make_physics.py demanded of the reference's runs before it wrote the files, from the files."""
    total = {}
    for name in ps.DEVICE_SCENES:
        for k, v in json.loads(bytes(np.load(ps.fixture_path(name))["reached"]).decode()).items():
            total[k] = total.get(k, 0) + v
    assert total["blocked_steps"] >= 30 and total["transfers_inside"] >= 5 and total["transfers_one"] >= 1
    assert total["body_ticks_3_steps"] >= 1 and total["tie_steps"] >= 1 and total["slab_over_1024_contact_beyond"] >= 1
    assert total["steps_over_256_contacts"] >= 1 and total["order_dependent_sums"] >= 1
    assert total["outside"] > 0          # the default mod's cubes stand on voxels at model x = size.x: vrt_body.rim
    # the default mod's run: the player falls from y = 0 and comes to rest
    z, spec = ps.load_fixture("default")
    assert z["pos"][0][-1][1] == 0 and z["pos"][1][-1][1] < 0
    assert z["pos"][-1][-1][1] == z["pos"][-2][-1][1] and -23 < z["pos"][-1][-1][1] < -22
    # the object that becomes visible before tick 3 is not there for the mover before it until tick 4
    z, spec = ps.load_fixture("edges_vis")
    assert z["visible"][2][2] == 0 and z["visible"][3][2] == 1
    assert z["pos"][3][0][0] > z["pos"][2][0][0] and z["pos"][4][0][0] == z["pos"][3][0][0]
    assert not z["visible"][:, 1].any() and z["maxs"][2][0][0] > 17     # the invisible dot at 17..19 was passed through
    # asleep and sprite-less objects never move; the asleep one still takes velocity
    z, spec = ps.load_fixture("edges_sleep")
    assert (z["pos"][:, 0] == z["pos"][0, 0]).all() and (z["pos"][:, 2] == [5, 0, 0]).all() and z["vel"][0][0][0] > 0
    assert (z["pos"][-1, 3] != [-20, 0, 0]).any()


def test_the_crowd_reaches_past_one_tile_of_bodies():
    """The scene of more bodies than the device walks at a time (1024): what make_physics.py demanded of the reference's run,
    from the file, and the record itself.  Measured: 3 blocked steps of the bar with contacts on both sides of index 1024, the
    lower block's terms first, and a sum that depends on their order; 1 step that hands velocity to a body on either side; 12 free
    steps of bodies at 1024 and beyond; both visibility cases."""
    z, spec = ps.load_fixture("crowd")
    R, T = ps.CROWD_ROLES, ps.CROWD_SCRIPT_TICK
    assert len(spec["objects"]) == ps.CROWD_N >= 1024 + 64 and spec["ticks"] == 4
    reached = json.loads(bytes(z["reached"]).decode())
    for key in ("contacts_both_sides_one_step", "transfers_both_sides_one_step", "movers_from_1024", "visible_before_met", "visible_now_met"):
        assert reached[key] >= 1, (key, reached)
    # everything is in view from tick 0 on but the two parked obstacles, which the script brings in before tick T
    late = [R["late_low"], R["late_high"]]
    others = np.delete(np.arange(ps.CROWD_N), late)
    assert z["visible"][:, others].all() and not z["visible"][:T, late].any() and z["visible"][T:, late].all()
    # last tick's flag for the mover before the obstacle (it moves on at tick T, stops at T + 1), this tick's for the one after it
    x, zz = z["pos"][:, R["mover_low"], 0], z["pos"][:, R["mover_1024"], 2]
    assert x[T] > x[T - 1] and x[T + 1] == x[T] and zz[T - 1] > zz[T - 2] and zz[T] == zz[T - 1]
    # the bar rests on both blocks from tick 1 on; both takers took velocity at tick 1
    y = z["pos"][:, R["bar"], 1]
    assert y[0] > y[1] == y[2] == y[3]
    assert z["vel"][0, R["taker_high"], 0] == 0 and z["vel"][1, R["taker_high"], 0] > 0 and z["vel"][1, R["taker_low"], 0] > 0


def test_fractional_solidity_follows_the_callers_draws():
    z, spec, counters = replay("fraction", seeded=True)
    assert spec["seed"] is not None and any(0 < m["solidity"] < 1 for m in spec["materials"])
    assert sum(int(c["blocked_steps"].sum()) for c in counters) > 0
    # other draws, another run: the record pins the reference's sequence, not just any
    objects, _, _, st = ps.project_scene(spec)
    other = random.Random(spec["seed"] + 1).random
    path = []
    for k in range(spec["ticks"]):
        world.tick(objects, vec3(*spec["cam"]), st, rng=other)
        path.append(ps.state(objects)["vel"])
    assert not np.array_equal(np.array(path), z["vel"])      # (how many voxel pairs met decides the friction)


def test_set_weight_is_the_references_sum():
    for name in ("default", "pile", "edges_rot", "edges_lod"):
        z, spec = ps.load_fixture(name)
        objects, _, _, _ = ps.project_scene(spec)
        got = np.array([float(o.weight) for o in objects], np.float64)
        assert np.array_equal(got.view(np.uint64), z["weight"].view(np.uint64)), name
    z, spec = ps.load_fixture("default")
    assert z["weight"][-1] == 0.7519999999999726             # the player: an inexact sum, not count * weight
    assert z["weight"][-1] != 1504 * 0.0005


def test_update_without_objects_is_visibility_only():
    _, spec = ps.load_fixture("edges_tiny")
    objects, _, _, st = ps.project_scene(spec)
    before = ps.state(objects)
    for o in objects:
        assert o.update(vec3(0, 0, 0), st) is True
    after = ps.state(objects)
    assert np.array_equal(before["pos"], after["pos"]) and np.array_equal(before["vel"], after["vel"]) and after["visible"].all()
    # accelerate rebinds: the vector handed in is not the object's
    v = vec3(1.0, 0.0, 0.0)
    objects[1].accelerate(v)
    objects[1].accelerate(v)
    assert objects[1].vel.tuple() == (2.0, 0.0, 0.0) and v.tuple() == (1.0, 0.0, 0.0)


# ---- 2. settings -------------------------------------------------------------------------------------------------------------
def test_physics_settings():
    keys = ("gravity", "friction", "friction_air", "min_velocity", "max_velocity", "dist_move")
    st = make_settings()
    assert [getattr(st, k) for k in keys] == [1, 1, 0.1, 0.01, 10, 64]
    st = load_settings(os.path.join(ps.GOLDEN, "mod_default", "config.cfg"), threads=1)
    assert [getattr(st, k) for k in keys] == [1, 1, 0.1, 0.01, 10, 64]
    assert make_settings(gravity=0.5).gravity == 0.5


# ---- 3. the C ABI ------------------------------------------------------------------------------------------------------------
def test_symbols_and_layout():
    text = open(HEADER).read()
    body = re.search(r"typedef struct vrt_body \{(.*?)\} vrt_body;", text, re.S).group(1)
    names = re.findall(r"^\s+(?:double|int32_t|int64_t|vrt_object)\s+(\w+)", body, re.M)
    fields = ["pos", "vel", "weight", "object", "half", "visible_before", "visible_now", "awake", "physics", "has_sprite", "steps",
              "blocked_steps", "contacts", "transfers", "moved", "status", "rim", "pad"]
    offsets = [0, 24, 48, 56, 120, 132, 136, 140, 144, 148, 152, 156, 160, 164, 168, 172, 176, 184]
    assert names == fields
    assert [getattr(nat.VrtBody, f).offset for f in fields] == offsets and [f for f, *_ in nat.VrtBody._fields_] == fields
    dt = np.dtype(nat.BODY_FIELDS)
    assert [dt.fields[f][1] for f in fields] == offsets and list(dt.names) == fields
    assert C.sizeof(nat.VrtBody) == 192 == nat.BODY_BYTES == dt.itemsize and C.sizeof(nat.VrtPhysicsParams) == 40
    assert dt.fields["object"][0].itemsize == 64 == C.sizeof(nat.VrtObject)
    assert [dt.fields["object"][0].fields[f][1] for f, *_ in nat.VrtObject._fields_] == [getattr(nat.VrtObject, f).offset for f, *_ in nat.VrtObject._fields_]
    assert re.search(r"int vrt_physics_tick\(vrt_body\* d_bodies, int32_t n_bodies, const uint8_t\* d_models, int64_t models_bytes,\s+"
                     r"const uint8_t\* d_remap, int32_t remap_bytes, const double\* d_matphys, int32_t n_materials,\s+"
                     r"const vrt_physics_params\* params, uint64_t\* d_stats, void\* stream\);", text)
    for name, word in (("BODIES", 8), ("REFUSED", 9), ("STEPS", 10), ("BLOCKED", 11), ("CONTACTS", 12), ("TRANSFERS", 13), ("CAPPED", 14)):
        assert re.search(r"VRT_S_PHYSICS_%s = %d\b" % (name, word), text), name
        assert getattr(nat, "S_PHYSICS_" + name) == word
    assert "#define VRT_PHYSICS_STEP_CAP (3 * (VRT_PHYSICS_MAX_VEL + 2))" in text and nat.PHYSICS_STEP_CAP == 3 * (1024 + 2)
    assert (nat.BODY_OK, nat.BODY_SKIPPED, nat.BODY_REFUSED) == (0, -1, -3)
    assert "#define VRT_ABI_VERSION 9" in text
    L = nat.lib()
    assert L.vrt_abi_version() == 9 and nat.ABI_VERSION == 9      # the change only adds a symbol
    assert L.vrt_physics_tick is not None and "vrt_physics_tick" in nat.EXPORTS
    # the build: a unit of its own list, in the one library, counted by needs_build(), and in the variant build
    assert [os.path.basename(u) for u in nat.PHYSICS_UNITS] == ["vrt_physics.hip"] and set(nat.PHYSICS_UNITS) <= set(nat.SOURCES)
    assert not set(nat.PHYSICS_UNITS) & set(nat.UNITS)
    assert "csrc/vrt_physics.hip" in open(os.path.join(ROOT, "tools", "build_variant.sh")).read()
    import python_raytracer_amd
    assert python_raytracer_amd.PhysicsResult is not None and "PhysicsResult" in python_raytracer_amd.__all__
    assert [f for f, _ in world.PHYSICS_COUNTER_FIELDS] == fields[10:16]


def test_physics_tick_rejects_bad_arguments_without_a_device():
    """Everything the entry point can refuse is refused before its first HIP call: these calls carry made-up device
    pointers, which nothing reads."""
    L = nat.lib()
    fake = 0x1000
    good = nat.VrtPhysicsParams(1.0, 1.0, 0.1, 0.01, 10.0)

    def call(bodies=fake, n=4, models=fake, models_bytes=64, remap=fake, remap_bytes=8, matphys=fake, n_materials=3, params=good, stats=fake):
        return L.vrt_physics_tick(bodies, n, models, models_bytes, remap, remap_bytes, matphys, n_materials,
                                  C.byref(params) if params is not None else None, stats, None)

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


# ---- 4. the compiler's report of the new translation unit --------------------------------------------------------------------
def test_physics_report_is_the_saved_one():
    if not os.path.exists(kernel_report.HIPCC):
        pytest.skip("no hipcc")
    fresh = kernel_report.parse(physics_report.compile_report())
    saved = physics_report.saved()
    assert list(fresh) == list(saved) and fresh == saved
    names = [n for n in fresh if "physics_kernel" in n]
    assert len(names) == 1 and len(fresh) == 1               # one kernel: one launch per tick, the statistics cleared inside it
    fig = fresh[names[0]]
    assert fig["VGPRs Spill"] == 0 and fig["ScratchSize [bytes/lane]"] == 0 and fig["SGPRs Spill"] == 0, fig
    assert fig["VGPRs"] <= 128                               # 1024 threads are 4 waves per SIMD: 512 / 4 registers each
    # the contact terms of one pass (1024 x 2 doubles), the candidate list (1024 ints), and the body whose turn it is
    assert 1024 * 16 + 1024 * 4 <= fig["LDS Size [bytes/block]"] <= 1024 * 16 + 1024 * 4 + 1024
