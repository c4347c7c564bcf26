"""Many physics ticks at once, without a GPU: the host path (world.run) against every run recorded from the real reference
(tests/golden/physics_*.npz), in segments between the scripts' ticks, tick by tick and bit for bit; the camera attachment
(Object.set_camera, world.run(follow=)) against the reference's own under a camera that follows a falling body
(tests/golden/physics_follow.npz, tests/golden/make_physics_follow.py); the C ABI's new records and symbol, what
vrt_physics_run refuses before any HIP call, and the compiler's resource report of
python_raytracer_amd/csrc/vrt_physics_run.hip against the saved one."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import kernel_report
import physics_follow_scenes as fs
import physics_run_report
import physics_run_util as ru
import physics_scenes as ps
from python_raytracer_amd import _native as nat
from python_raytracer_amd import world
from python_raytracer_amd.lib import quaternion, vec2, vec3

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vrt.h")
HOST_SCENES = [n for n in ps.SCENES if ps.SCENES[n]["seed"] is None]


# ---- 1. the host run is the reference's --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", HOST_SCENES)
def test_host_run_is_the_references(name):
    z, spec = ps.load_fixture(name)
    objects, _, _, st = ps.project_scene(spec)
    twins, _, _, _ = ps.project_scene(spec)
    has_sprite = np.array([bool(o.sprite) for o in objects])
    cam = spec["cam"]
    cuts = ru.segments(spec)
    assert cuts[0][0] == 0 and cuts[-1][1] == spec["ticks"] and [a for a, _ in cuts[1:]] == sorted(int(k) for k in spec["script"])
    for first, last in cuts:
        ps.clear_redraw(objects), ps.clear_redraw(twins)
        cam = ps.apply_script(spec, first, objects, vec3, cam)
        ps.apply_script(spec, first, twins, vec3, cam)
        entry = ps.state(objects)
        counters, trace = world.run(objects, vec3(*cam), st, last - first, trace=True)
        assert trace.shape == (last - first, len(objects)) == counters.shape
        ru.assert_segment(z, first, trace, entry, has_sprite, name)
        # the loop of world.tick on a twin: the same counters, the same objects, the same `awake`
        for k in range(first, last):
            asleep = [o.pos.distance(vec3(*cam)) > st.dist_move for o in twins]
            assert np.array_equal(world.tick(twins, vec3(*cam), st), counters[k - first]), (name, k)
            assert np.array_equal(trace[k - first]["awake"] == 0, asleep), (name, k)
            for f, _ in world.PHYSICS_COUNTER_FIELDS:
                assert np.array_equal(trace[k - first][f], counters[k - first][f])
        got, want = ps.state(objects), ps.state(twins)
        assert all(got[f].tobytes() == want[f].tobytes() for f in got), name
    # without trace: the counters alone
    again, _, _, _ = ps.project_scene(spec)
    counters, none = world.run(again, vec3(*spec["cam"]), st, cuts[0][1])
    assert none is None and counters.shape == (cuts[0][1], len(again))


def test_the_script_ticks_are_where_the_issue_says():
    assert [a for a, _ in ru.segments(ps.SCENES["edges_vis"])] == [0, 3]
    assert [a for a, _ in ru.segments(ps.SCENES["edges_teleport"])] == [0, 2, 8]
    assert [a for a, _ in ru.segments(ps.SCENES["crowd"])] == [0, 2]
    assert all(len(ru.segments(ps.SCENES[n])) == 1 for n in HOST_SCENES if n not in ("edges_vis", "edges_teleport", "crowd"))
    assert set(ps.SCENES) - set(HOST_SCENES) == {"fraction"}
    with pytest.raises(ValueError):
        world.run([], vec3(0, 0, 0), None, 0)


# ---- 2. the camera attachment ------------------------------------------------------------------------------------------------
def follow_scene():
    z = np.load(fs.PATH)
    spec = json.loads(bytes(z["spec"]).decode())
    objects, _, _, st = ps.project_scene(spec)
    return z, spec, objects, st


def test_the_follow_fixture_shows_that_the_attachment_matters():
    """What make_physics_follow.py demanded of the reference's two runs before it wrote the file, from the file."""
    z, spec, objects, st = follow_scene()
    assert json.loads(json.dumps(fs.SCENE)) == spec
    who = spec["follow"]
    assert (z["pos"][-1] != z["fixed_final_pos"]).any(axis=1).sum() >= 2
    # held camera: the cube stops in mid-air; camera that follows: it lands, and the ball, asleep at first, wakes and falls too
    assert 13 < z["fixed_final_pos"][who][1] < 14 and 2 < z["pos"][-1][who][1] < 3 and z["pos"][-1][who][1] == z["pos"][-2][who][1]
    assert not z["awake"][0][1] and z["awake"][-1][1] and z["pos"][-1][1][1] < spec["objects"][1]["pos"][1] == z["fixed_final_pos"][1][1]
    assert not z["visible"][0][2] and z["visible"][-1][2]                      # the dot comes into view
    assert np.allclose(z["cam_start"], spec["cam"], atol=1e-9) and (z["cam_pos"][-1] != z["cam_start"]).any()


def test_set_camera_and_run_follow_are_the_references():
    z, spec, objects, st = follow_scene()
    has_sprite = np.array([bool(o.sprite) for o in objects])
    who = fs.attach(objects, vec2)
    assert who is objects[spec["follow"]] and np.array_equal(ru.bits(who.cam_pos.tuple()), ru.bits(z["cam_start"]))
    assert who.camera_offset().y == 4 and abs(who.camera_offset().x - 3) < 1e-12 and tuple(z["cam_start"]) != (3.0, 44.0, 0.0)
    ps.clear_redraw(objects)
    entry = ps.state(objects)
    # pos_cam is not used where a body is followed
    counters, trace = world.run(objects, vec3(1e6, 1e6, 1e6), st, spec["ticks"], follow=who, trace=True)
    ru.assert_segment(z, 0, trace, entry, has_sprite, "follow")
    assert np.array_equal(ru.bits(who.cam_pos.tuple()), ru.bits(z["cam_pos"][-1]))
    # tick by tick, as Window.update does it: cam_pos after every tick
    z, spec, objects, st = follow_scene()
    who = fs.attach(objects, vec2)
    for k in range(spec["ticks"]):
        ps.clear_redraw(objects)
        world.tick(objects, who.cam_pos, st)
        ps.assert_tick(z, k, objects, "follow, tick by tick")
        assert np.array_equal(ru.bits(who.cam_pos.tuple()), ru.bits(z["cam_pos"][k])), k
    # the same scene under the camera held where it started
    z, spec, objects, st = follow_scene()
    who = fs.attach(objects, vec2)
    world.run(objects, who.cam_pos, st, spec["ticks"])
    assert np.array_equal(ru.bits(ps.state(objects)["pos"]), ru.bits(z["fixed_final_pos"]))


def test_camera_fields_and_rotation():
    o = world.Object(pos=vec3(1, 2, 3))
    assert o.cam_vec == 0 and o.cam_pos.tuple() == (0, 0, 0) and o.cam_rot.array() == [0, 0, 0, 0]
    o.move(vec3(4, 5, 6))                                # no attachment: nothing follows
    assert o.cam_pos.tuple() == (0, 0, 0) and o.cam_rot.array() == [0, 0, 0, 0]
    o.set_camera(vec2(0, 0))
    assert o.cam_pos.tuple() == (0, 0, 0)
    o.set_camera(vec2(0, 2))                             # an offset straight up is an attachment too
    assert o.cam_pos.tuple() == (4, 7, 6) and o.cam_rot.array() == vec3(0, 0, 0).quaternion().array() == [0, 0, 0, 1]
    # turned a quarter about y: forward is what the rotation's quaternion says, the height is untouched
    t = world.Object(pos=vec3(10, 0, 0), rot=vec3(30, 90, 0))
    t.set_camera(vec2(8, 1))
    d = vec3(0, 90, 0).quaternion().vec_forward()
    assert t.cam_pos.tuple() == (10 + 8 * d.x, 1, 0 + 8 * d.z) and abs(d.x - 1) < 1e-12 and abs(d.z) < 1e-12
    assert t.cam_rot.array() == vec3(30, 90, 0).quaternion().array() and isinstance(t.cam_rot, quaternion)
    t.move(vec3(10, 0, 0))                               # a move to where it stands is none
    t.cam_pos = vec3(0, 0, 0)
    t.move(vec3(10, 0, 0))
    assert t.cam_pos.tuple() == (0, 0, 0)
    t.move(vec3(11, 0, 0))
    assert t.cam_pos.tuple() == (11 + 8 * d.x, 1, 0 + 8 * d.z)


# ---- 3. the C ABI ------------------------------------------------------------------------------------------------------------
def test_symbols_and_layout():
    text = open(HEADER).read()
    body = re.search(r"typedef struct vrt_body_sample \{(.*?)\} vrt_body_sample;", text, re.S).group(1)
    assert re.findall(r"(\w+)(?:\[\d\])?[,;]", re.sub(r"/\*.*?\*/", "", body)) == ["pos", "vel", "mins", "maxs", "visible", "awake", "out"]
    fields = ["pos", "vel", "mins", "maxs", "visible", "awake", "out"]
    offsets = [0, 24, 48, 60, 72, 76, 80]
    assert [getattr(nat.VrtBodySample, f).offset for f in fields] == offsets and C.sizeof(nat.VrtBodySample) == 104 == nat.BODY_SAMPLE_BYTES
    dt = np.dtype(nat.BODY_SAMPLE_FIELDS)
    assert dt.itemsize == 104 and [dt.fields[f][1] for f in fields[:6]] == offsets[:6]
    assert [dt.fields[f][1] for f, _ in world.PHYSICS_COUNTER_FIELDS] == [80 + 4 * i for i in range(6)]
    run = ["cam", "offset", "dist_max", "dist_move", "budget", "n_ticks", "follow"]
    assert [f for f, _ in nat.VrtPhysicsRunParams._fields_] == run and C.sizeof(nat.VrtPhysicsRunParams) == 80
    assert [getattr(nat.VrtPhysicsRunParams, f).offset for f in run] == [0, 24, 48, 56, 64, 72, 76]
    body = re.search(r"typedef struct vrt_physics_run_params \{(.*?)\} vrt_physics_run_params;", text, re.S).group(1)
    assert re.findall(r"^\s+(?:double|int32_t|int64_t)\s+(\w+)", body, re.M) == run
    assert re.search(r"int vrt_physics_run\(vrt_body\* d_bodies, int32_t n_bodies, const uint8_t\* d_models, int64_t models_bytes,\s+"
                     r"const uint8_t\* d_remap, int32_t remap_bytes, const double\* d_matphys, int32_t n_materials,\s+"
                     r"const vrt_physics_params\* params, const vrt_physics_run_params\* run, vrt_body_sample\* d_trace,\s+"
                     r"uint64_t\* d_stats, void\* stream\);", text)
    assert re.search(r"VRT_S_PHYSICS_WORK = 5\b", text) and re.search(r"VRT_S_PHYSICS_TICKS = 6\b", text)
    assert (nat.S_PHYSICS_WORK, nat.S_PHYSICS_TICKS) == (5, 6)
    assert "#define VRT_PHYSICS_RUN_BUDGET %d\n" % nat.PHYSICS_RUN_BUDGET in text
    assert "fractional solidity is not solid" in text          # the run makes no draws, and the header says so
    assert "#define VRT_ABI_VERSION 9" in text
    L = nat.lib()
    assert L.vrt_abi_version() == 9 and nat.ABI_VERSION == 9      # the change only adds a symbol
    assert L.vrt_physics_run is not None and "vrt_physics_run" in nat.EXPORTS
    # the build: a unit of its own list, in the one library, counted by needs_build(), and in the variant build
    assert [os.path.basename(u) for u in nat.PHYSICS_RUN_UNITS] == ["vrt_physics_run.hip"] and set(nat.PHYSICS_RUN_UNITS) <= set(nat.SOURCES)
    assert not set(nat.PHYSICS_RUN_UNITS) & set(nat.UNITS + nat.PHYSICS_UNITS + nat.PHYSICS_DRAWS_UNITS)
    assert [os.path.basename(u) for u in nat.PHYSICS_UNITS] == ["vrt_physics.hip"]
    assert [os.path.basename(u) for u in nat.PHYSICS_DRAWS_UNITS] == ["vrt_physics_draws.hip"]
    assert "csrc/vrt_physics_run.hip" in open(os.path.join(ROOT, "tools", "build_variant.sh")).read()
    import python_raytracer_amd
    assert python_raytracer_amd.RunResult is not None and "RunResult" in python_raytracer_amd.__all__


def test_physics_run_rejects_bad_arguments_without_a_device():
    """Everything the entry point can refuse is refused before its first HIP call: these calls carry made-up device
    pointers, which nothing reads."""
    L = nat.lib()
    fake = 0x1000
    good = nat.VrtPhysicsParams(1.0, 1.0, 0.1, 0.01, 10.0)

    def run_params(**change):
        rp = nat.VrtPhysicsRunParams((C.c_double * 3)(0.0, 4.0, 3.0), (C.c_double * 3)(0.0, 4.0, 3.0), 40.0, 24.0, 1 << 16, 8, 2)
        for k, v in change.items():
            if k in ("cam", "offset"):
                getattr(rp, k)[v[0]] = v[1]
            else:
                setattr(rp, k, v)
        return rp

    def call(bodies=fake, n=4, models=fake, models_bytes=64, remap=fake, remap_bytes=8, matphys=fake, n_materials=3, params=good,
             run=run_params(), trace=fake, stats=fake):
        return L.vrt_physics_run(bodies, n, models, models_bytes, remap, remap_bytes, matphys, n_materials,
                                 C.byref(params) if params is not None else None, C.byref(run) if run is not None else None, trace, stats, None)

    # the tick's refusals
    assert call(stats=None) == -1 and call(stats=None, n=0, run=run_params(follow=-1)) == -1 and call(params=None) == -1 and call(stats=fake + 4) == -1
    assert call(n=-1) == -1 and call(n=(1 << 20) + 1) == -1
    assert call(bodies=None) == -1 and call(bodies=fake + 4) == -1 and call(matphys=None) == -1 and call(matphys=fake + 4) == -1
    assert call(models=None) == -1 and call(remap=None) == -1 and call(models_bytes=-1) == -1 and call(remap_bytes=-1) == -1
    assert call(n_materials=-1) == -1 and call(n_materials=256) == -1
    bad = nat.VrtPhysicsParams(1.0, 1.0, float("nan"), 0.01, 10.0)
    assert call(params=bad) == -1
    # ... and the run's own
    assert call(run=None) == -1
    assert call(run=run_params(n_ticks=0)) == -1 and call(run=run_params(n_ticks=-3)) == -1
    assert call(run=run_params(budget=0)) == -1 and call(run=run_params(budget=-1)) == -1
    assert call(run=run_params(follow=-2)) == -1 and call(run=run_params(follow=4)) == -1 and call(n=0, run=run_params(follow=0)) == -1
    for value in (float("nan"), float("inf"), float("-inf")):
        for axis in range(3):
            assert call(run=run_params(cam=(axis, value))) == -1 and call(run=run_params(offset=(axis, value))) == -1
        assert call(run=run_params(dist_max=value)) == -1 and call(run=run_params(dist_move=value)) == -1
    assert call(trace=fake + 4) == -1 and call(trace=fake + 1) == -1


# ---- 4. the compiler's report of the new translation unit --------------------------------------------------------------------
def test_physics_run_report_is_the_saved_one():
    if not os.path.exists(kernel_report.HIPCC):
        pytest.skip("no hipcc")
    fresh = kernel_report.parse(physics_run_report.compile_report())
    saved = physics_run_report.saved()
    assert list(fresh) == list(saved) and fresh == saved
    names = [n for n in fresh if "physics_run_kernel" in n]
    assert len(names) == 1 and len(fresh) == 1               # one kernel: one launch for many ticks, the statistics cleared inside it
    fig = fresh[names[0]]
    assert fig["VGPRs Spill"] == 0 and fig["ScratchSize [bytes/lane]"] == 0, fig     # no vector spills, no scratch
    assert fig["VGPRs"] <= 128                               # 1024 threads are 4 waves per SIMD: 512 / 4 registers each
    # the LDS of the tick's kernel exactly: the run adds registers, not shared state
    import physics_report
    tick = list(physics_report.saved().values())[0]
    assert fig["LDS Size [bytes/block]"] == tick["LDS Size [bytes/block]"]
