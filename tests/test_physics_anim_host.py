"""Sprite animation during a physics run, without a GPU: Sprite.frame_at against the table recorded from the real reference's
anim_update; the host path (world.run(clock=)) against every tick of every scene of tests/golden/physics_anim.npz
(tests/golden/make_physics_anim.py, tests/physics_anim_scenes.py), bit for bit, weights and frames included; world.run without
a clock against the recording under a held clock; what run(clock=) refuses; the C ABI's new symbol and records; and the
compiler's resource report of python_raytracer_amd/csrc/vrt_physics_anim.hip against the saved one."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import kernel_report
import physics_anim_report
import physics_anim_scenes as an
import physics_run_util as ru
import physics_scenes as ps
from python_raytracer_amd import _native as nat
from python_raytracer_amd import world
from python_raytracer_amd.lib import vec3

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vrt.h")


# ---- 1. the clock ------------------------------------------------------------------------------------------------------------
def test_frame_at_is_the_references_anim_update():
    z, _ = an.load_fixture()
    rows = list(zip(z["table_anim"], z["table_now"], z["table_frame"]))
    assert len(rows) == len(an.TABLE_ANIMS) * len(an.TABLE_NOWS)
    assert [tuple(a) for a in z["table_anim"][::len(an.TABLE_NOWS)]] == [tuple(float(v) for v in a) for a in an.TABLE_ANIMS]
    # what the issue asks the table to cover
    times = z["table_anim"][:, 2]
    assert (times < 0).any() and (times != np.round(times)).any() and (np.abs(times) <= 1e-9).any() and z["table_now"].max() >= 2 ** 40
    spr = world.Sprite(frames=an.TABLE_FRAMES)
    for (first, last, ft), now, frame in rows:
        spr.anim_set(int(first), int(last), float(ft))
        assert spr.frame == 0 and spr.frame_time == float(ft) * 1000 and (spr.frame_start, spr.frame_end) == (int(first), int(last))
        assert spr.frame_at(int(now)) == int(frame), (first, last, ft, now)
        spr.anim_update(int(now))
        assert spr.frame == int(frame) and isinstance(spr.frame, int)
    assert len(set(z["table_frame"].tolist())) == an.TABLE_FRAMES


def test_anim_set_clips_as_the_reference_and_anim_update_needs_frames_and_a_time():
    spr = world.Sprite(frames=3)
    assert (spr.frame, spr.frame_time, spr.frame_start, spr.frame_end) == (0, 0, 0, 0) and not spr.animated
    spr.anim_update(12345)
    assert spr.frame == 0                                         # no frame time: nothing plays
    spr.frame = 2
    spr.anim_set(7, 9, 0.25)
    assert (spr.frame, spr.frame_time, spr.frame_start, spr.frame_end) == (0, 250.0, 3, 3) and spr.animated    # len(frames), as data.py:300-301
    one = world.Sprite(frames=1)
    one.anim_set(0, 0, 1)
    one.anim_update(5000)
    assert one.frame == 0 and not one.animated and one.frame_time == 1000


# ---- 2. the host run is the reference's ------------------------------------------------------------------------------------
def test_the_fixture_holds_the_scenes_and_what_they_are_for():
    z, specs = an.load_fixture()
    assert specs == json.loads(json.dumps(an.SCENES))
    assert os.path.getsize(an.PATH) <= max(os.path.getsize(ps.fixture_path(n)) for n in ps.SCENES)
    for name, spec in specs.items():
        n = len(spec["objects"])
        assert (n <= 8 and spec["ticks"] <= 40) or (name == "crowd" and 1024 < n <= 1040 and spec["ticks"] == 3)
        assert all(max(s["size"]) <= 12 for s in spec["sprites"].values())
        assert z[name + "/weight"].shape == (spec["ticks"], n) and z[name + "/frame"].shape == (spec["ticks"], len(spec["sprites"]))
        assert z[name + "/frame"].any() and (z[name + "/pos"][-1] != z[name + "/held_pos"][-1]).any()     # (1) it switches, and that matters
    # (2) the stale weight: the twins of `weights` weigh differently, and fall differently afterwards
    w, v = z["weights/weight"], z["weights/vel"]
    apart = np.nonzero(w[:, 0] != w[:, 1])[0]
    assert len(apart) and (w[:, 1] == z["weights/weight0"][1]).all() and (v[apart[0] + 1:, 0, 1] != v[apart[0] + 1:, 1, 1]).any()
    # (3) asleep: the lamp of `wake` stays behind its schedule; (5) `weights` plays backwards: 0, 2, 1
    lamp = world.Sprite(frames=2)
    lamp.anim_set(*specs["wake"]["sprites"]["lamp"]["anim"])
    start, step = specs["wake"]["clock"]
    due = [lamp.frame_at(start + k * step) for k in range(specs["wake"]["ticks"])]
    assert (z["wake/frame"][:, 0] != due).any() and z["wake/frame"][-1, 0] == due[-1]
    assert specs["weights"]["sprites"]["blob"]["anim"][2] < 0
    played = [f for i, f in enumerate(z["weights/frame"][:, 0].tolist()) if i == 0 or f != z["weights/frame"][i - 1, 0]]
    assert played[:4] == [2, 1, 0, 2]
    # (6) the platform is not physical, never moves, and after the tick that shows it has `redraw` exactly where its frame changes
    f = z["platform/frame"][:, 0]
    assert not specs["platform"]["objects"][1]["physics"] and np.array_equal(z["platform/redraw"][1:, 1], np.diff(f) != 0)
    assert (np.diff(f) != 0).sum() >= 2 and (z["platform/pos"][:, 1] == 0).all()
    # the crowd: the switching body beyond 1024, sharers on both sides, and both movers end elsewhere than under the held clock
    R = an.CROWD_ROLES
    assert R["blink_low"] < R["mover_low"] < 1024 < R["switcher"] < R["mover_high"] < R["blink_high"]
    assert z["crowd/redraw"][1][R["switcher"]] and not z["crowd/redraw"][1][[R["blink_low"], R["blink_high"]]].any()
    assert all((z["crowd/pos"][-1][R[m]] != z["crowd/held_pos"][-1][R[m]]).any() for m in ("mover_low", "mover_high"))


@pytest.mark.parametrize("name", list(an.SCENES))
def test_host_run_with_a_clock_is_the_references(name):
    z, spec, objects, sprites, st, who = an.fresh(name)
    out = world.run(objects, vec3(*spec["cam"]), st, spec["ticks"], follow=who, trace=True, clock=tuple(spec["clock"]))
    assert len(out) == 3
    counters, trace, anim = out
    assert trace.shape == anim.shape == counters.shape == (spec["ticks"], len(objects)) and anim.dtype == np.dtype(nat.ANIM_SAMPLE_FIELDS)
    an.assert_ticks(z, name, spec, objects, sprites, trace, anim, name)
    # (4) in the tick of a switch the bodies before the switching one met the old frame: they did not see `switched` bodies' new one
    # -- the fixture generator replays the scenes with the switch made early and demands another end; here, tick by tick with
    # world.tick(now=), the same objects come out
    z, spec, twins, twin_sprites, st, who = an.fresh(name)
    start, step = spec["clock"]
    for k in range(spec["ticks"]):
        cam = who.cam_pos if who is not None else vec3(*spec["cam"])
        assert np.array_equal(world.tick(twins, cam, st, now=start + k * step), counters[k]), (name, k)
        assert [bool(o.last_switched) for o in twins] == (anim[k]["switched"] != 0).tolist()
    got, want = ps.state(objects), ps.state(twins)
    assert all(got[f].tobytes() == want[f].tobytes() for f in got if f != "redraw"), name
    # without trace
    z, spec, again, _, st, who = an.fresh(name)
    counters2, none, none2 = world.run(again, vec3(*spec["cam"]), st, spec["ticks"], follow=who, clock=tuple(spec["clock"]))
    assert none is None and none2 is None and np.array_equal(counters2, counters)


@pytest.mark.parametrize("name", list(an.SCENES))
def test_host_run_without_a_clock_is_unchanged(name):
    z, spec, objects, sprites, st, who = an.fresh(name)
    out = world.run(objects, vec3(*spec["cam"]), st, spec["ticks"], follow=who, trace=True)
    assert len(out) == 2
    held_pos, held_vel = z[name + "/held_pos"], z[name + "/held_vel"]
    assert len(held_pos) in (1, spec["ticks"])
    assert np.array_equal(ru.bits(out[1]["pos"][-len(held_pos):]), ru.bits(held_pos))
    assert np.array_equal(ru.bits(out[1]["vel"][-len(held_vel):]), ru.bits(held_vel))
    assert all(s.frame == 0 for s in sprites.values())
    assert np.array_equal(ru.bits([float(o.weight) for o in objects]), ru.bits(z[name + "/weight0"]))
    # tick() and update() without a clock: no frame changes either
    world.tick(objects, vec3(*spec["cam"]), st)
    objects[0].update(vec3(*spec["cam"]), st, objects)
    assert all(s.frame == 0 for s in sprites.values()) and not objects[0].last_switched


# ---- 3. what a run with a clock refuses -------------------------------------------------------------------------------------
def test_run_refuses_ranges_outside_the_frames_and_bad_clocks():
    z, spec, objects, sprites, st, who = an.fresh("platform")
    cam = vec3(*spec["cam"])
    before = ps.state(objects)
    plat = sprites["plat"]
    for first, last in ((0, 2), (1, 5), (2, 1), (-1, 1), (0, 1.0), (0.0, 1), (True, 1)):
        plat.anim_set(0, 1, 0.2)
        plat.frame_start, plat.frame_end = first, last
        with pytest.raises(ValueError, match="frame_start"):
            world.run(objects, cam, st, 2, clock=(0, 50))
    plat.anim_set(0, 2, 0.2)                                  # clipped to len(frames) = 2: one past the last frame
    with pytest.raises(ValueError):
        world.run(objects, cam, st, 2, clock=(0, 50))
    plat.anim_set(0, 1, 0.2)
    for clock in ((-1, 50), (0, -50), (0.0, 50), (0, 50.0), (0,), (0, 50, 1), 50, "ab", (True, 1)):
        with pytest.raises(ValueError, match="clock"):
            world.run(objects, cam, st, 2, clock=clock)
    after = ps.state(objects)
    assert all(before[f].tobytes() == after[f].tobytes() for f in before) and plat.frame == 0        # nothing moved
    # a range that is no animation (no frame time) is not judged; a step of 0 holds the clock
    plat.anim_set(5, 9, 0)
    world.run(objects, cam, st, 1, clock=(0, 0))
    plat.anim_set(0, 1, 0.2)
    world.run(objects, cam, st, 2, clock=(np.int64(200), np.int32(0)))
    assert plat.frame == 1


# ---- 4. the C ABI -----------------------------------------------------------------------------------------------------------
def struct_fields(text, name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, re.S).group(1)
    return re.findall(r"^\s+(double|int32_t|int64_t)\s+(\w+);", re.sub(r"/\*.*?\*/", "", body), re.M)


def test_symbol_and_layout():
    text = open(HEADER).read()
    ctype = {"double": C.c_double, "int32_t": C.c_int32, "int64_t": C.c_int64}
    dtype = {"double": "<f8", "int32_t": "<i4", "int64_t": "<i8"}
    for name, cls, fields, size in (("vrt_anim_sprite", nat.VrtAnimSprite, nat.ANIM_SPRITE_FIELDS, nat.ANIM_SPRITE_BYTES),
                                    ("vrt_anim_frame", nat.VrtAnimFrame, nat.ANIM_FRAME_FIELDS, nat.ANIM_FRAME_BYTES),
                                    ("vrt_anim_sample", nat.VrtAnimSample, nat.ANIM_SAMPLE_FIELDS, nat.ANIM_SAMPLE_BYTES)):
        declared = struct_fields(text, name)
        assert [(f, ctype[t]) for t, f in declared] == list(cls._fields_), name
        assert [(f, dtype[t]) for t, f in declared] == list(fields), name
        dt = np.dtype(fields)
        assert C.sizeof(cls) == dt.itemsize == size and "%d bytes" % size in re.search(r"typedef struct %s \{(.*)" % name, text).group(1)
        assert [getattr(cls, f).offset for f, _ in fields] == [dt.fields[f][1] for f, _ in fields]     # (no padding in either)
    assert (nat.ANIM_SPRITE_BYTES, nat.ANIM_FRAME_BYTES, nat.ANIM_SAMPLE_BYTES) == (16, 32, 16)
    assert re.search(r"int vrt_physics_run_anim\(vrt_body\* d_bodies, int32_t n_bodies, const uint8_t\* d_models, int64_t models_bytes,\s+"
                     r"const uint8_t\* d_remap, int32_t remap_bytes, const double\* d_matphys, int32_t n_materials,\s+"
                     r"const vrt_physics_params\* params, const vrt_physics_run_params\* run, vrt_body_sample\* d_trace,\s+"
                     r"uint64_t\* d_stats, void\* stream, const int32_t\* d_body_sprite, vrt_anim_sprite\* d_sprites,\s+"
                     r"int32_t n_sprites, const vrt_anim_frame\* d_frames, int32_t n_frame_rows, const int32_t\* d_schedule,\s+"
                     r"vrt_anim_sample\* d_anim_trace\);", text)
    assert "#define VRT_ABI_VERSION 9" in text and nat.BODY_EVER_SWITCHED == 4
    L = nat.lib()
    assert L.vrt_abi_version() == 9 and nat.ABI_VERSION == 9      # the change only adds a symbol
    assert L.vrt_physics_run_anim is not None and nat.EXPORTS[-1] == "vrt_physics_run_anim"
    assert C.sizeof(nat.VrtBody) == 192                           # the body record is what it was
    # the build: the sixth unit of the one library, counted by needs_build(), and in the variant build
    assert [os.path.basename(u) for u in nat.PHYSICS_ANIM_UNITS] == ["vrt_physics_anim.hip"] and set(nat.PHYSICS_ANIM_UNITS) <= set(nat.SOURCES)
    units = nat.UNITS + nat.PHYSICS_UNITS + nat.PHYSICS_DRAWS_UNITS + nat.PHYSICS_RUN_UNITS
    assert len(units) == 5 and not set(nat.PHYSICS_ANIM_UNITS) & set(units)
    assert "csrc/vrt_physics_anim.hip" in open(os.path.join(ROOT, "tools", "build_variant.sh")).read()
    import python_raytracer_amd
    assert python_raytracer_amd.RunResult is not None


def test_physics_run_anim_rejects_bad_arguments_without_a_device():
    """Everything the entry point can refuse is refused before its first HIP call: these calls carry made-up device
    pointers, which nothing reads."""
    L = nat.lib()
    fake = 0x1000
    good = nat.VrtPhysicsParams(1.0, 1.0, 0.1, 0.01, 10.0)

    def call(n=4, run_ticks=8, trace=fake, body_sprite=fake, sprites=fake, n_sprites=2, frames=fake, n_rows=4, schedule=fake, anim_trace=fake,
             stats=fake):
        rp = nat.VrtPhysicsRunParams((C.c_double * 3)(0.0, 4.0, 3.0), (C.c_double * 3)(0.0, 4.0, 3.0), 40.0, 24.0, 1 << 16, run_ticks, 2)
        return L.vrt_physics_run_anim(fake, n, fake, 64, fake, 8, fake, 3, C.byref(good), C.byref(rp), trace, stats, None,
                                      body_sprite, sprites, n_sprites, frames, n_rows, schedule, anim_trace)

    # vrt_physics_run's refusals are this call's
    assert call(stats=None) == -1 and call(n=-1) == -1 and call(run_ticks=0) == -1 and call(trace=fake + 4) == -1
    # ... and its own: negative counts, NULL or misaligned arrays while there are sprites
    assert call(n_sprites=-1) == -1 and call(n_rows=-1) == -1 and call(n_sprites=0, n_rows=-1) == -1
    assert call(sprites=None) == -1 and call(schedule=None) == -1 and call(body_sprite=None) == -1 and call(frames=None) == -1
    assert call(sprites=fake + 2) == -1 and call(schedule=fake + 1) == -1 and call(body_sprite=fake + 3) == -1
    assert call(frames=fake + 4) == -1 and call(anim_trace=fake + 4) == -1 and call(anim_trace=fake + 4, n_sprites=0) == -1


# ---- 5. the compiler's report of the new translation unit -------------------------------------------------------------------
def test_physics_anim_report_is_the_saved_one():
    if not os.path.exists(kernel_report.HIPCC):
        pytest.skip("no hipcc")
    fresh_report = kernel_report.parse(physics_anim_report.compile_report())
    saved = physics_anim_report.saved()
    assert list(fresh_report) == list(saved) and fresh_report == saved
    names = [n for n in fresh_report if "physics_anim_kernel" in n]
    assert len(names) == 1 and len(fresh_report) == 1           # one kernel: the run's launch, with the switch inside it
    fig = fresh_report[names[0]]
    assert fig["VGPRs Spill"] == 0 and fig["ScratchSize [bytes/lane]"] == 0, fig     # no vector spills, no scratch
    assert fig["VGPRs"] <= 128                               # 1024 threads are 4 waves per SIMD: 512 / 4 registers each
    assert fig["Occupancy [waves/SIMD]"] >= 4
    # the run's LDS and one frame row with the word that says which sprite switches
    import physics_run_report
    run = list(physics_run_report.saved().values())[0]
    assert 0 < fig["LDS Size [bytes/block]"] - run["LDS Size [bytes/block]"] <= 64
