"""What-if runs, without a GPU: the host form (world.run_many) against the recorded reference and against world.run on hand-made
twins, bit for bit, with the caller's objects left alone; what `variants` refuses; the C ABI's new symbol, what
vrt_physics_run_batch refuses before any HIP call, and the compiler's resource report of
python_raytracer_amd/csrc/vrt_physics_batch.hip against the saved one."""
import os
import re

import numpy as np
import pytest

import kernel_report
import physics_batch_report
import physics_batch_util as bu
import physics_run_util as ru
import physics_scenes as ps
from python_raytracer_amd import _native as nat
from python_raytracer_amd import world
from python_raytracer_amd.lib import vec3

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vrt.h")


def same_state(a, b):
    sa, sb = ps.state(a), ps.state(b)
    return all(sa[f].tobytes() == sb[f].tobytes() for f in sa)


# ---- 1. the host form is the loop --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["default", "edges_ties"])
def test_host_run_many_is_the_loop_of_runs(name):
    z, spec = ps.load_fixture(name)
    objects, _, _, st = ps.project_scene(spec)
    has_sprite = np.array([bool(o.sprite) for o in objects])
    first, last = ru.segments(spec)[0]
    assert first == 0
    ps.clear_redraw(objects)
    objects[0].redraw = True                                   # a flag that is set stays set, in the copies and here
    entry = ps.state(objects)
    cam = vec3(*spec["cam"])
    changes = bu.changes(objects, spec["cam"])[:5]                          # {} and a moved body, a thrown body, both, two bodies
    assert changes[0] == {} and [len(c) for c in changes[1:]] == [1, 1, 1, 2] and set(changes[3][min(changes[3])]) == {"pos", "vel"}
    got = world.run_many(objects, cam, st, last, [bu.mapping(objects, c) for c in changes], trace=True)
    assert len(got) == 5
    after = ps.state(objects)
    assert all(entry[f].tobytes() == after[f].tobytes() for f in entry)          # the caller's objects: untouched, redraw included
    # variant {}: the reference's record (the flag set above is not the fixture's)
    entry["redraw"][0] = False
    rows = got[0][2].copy()
    ru.assert_segment(z, 0, rows, entry, has_sprite, name + " (run_many, {})")
    finals = set()
    for change, (copies, counters, states) in zip(changes, got):
        assert all(c is not o and c.sprite is o.sprite and c.pos is not o.pos for c, o in zip(copies, objects))
        twin = bu.altered(objects, change)
        want_counters, want_states = world.run(twin, cam, st, last, trace=True)
        assert ru.same_records(counters, want_counters) and ru.same_records(states, want_states), (name, change)
        assert same_state(copies, twin), (name, change)
        finals.add(states[-1]["pos"].tobytes() + states[-1]["vel"].tobytes())
    assert len(finals) == 5                                    # five different futures
    # without trace, and with a followed body
    (copies, counters, none), = world.run_many(objects, cam, st, 2, [{}])
    assert none is None and counters.shape == (2, len(objects))


def test_host_run_many_follows_each_copy_of_the_body():
    import json
    import physics_follow_scenes as fs
    from python_raytracer_amd.lib import vec2
    z = np.load(fs.PATH)
    spec = json.loads(bytes(z["spec"]).decode())
    objects, _, _, st = ps.project_scene(spec)
    who = fs.attach(objects, vec2)
    ps.clear_redraw(objects)
    entry = ps.state(objects)
    far = vec3(1e6, 1e6, 1e6)
    changes = [{}, {fs.FOLLOW: dict(vel=(0, 0, 1.5))}, {fs.FOLLOW: dict(pos=(40, 40, 0))}]
    got = world.run_many(objects, far, st, spec["ticks"], [bu.mapping(objects, c) for c in changes], follow=who, trace=True)
    ru.assert_segment(z, 0, got[0][2], entry, np.array([bool(o.sprite) for o in objects]), "follow (run_many)")
    assert np.array_equal(ru.bits(got[0][0][fs.FOLLOW].cam_pos.tuple()), ru.bits(z["cam_pos"][-1]))
    assert np.array_equal(ru.bits(who.cam_pos.tuple()), ru.bits(z["cam_start"]))
    for change, (copies, counters, states) in zip(changes, got):
        twin = bu.altered(objects, change)
        _, want = world.run(twin, far, st, spec["ticks"], follow=twin[fs.FOLLOW], trace=True)
        assert ru.same_records(states, want) and same_state(copies, twin)
        assert copies[fs.FOLLOW].cam_pos.tuple() == twin[fs.FOLLOW].cam_pos.tuple()
    # carried out of dist_move of the ball, the camera never wakes it
    assert got[0][2][:, 1]["awake"].any() and not got[2][2][:, 1]["awake"].any()
    with pytest.raises(ValueError, match="not one of"):
        world.run_many(objects[:2], far, st, 2, [{}], follow=who)


# ---- 2. what `variants` refuses ----------------------------------------------------------------------------------------------
def test_variants_errors():
    _, spec = ps.load_fixture("edges_tiny")
    objects, _, _, st = ps.project_scene(spec)
    foreign, _, _, _ = ps.project_scene(spec)
    cam = vec3(*spec["cam"])
    before = ps.state(objects)
    bad = [{foreign[1]: {"vel": vec3(1, 0, 0)}},
           {objects[1]: {"velocity": vec3(1, 0, 0)}},
           {objects[1]: {"pos": vec3(0, float("nan"), 0)}},
           {objects[1]: {"vel": vec3(float("inf"), 0, 0)}}]
    for variant in bad:
        with pytest.raises(ValueError):
            world.run_many(objects, cam, st, 2, [{}, variant])
        with pytest.raises(ValueError):
            world._variants(objects, [variant], "DeviceWorld.run_many()")      # the one check both forms make
    after = ps.state(objects)
    assert all(before[f].tobytes() == after[f].tobytes() for f in before)
    # what the device would refuse is no error here: the host steps it
    out = world.run_many(objects, cam, st, 1, [{objects[1]: {"vel": vec3(0, -1025, 0)}}])
    assert out[0][1][0][1]["status"] == 0


# ---- 3. the C ABI ------------------------------------------------------------------------------------------------------------
def test_symbol_and_units():
    text = open(HEADER).read()
    assert "#define VRT_ABI_VERSION 9" in text
    L = nat.lib()
    assert L.vrt_abi_version() == 9 and nat.ABI_VERSION == 9      # the change only adds a symbol
    assert L.vrt_physics_run_batch is not None and "vrt_physics_run_batch" in nat.EXPORTS and nat.EXPORTS[-1] != "vrt_physics_run_batch"
    assert re.search(r"int vrt_physics_run_batch\(vrt_body\* d_bodies, int32_t n_runs, int32_t n_bodies, const uint8_t\* d_models, int64_t models_bytes,\s+"
                     r"const uint8_t\* d_remap, int32_t remap_bytes, const double\* d_matphys, int32_t n_materials,\s+"
                     r"const vrt_physics_params\* params, const vrt_physics_run_params\* run, int32_t\* d_ticks_done,\s+"
                     r"vrt_body_sample\* d_trace, uint64_t\* d_stats, void\* stream\);", text)
    assert re.search(r"VRT_S_PHYSICS_BATCH_BADTICK = %d\b" % nat.S_PHYSICS_BATCH_BADTICK, text)
    assert "#define VRT_PHYSICS_BATCH_MAX_RUNS %d\n" % nat.PHYSICS_BATCH_MAX_RUNS in text and nat.PHYSICS_BATCH_MAX_RUNS == 4096
    # a word no other physics call writes
    taken = {nat.S_PHYSICS_WORK, nat.S_PHYSICS_TICKS, nat.S_PHYSICS_RNG_INVALID, nat.S_PHYSICS_DRAWS, nat.S_PHYSICS_BODIES,
             nat.S_PHYSICS_REFUSED, nat.S_PHYSICS_STEPS, nat.S_PHYSICS_BLOCKED, nat.S_PHYSICS_CONTACTS, nat.S_PHYSICS_TRANSFERS,
             nat.S_PHYSICS_CAPPED}
    assert nat.S_PHYSICS_BATCH_BADTICK not in taken and 0 <= nat.S_PHYSICS_BATCH_BADTICK < nat.NSTATS
    assert [os.path.basename(u) for u in nat.PHYSICS_BATCH_UNITS] == ["vrt_physics_batch.hip"] and set(nat.PHYSICS_BATCH_UNITS) <= set(nat.SOURCES)
    assert "csrc/vrt_physics_batch.hip" in open(os.path.join(ROOT, "tools", "build_variant.sh")).read()
    # the other physics units' file lists are as they were
    lists = [nat.PHYSICS_UNITS, nat.PHYSICS_DRAWS_UNITS, nat.PHYSICS_RUN_UNITS, nat.PHYSICS_ANIM_UNITS, nat.PHYSICS_RUN_DRAWS_UNITS]
    assert [[os.path.basename(u) for u in units] for units in lists] == [["vrt_physics.hip"], ["vrt_physics_draws.hip"], ["vrt_physics_run.hip"],
                                                                        ["vrt_physics_anim.hip"], ["vrt_physics_run_draws.hip"]]
    assert not set(nat.PHYSICS_BATCH_UNITS) & set(nat.UNITS + nat.CHUNK_LISTS_UNITS + sum(lists, []))
    import python_raytracer_amd
    assert python_raytracer_amd.BatchRunResult is not None and "BatchRunResult" in python_raytracer_amd.__all__


def test_physics_run_batch_rejects_bad_arguments_without_a_device():
    bu.assert_refusals(nat.lib())


# ---- 4. the compiler's report of the new translation unit --------------------------------------------------------------------
def test_physics_batch_report_is_the_saved_one():
    if not os.path.exists(kernel_report.HIPCC):
        pytest.skip("no hipcc")
    fresh = kernel_report.parse(physics_batch_report.compile_report())
    saved = physics_batch_report.saved()
    assert list(fresh) == list(saved) and fresh == saved
    names = [n for n in fresh if "physics_batch_kernel" in n]
    assert len(names) == 1 and len(fresh) == 1               # one kernel: one launch for all runs, the statistics cleared inside it
    fig = fresh[names[0]]
    assert fig["VGPRs Spill"] == 0 and fig["ScratchSize [bytes/lane]"] == 0, fig     # no vector spills, no scratch
    assert fig["Occupancy [waves/SIMD]"] >= 4                # 1024 threads are 4 waves per SIMD: a run's workgroup fits a CU
    # the LDS of the run's kernel exactly: a batch adds a grid, not shared state
    import physics_run_report
    run = list(physics_run_report.saved().values())[0]
    assert fig["LDS Size [bytes/block]"] == run["LDS Size [bytes/block]"]
