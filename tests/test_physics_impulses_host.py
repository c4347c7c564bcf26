"""Scripted accelerations on the host (world.run(impulses=), world.run_many(impulses=) and the "impulses" key of a variant), held
bit for bit to the real reference through tests/golden/physics_impulses.npz -- its Object.accelerate called between its own ticks
-- and to the hand-written loop they replace; the merge order of a batch; the ValueErrors; the header, the constants and the
build; what the entry point refuses before any HIP call; and the compiler's report of the new translation unit against the saved
one.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import kernel_report
import physics_impulse_scenes as sc
import physics_impulses_report
import physics_impulses_util as iu
import physics_scenes as ps
from python_raytracer_amd import _native as nat
from python_raytracer_amd import world
from python_raytracer_amd.lib import vec3

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. the host's run is the reference's, and the loop it replaces ------------------------------------------------------------
@pytest.mark.parametrize("key", iu.RUNS)
def test_run_with_impulses_is_the_references_bit_for_bit(key):
    objects, states, draws, _ = iu.play(key, iu.host_runner)
    iu.assert_is_fixture(key, states, draws, per_tick=False)
    z = iu.fixture()[key]
    assert np.array_equal(ps.state(objects)["vel"].view(np.uint64), z["vel"][-1].view(np.uint64))    # ... and so are the objects


def test_the_fixture_shows_what_its_scenes_are_named_for():
    z = np.load(sc.PATH)
    reached = __import__("json").loads(bytes(z["reached"]).decode())
    assert len(reached) >= 18 and all(reached.values()), reached
    f = iu.fixture()
    assert f["order"]["vel"][-1, 0, 0] == 1.0 and f["order@reversed"]["vel"][-1, 0, 0] == 1.0 + 2.0 ** -52
    assert os.path.getsize(sc.PATH) <= 400000
    # ... in the layout the device takes: what the scripts of the scenes become
    rows, first = world.impulse_rows([[(t, 0, v) for t, _, v in sc.impulses_of(sc.ORDER, [None, None])]])
    assert rows.dtype.itemsize == nat.IMPULSE_BYTES and first.tolist() == [0, 4] and rows["tick"].tolist() == [2] * 4


@pytest.mark.parametrize("key", iu.SCENES)
def test_run_with_impulses_is_the_hand_written_loop(key):
    a, states, draws, _ = iu.play(key, iu.host_runner)
    b, by_hand, draws2, _ = iu.play(key, iu.by_hand(iu.host_plain))
    assert iu.same_records(states, by_hand) and iu.same_state(a, b)
    assert draws is None or int(draws.sum()) == int(draws2.sum())


# ---- 2. a batch: per-variant and shared impulses -------------------------------------------------------------------------------
def test_run_many_is_run_on_twins_and_leaves_the_callers_objects_alone():
    spec, objects, st, cam, variants, shared = iu.jump_batch()
    ticks = spec["ticks"]
    entry = ps.state(objects)
    out = world.run_many(objects, cam, st, ticks, [iu.variant_mapping(objects, v) for v in variants], trace=True,
                         impulses=[(t, objects[k], vel) for t, k, vel in shared])
    assert all(entry[f].tobytes() == ps.state(objects)[f].tobytes() for f in entry)          # the caller's objects are untouched
    finals = []
    for k, change in enumerate(variants):
        twin, impulses = iu.variant_twin(objects, change, shared)
        counters, states = world.run(twin, cam, st, ticks, trace=True, impulses=impulses)
        assert len(out[k]) == 3 and iu.same_records(out[k][2], states) and iu.same_records(out[k][1], counters), k
        assert iu.same_state(out[k][0], twin), k
        finals.append(states[-1].tobytes())
    assert len(set(finals)) == 8                                                              # eight different futures
    # without the key and without impulses=: as ever
    plain = world.run_many(objects, cam, st, ticks, [{}], trace=True)
    assert iu.same_records(plain[0][2], world.run(iu.bu.twins(objects), cam, st, ticks, trace=True)[1])


def test_run_many_applies_shared_impulses_before_a_variants_own():
    spec, objects, st, _, _ = iu.fresh("order")
    cam, ticks, p = vec3(*spec["cam"]), spec["ticks"], sc.P53
    own_small = {objects[0]: dict(impulses=[(2, (p, 0, 0)), (2, vec3(p, 0, 0))])}
    own_big = {objects[0]: dict(impulses=[(2, (1.0, 0, 0))])}
    a = world.run_many(objects, cam, st, ticks, [own_small], trace=True, impulses=[(2, objects[0], (1.0, 0, 0))])[0]
    b = world.run_many(objects, cam, st, ticks, [own_big], trace=True, impulses=[(2, objects[0], (p, 0, 0)), (2, objects[0], (p, 0, 0))])[0]
    assert a[2]["vel"][-1, 0, 0] == 1.0 and b[2]["vel"][-1, 0, 0] == 1.0 + 2.0 ** -52          # 1 + p + p, and p + p + 1
    z = iu.fixture()
    assert np.array_equal(a[2]["vel"][:, 0].view(np.uint64), z["order"]["vel"][:, 0].view(np.uint64))
    assert np.array_equal(b[2]["vel"][:, 0].view(np.uint64), z["order@reversed"]["vel"][:, 0].view(np.uint64))


def test_run_many_with_draws_makes_the_references_draws_per_tick():
    spec, objects, st, _, gen = iu.fresh("wade_thrust")
    shared = sc.impulses_of(spec, objects)
    before = gen.getstate()
    twins, counters, states, draws, state = world.run_many(objects, vec3(*spec["cam"]), st, spec["ticks"], [{}], trace=True, rng=gen,
                                                           impulses=shared)[0]
    iu.assert_is_fixture("wade_thrust", states, draws)
    assert gen.getstate() == before
    fluid = np.load(ps.fixture_path("fluid"))["draws"]
    first = sc.THRUST_TICKS[0]
    assert np.array_equal(draws[:first], fluid[:first]) and draws[first] != fluid[first]


# ---- 3. what is refused ----------------------------------------------------------------------------------------------------
def test_value_errors():
    spec, objects, st, _, _ = iu.fresh("jump")
    cam, cube = vec3(*spec["cam"]), objects[1]
    for bad in ([(0, world.Object(), (0, 1, 0))], [(-1, cube, (0, 1, 0))], [(4, cube, (0, 1, 0))], [(1.0, cube, (0, 1, 0))],
                [(1, cube, (0, float("nan"), 0))], [(1, cube, (0, float("inf"), 0))], [(1, cube, (0, 1))], [(1, cube, "abc")],
                [(1, cube)]):
        with pytest.raises(ValueError):
            world.run(objects, cam, st, 4, impulses=bad)
        with pytest.raises(ValueError):
            world.run_many(objects, cam, st, 4, [{}], impulses=bad)
    for own in ([(4, (0, 1, 0))], [(0, (0, float("nan"), 0))], [(0, cube, (0, 1, 0))]):
        with pytest.raises(ValueError):
            world.run_many(objects, cam, st, 4, [{cube: dict(impulses=own)}])
    with pytest.raises(ValueError, match="not one of"):
        world.run_many(objects, cam, st, 4, [{world.Object(): dict(impulses=[(0, (0, 1, 0))])}])
    with pytest.raises(ValueError, match="clock"):
        world.run(objects, cam, st, 4, clock=(0, 10), impulses=[])
    assert ps.state(objects)["vel"].tolist() == [[0.0] * 3] * 2                               # a refused call has accelerated nothing
    # an empty list is a run without
    a, b = iu.bu.twins(objects), iu.bu.twins(objects)
    assert iu.same_records(world.run(a, cam, st, 4, trace=True, impulses=[])[1], world.run(b, cam, st, 4, trace=True)[1])
    # numpy numbers and vec3 are numbers
    c = iu.bu.twins(objects)
    world.run(c, cam, st, 4, impulses=[(np.int64(3), c[1], vec3(0, 1, 0)), (0, c[1], np.array([0.5, 0, 0]))])


def test_impulse_rows_are_sorted_stably_by_tick_and_body():
    lists = [[(2, 1, (1.0, 0, 0)), (0, 1, (2.0, 0, 0)), (2, 0, (3.0, 0, 0)), (2, 1, (4.0, 0, 0)), (0, 1, (5.0, 0, 0))], [], [(1, 0, (6.0, 0, 0))]]
    rows, first = world.impulse_rows(lists)
    assert rows.dtype == np.dtype(nat.IMPULSE_FIELDS) and rows.dtype.itemsize == 32 and first.dtype == np.int32
    assert first.tolist() == [0, 5, 5, 6]
    assert list(zip(rows["tick"].tolist(), rows["body"].tolist(), rows["vel"][:, 0].tolist())) == [
        (0, 1, 2.0), (0, 1, 5.0), (2, 0, 3.0), (2, 1, 1.0), (2, 1, 4.0), (1, 0, 6.0)]


# ---- 4. the header, the constants and the build --------------------------------------------------------------------------------
def test_header_and_native_constants_agree():
    text = open(os.path.join(ROOT, "include", "vrt.h")).read()
    L = nat.lib()
    assert L.vrt_abi_version() == 9 and nat.ABI_VERSION == 9 and re.search(r"#define VRT_ABI_VERSION 9\b", text)   # the change only adds
    assert nat.IMPULSE_BYTES == 32 == np.dtype(nat.IMPULSE_FIELDS).itemsize == C.sizeof(nat.VrtImpulse) and C.sizeof(nat.VrtImpulseList) == 24
    for (name, *_), (cname, _) in zip(nat.IMPULSE_FIELDS, nat.VrtImpulse._fields_):
        assert name == cname and np.dtype(nat.IMPULSE_FIELDS).fields[name][1] == getattr(nat.VrtImpulse, name).offset
    assert re.search(r"typedef struct vrt_impulse \{\s+/\* 32 bytes \*/", text)
    assert re.search(r"#define VRT_PHYSICS_MAX_IMPULSES \(1 << 20\)", text) and nat.PHYSICS_MAX_IMPULSES == 1 << 20
    assert re.search(r"VRT_S_PHYSICS_IMPULSES = 0,", text) and re.search(r"VRT_S_PHYSICS_IMPULSES_BAD = 1\b", text)
    assert (nat.S_PHYSICS_IMPULSES, nat.S_PHYSICS_IMPULSES_BAD) == (0, 1)
    # no physics kernel used these two words before: every other VRT_S_PHYSICS_* is word 4 or above
    others = [int(v) for n, v in re.findall(r"\b(VRT_S_PHYSICS_\w+) = (\d+)", text) if "IMPULSES" not in n]
    assert len(others) >= 12 and min(others) >= 4
    assert re.search(r"int vrt_physics_run_batch_impulses\(vrt_body\* d_bodies, int32_t n_runs, int32_t n_bodies, const uint8_t\* d_models, int64_t models_bytes,\s+"
                     r"const uint8_t\* d_remap, int32_t remap_bytes, const double\* d_matphys, int32_t n_materials,\s+"
                     r"const vrt_physics_params\* params, const vrt_physics_run_params\* run, int32_t\* d_ticks_done,\s+"
                     r"vrt_body_sample\* d_trace, uint64_t\* d_stats, void\* stream, uint32_t\* d_rng, uint64_t\* d_tick_draws,\s+"
                     r"const vrt_contact_log\* log, const vrt_impulse_list\* impulses\);", text)
    assert nat.EXPORTS.count("vrt_physics_run_batch_impulses") == 1 and L.vrt_physics_run_batch_impulses is not None
    assert list(L.vrt_physics_run_batch_impulses.argtypes)[:-1] == list(L.vrt_physics_run_batch_contacts.argtypes)
    assert [os.path.basename(u) for u in nat.PHYSICS_IMPULSES_UNITS] == ["vrt_physics_impulses.hip"]
    assert set(nat.PHYSICS_IMPULSES_UNITS) <= set(nat.SOURCES) and all(os.path.exists(s) for s in nat.SOURCES)
    assert "csrc/vrt_physics_impulses.hip" in open(os.path.join(ROOT, "tools", "build_variant.sh")).read()


def test_entry_point_rejects_bad_arguments_without_a_device():
    """Everything the entry point can refuse is refused before its first HIP call: these calls carry made-up device pointers,
    which nothing reads."""
    iu.assert_refusals(nat.lib())


def test_result_fields_are_none_without_impulses():
    from python_raytracer_amd.results import BatchRunResult, RunResult
    assert isinstance(RunResult.impulses_applied, property) and isinstance(RunResult.impulses_skipped, property)
    assert isinstance(BatchRunResult.impulses_applied, property) and isinstance(BatchRunResult.impulses_skipped, property)


# ---- 5. the compiler's report of the new translation unit ----------------------------------------------------------------------
def test_physics_impulses_report_is_the_saved_one():
    if not os.path.exists(kernel_report.HIPCC):
        pytest.skip("no hipcc")
    fresh = kernel_report.parse(physics_impulses_report.compile_report())
    saved = physics_impulses_report.saved()
    assert list(fresh) == list(saved) and fresh == saved
    # two kernels, each with the log and without: four instances, each held on its own
    assert len(fresh) == 4
    assert sum("physics_impulses_kernelILb" in n for n in fresh) == 2 and sum("physics_impulses_draws_kernelILb" in n for n in fresh) == 2
    for name, fig in fresh.items():
        # a workgroup of 16 waves launches without scratch and without a vector register spilled
        assert fig["VGPRs"] <= 128 and fig["VGPRs Spill"] == 0 and fig["ScratchSize [bytes/lane]"] == 0, (name, fig)
        assert fig["Occupancy [waves/SIMD]"] >= 4 and 0 < fig["LDS Size [bytes/block]"] <= 65536, (name, fig)
    # the list's state is a few LDS words on top of the kernels restated, not an array
    import physics_contacts_report
    restated = physics_contacts_report.saved()
    for kind in ("draws_kernel", "contacts_kernel"):
        old = [v for n, v in restated.items() if ("draws" in n) == ("draws" in kind)][0]
        new = [v for n, v in fresh.items() if ("draws" in n) == ("draws" in kind) and "ILb1E" in n][0]
        assert old["LDS Size [bytes/block]"] <= new["LDS Size [bytes/block]"] <= old["LDS Size [bytes/block]"] + 128, (kind, old, new)
