"""The contact log on the host (world.Contacts, world.run(contacts=), world.run_many(contacts=), results.ContactRecords), held
record for record to the real reference through tests/golden/physics_contacts.npz; its counts against the `contacts` counters,
its material pairs against the friction terms of update_physics(trace=); the two filters and the capacity; the header, the
constants and the build; what the entry point refuses before any HIP call; and the compiler's report of the new translation unit
against the saved one.  No GPU."""
import os
import random
import re

import numpy as np
import pytest

import kernel_report
import physics_batch_util as bu
import physics_contacts_report
import physics_contacts_util as cu
import physics_scenes as ps
from python_raytracer_amd import _native as nat
from python_raytracer_amd import world
from python_raytracer_amd.lib import vec3
from python_raytracer_amd.results import ContactRecords

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. the host's log is the reference's ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cu.SCENES)
def test_host_log_is_the_references_record_for_record(name):
    want, ticks = cu.fixture()[name]
    spec, objects, mats, st, counters, states, log = cu.host(name)
    assert ticks == spec["ticks"] and len(want) > 0                    # the file holds every scene's whole run
    assert isinstance(log, ContactRecords) and log.records.dtype == np.dtype(nat.CONTACT_FIELDS) and log.records.dtype.itemsize == 40
    assert log.total == len(log.records) == len(want) and log.lost == 0 and log.materials[0] is None
    got = cu.in_scene_materials(log, mats)
    assert got.tobytes() == want.tobytes(), (name, np.nonzero(got != want)[0][:5])
    assert not log.records["reserved"].any()
    # the order is the reference's: ticks -> bodies -> steps -> met bodies (ascending within a step) -> x -> y -> z
    key = np.stack([log.records[f].astype(np.int64) for f in ("tick", "mover", "step", "other")] +
                   [log.records["voxel"][:, a].astype(np.int64) for a in range(3)], axis=1)
    assert all(tuple(a) < tuple(b) for a, b in zip(key[:-1], key[1:])), name


@pytest.mark.parametrize("name", cu.SCENES)
def test_every_tick_and_body_has_as_many_records_as_its_counter(name):
    spec, objects, mats, st, counters, states, log = cu.host(name)
    count = np.zeros(counters.shape, np.int64)
    np.add.at(count, (log.records["tick"], log.records["mover"]), 1)
    assert np.array_equal(count, counters["contacts"]) and count.sum() == log.total > 0


@pytest.mark.parametrize("name", cu.SCENES)
def test_logged_material_pairs_give_the_friction_terms_in_order(name):
    spec, objects, mats, st, cam, gen = cu.fresh(name)
    terms = []
    for t in range(spec["ticks"]):
        steps = []
        world.tick(objects, cam, st, rng=gen.random if gen else None, trace=steps)
        terms += [term for _, s in steps for term in s["terms"]]
    log = cu.host(name)[6]
    # (the host run's Materials are another build of the scene: the same list, index for index)
    from_log = [log.materials[r["mat_other"]].friction * log.materials[r["mat_mover"]].friction * st.friction for r in log.records]
    assert len(terms) == log.total and np.array_equal(np.array(from_log).view(np.uint64), np.array(terms, np.float64).view(np.uint64))


# ---- 2. the filters and the capacity -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["edges_chain", "pile", "fluid"])
def test_pairs_is_the_first_record_of_each_touch(name):
    voxels, pairs = cu.host(name)[6], cu.host(name, "pairs")[6]
    want = cu.first_of_each_pair(voxels.records)
    assert 0 < len(want) < voxels.total and pairs.total == len(want) and pairs.records.tobytes() == want.tobytes()
    grouped = voxels.pairs()
    assert grouped.dtype.names == tuple(f[0] for f in nat.CONTACT_FIELDS) + ("count",)
    assert int(grouped["count"].sum()) == voxels.total and len(grouped) == len(want)
    assert all(np.array_equal(grouped[f[0]], want[f[0]]) for f in nat.CONTACT_FIELDS)
    assert (grouped["count"] >= 1).all() and grouped["count"].max() > 1


def test_of_keeps_the_records_of_the_listed_objects():
    spec, objects, mats, st, counters, states, full = cu.host("pile")
    _, mine, _, _, cam, _ = cu.fresh("pile")
    who = [mine[3], mine[17]]
    *_, log = world.run(mine, cam, st, spec["ticks"], contacts=world.Contacts(cu.ALL, "voxels", of=who))
    r = full.records
    want = r[np.isin(r["mover"], [3, 17]) | np.isin(r["other"], [3, 17])]
    assert 0 < len(want) < len(r) and log.total == len(want) and log.records.tobytes() == want.tobytes()
    assert (want["other"] == 3).any() or (want["other"] == 17).any()                # ... as the other as well as the mover
    # ContactRecords.of and .first: by Object and by index
    assert log.of(mover=mine[3]).tobytes() == want[want["mover"] == 3].tobytes() == log.of(mover=3).tobytes()
    assert log.of(other=mine[0]).tobytes() == want[want["other"] == 0].tobytes()
    assert log.first(mine[3]).tobytes() == want[want["mover"] == 3][0].tobytes() and log.first(mine[3], other=mine[3]) is None
    with pytest.raises(ValueError):
        log.of(mover=world.Object())
    # nobody listed: nothing logged, everything else as ever
    counters2, _, none = world.run(cu.fresh("pile")[1], cam, st, spec["ticks"], trace=True, contacts=world.Contacts(cu.ALL, "voxels", of=[]))
    assert none.total == 0 and len(none.records) == 0 and np.array_equal(counters2, counters)


@pytest.mark.parametrize("capacity", [0, 1, 1701, 3402, 5000])
def test_capacity_keeps_the_prefix_and_counts_the_rest(capacity):
    spec, objects, mats, st, counters, states, full = cu.host("pile")
    assert full.total == 3402
    *_, log = world.run(cu.fresh("pile")[1], vec3(*spec["cam"]), st, spec["ticks"], contacts=world.Contacts(capacity, "voxels"))
    assert log.total == full.total and log.lost == max(0, full.total - capacity) and log.capacity == capacity
    assert len(log.records) == min(capacity, full.total) and log.records.tobytes() == full.records[:capacity].tobytes()


def test_a_run_with_a_log_is_the_run_without_one():
    for name in ("edges_chain", "fluid"):
        spec, objects, mats, st, counters, states, log = cu.host(name)
        _, plain, _, _, cam, gen = cu.fresh(name)
        counters2, states2 = world.run(plain, cam, st, spec["ticks"], trace=True, rng=gen.random if gen else None)
        assert counters.tobytes() == counters2.tobytes() and states.tobytes() == states2.tobytes()


def test_run_many_appends_every_variants_log():
    spec, objects, mats, st, cam, _ = cu.fresh("edges_tiny")
    variants = [{}, {objects[1]: dict(vel=vec3(0.5, 0, 0))}, {objects[1]: dict(pos=vec3(40, 5, 0))}]
    request = world.Contacts(cu.ALL, "voxels", of=[objects[1]])
    out = world.run_many(objects, cam, st, spec["ticks"], variants, contacts=request)
    assert [len(o) for o in out] == [4, 4, 4]
    assert cu.same_log(out[0][3], cu.host("edges_tiny")[6]) and out[2][3].total == 0 and out[1][3].total > 0
    drew = world.run_many(objects, cam, st, spec["ticks"], variants, rng=random.Random(5), contacts=request)
    assert [len(o) for o in drew] == [6, 6, 6] and all(cu.same_log(a[3], b[5]) for a, b in zip(out, drew))
    assert len(world.run_many(objects, cam, st, 2, variants)[0]) == 3                # without contacts=: as ever
    with pytest.raises(ValueError, match="not one of"):
        world.run_many(objects, cam, st, 2, variants, contacts=world.Contacts(of=[world.Object()]))


def test_value_errors():
    with pytest.raises(ValueError, match="capacity"):
        world.Contacts(capacity=-1)
    with pytest.raises(ValueError, match="mode"):
        world.Contacts(mode="faces")
    with pytest.raises(ValueError, match="mode"):
        world.Contacts(mode=1)
    spec, objects, mats, st, cam, _ = cu.fresh("edges_tiny")
    with pytest.raises(ValueError, match="not one of"):
        world.run(objects, cam, st, 2, contacts=world.Contacts(of=[objects[1], world.Object()]))
    with pytest.raises(TypeError):
        world.run(objects, cam, st, 2, contacts="pairs")
    c = world.Contacts()
    assert (c.capacity, c.mode, c.of) == (4096, "pairs", None) and c.mask(objects, "x") is None
    assert world.Contacts(of=[objects[1]]).mask(objects, "x").tolist() == [0, 3]


# ---- 3. the header, the constants and the build ------------------------------------------------------------------------------
def test_header_and_native_constants_agree():
    text = open(os.path.join(ROOT, "include", "vrt.h")).read()
    L = nat.lib()
    assert L.vrt_abi_version() == 9 and nat.ABI_VERSION == 9 and re.search(r"#define VRT_ABI_VERSION 9\b", text)   # the change only adds
    assert nat.CONTACT_BYTES == 40 == np.dtype(nat.CONTACT_FIELDS).itemsize == __import__("ctypes").sizeof(nat.VrtContact)
    assert __import__("ctypes").sizeof(nat.VrtContactLog) == 32
    for (name, *_), (cname, _) in zip(nat.CONTACT_FIELDS, nat.VrtContact._fields_):
        assert name == cname and np.dtype(nat.CONTACT_FIELDS).fields[name][1] == getattr(nat.VrtContact, name).offset
    assert re.search(r"typedef struct vrt_contact \{\s+/\* 40 bytes \*/", text)
    body = text[text.index("typedef struct vrt_contact {"):text.index("} vrt_contact;")]
    assert re.findall(r"\b(\w+)(?:\[\d\])?;", re.sub(r"/\*.*?\*/", "", body, flags=re.S)) ==[f[0] for f in nat.CONTACT_FIELDS]
    assert re.search(r"VRT_CONTACTS_VOXELS = 0,", text) and re.search(r"VRT_CONTACTS_PAIRS = 1\b", text)
    assert (nat.CONTACTS_VOXELS, nat.CONTACTS_PAIRS) == (0, 1) and world.Contacts.MODES == {"voxels": 0, "pairs": 1}
    assert re.search(r"int vrt_physics_run_batch_contacts\(vrt_body\* d_bodies, int32_t n_runs, int32_t n_bodies, const uint8_t\* d_models, int64_t models_bytes,\s+"
                     r"const uint8_t\* d_remap, int32_t remap_bytes, const double\* d_matphys, int32_t n_materials,\s+"
                     r"const vrt_physics_params\* params, const vrt_physics_run_params\* run, int32_t\* d_ticks_done,\s+"
                     r"vrt_body_sample\* d_trace, uint64_t\* d_stats, void\* stream, uint32_t\* d_rng, uint64_t\* d_tick_draws,\s+"
                     r"const vrt_contact_log\* log\);", text)
    assert nat.EXPORTS.count("vrt_physics_run_batch_contacts") == 1 and L.vrt_physics_run_batch_contacts is not None
    assert list(L.vrt_physics_run_batch_contacts.argtypes)[:-1] == list(L.vrt_physics_run_batch_draws.argtypes)
    # the build: a unit of its own in the one library, counted by needs_build() with its header, and in the variant build
    assert [os.path.basename(u) for u in nat.PHYSICS_CONTACTS_UNITS] == ["vrt_physics_contacts.hip"]
    assert set(nat.PHYSICS_CONTACTS_UNITS) <= set(nat.SOURCES) and os.path.join(nat.HERE, "csrc", "vrt_physics_contacts.h") in nat.SOURCES
    assert all(os.path.exists(s) for s in nat.SOURCES)
    assert "csrc/vrt_physics_contacts.hip" in open(os.path.join(ROOT, "tools", "build_variant.sh")).read()


def test_entry_point_rejects_bad_arguments_without_a_device():
    """Everything the entry point can refuse is refused before its first HIP call: these calls carry made-up device pointers,
    which nothing reads."""
    cu.assert_refusals(nat.lib())


# ---- 4. the compiler's report of the new translation unit --------------------------------------------------------------------
def test_physics_contacts_report_is_the_saved_one():
    if not os.path.exists(kernel_report.HIPCC):
        pytest.skip("no hipcc")
    fresh = kernel_report.parse(physics_contacts_report.compile_report())
    saved = physics_contacts_report.saved()
    assert list(fresh) == list(saved) and fresh == saved
    assert len(fresh) == 2 and sum("physics_contacts_kernel" in n for n in fresh) == 1 and sum("physics_contacts_draws_kernel" in n for n in fresh) == 1
    for name, fig in fresh.items():
        # a workgroup of 16 waves launches without scratch and without a vector register spilled
        assert fig["VGPRs"] <= 128 and fig["VGPRs Spill"] == 0 and fig["ScratchSize [bytes/lane]"] == 0, (name, fig)
        assert fig["Occupancy [waves/SIMD]"] >= 4 and 0 < fig["LDS Size [bytes/block]"] <= 65536, (name, fig)
    # the drawing instance adds two words of LDS to the kernel it restates, not an array
    import physics_batch_draws_report
    draws = [v for n, v in fresh.items() if "draws" in n][0]
    restated = list(physics_batch_draws_report.saved().values())[0]
    assert restated["LDS Size [bytes/block]"] <= draws["LDS Size [bytes/block]"] <= restated["LDS Size [bytes/block]"] + 16
