"""What the tests of the contact log share (tests/test_physics_contacts_host.py, tests/test_gpu_physics_contacts.py): the fixture
recorded from the real reference (tests/golden/physics_contacts.npz, made by tests/golden/make_physics_contacts.py), each of its
scenes run once through the host path, the host's filters written out by hand, and the calls of vrt_physics_run_batch_contacts
that it refuses before any HIP call.  Nothing of the GPU is imported."""
import ctypes as C
import functools
import os
import random

import numpy as np

import physics_batch_util as bu
import physics_scenes as ps
from python_raytracer_amd import _native as nat
from python_raytracer_amd import world
from python_raytracer_amd.lib import vec3

PATH = os.path.join(ps.GOLDEN, "physics_contacts.npz")
SCENES = ("edges_tiny", "edges_rot", "edges_chain", "pile", "default", "fluid")
ALL = 1 << 20     # a capacity no scene of the fixture reaches


def fresh(name):
    """(spec, objects, materials, settings, camera, a seeded generator or None) of a fixture scene, built anew."""
    _, spec = ps.load_fixture(name)
    objects, _, mats, st = ps.project_scene(spec)
    ps.clear_redraw(objects)
    gen = random.Random(spec["seed"]) if spec["seed"] is not None else None
    return spec, objects, mats, st, vec3(*spec["cam"]), gen


@functools.lru_cache(maxsize=None)
def fixture():
    z = np.load(PATH)
    return {name: (z[name], int(z[name + "_ticks"])) for name in SCENES}


@functools.lru_cache(maxsize=None)
def host(name, mode="voxels", ticks=None):
    """world.run(contacts=Contacts(ALL, mode)) on the scene, computed once and shared: (spec, objects after the run, materials of
    the scene, settings, counters, states, the ContactRecords).  Nobody changes what it returns."""
    spec, objects, mats, st, cam, gen = fresh(name)
    counters, states, log = world.run(objects, cam, st, ticks or spec["ticks"], trace=True, rng=gen.random if gen else None,
                                      contacts=world.Contacts(ALL, mode))
    return spec, objects, mats, st, counters, states, log


def in_scene_materials(log, mats):
    """The records of a log with mat_other and mat_mover as indices into the scene's material list, as the fixture has them."""
    index = {id(m): i for i, m in enumerate(mats)}
    out = log.records.copy()
    for f in ("mat_other", "mat_mover"):
        out[f] = [index[id(log.materials[g])] for g in log.records[f]]
    return out


def first_of_each_pair(records):
    """The host filter of PAIRS mode, written out: the first record of each (tick, mover, step, other)."""
    keep, seen = [], set()
    for i, r in enumerate(records):
        key = (int(r["tick"]), int(r["mover"]), int(r["step"]), int(r["other"]))
        if key not in seen:
            seen.add(key)
            keep.append(i)
    return records[keep]


def same_log(a, b):
    """Two ContactRecords agree: every byte of the stored rows, the totals, and the Materials the ids stand for (the same
    objects, or -- two builds of one scene -- materials of the same physical properties)."""
    if a.total != b.total or a.lost != b.lost or a.records.dtype != b.records.dtype or a.records.tobytes() != b.records.tobytes():
        return False
    used = set(a.records["mat_other"].tolist()) | set(a.records["mat_mover"].tolist())
    what = lambda m: (m.solidity, m.weight, m.friction, m.elasticity)  # noqa: E731
    return all(a.materials[g] is b.materials[g] or what(a.materials[g]) == what(b.materials[g]) for g in used)


def contacts_call(L, draws=False):
    """vrt_physics_run_batch_contacts with made-up device pointers, which nothing reads before the checks are through:
    call(**batch arguments, rng, tick_draws, log) and a maker of logs."""
    fake = 0x1000

    def make_log(records=fake, counts=fake, mask=None, capacity=16, mode=nat.CONTACTS_PAIRS):
        return nat.VrtContactLog(records, counts, mask, capacity, mode)

    def call(rng=fake if draws else None, tick_draws=fake if draws else None, log=make_log(), **batch):
        class Entry:
            @staticmethod
            def vrt_physics_run_batch(*args):
                return L.vrt_physics_run_batch_contacts(*args, rng, tick_draws, C.byref(log) if log is not None else None)
        return bu.batch_call(Entry)[0](**batch)
    return call, make_log, fake


def assert_refusals(L):
    """Every VRT_ERR_ARG of the entry point, before any HIP call: the restated entries' and the log's own."""
    fake = 0x1000
    for draws in (False, True):
        class Restated:
            """vrt_physics_run_batch_contacts under the batch's name, with a good log (and good generators)"""
            @staticmethod
            def vrt_physics_run_batch(*args):
                log = nat.VrtContactLog(fake, fake, None, 16, nat.CONTACTS_VOXELS)
                return L.vrt_physics_run_batch_contacts(*args, fake if draws else None, fake if draws else None, C.byref(log))
        bu.assert_refusals(Restated)
        call, make_log, _ = contacts_call(L, draws)
        assert call(log=None) == -1                                                                 # a NULL log
        assert call(log=make_log(capacity=-1)) == -1                                                # capacity < 0
        assert call(log=make_log(mode=2)) == -1 and call(log=make_log(mode=-1)) == -1               # a mode other than the two
        assert call(log=make_log(counts=None)) == -1 and call(log=make_log(counts=fake + 4)) == -1  # NULL or misaligned d_counts
        assert call(log=make_log(records=None)) == -1                                               # d_records NULL with capacity > 0
        assert call(log=make_log(records=fake + 4)) == -1 and call(log=make_log(records=fake + 4, capacity=0)) == -1   # misaligned
        assert call(runs=3, log=make_log(capacity=(1 << 31) // 3 + 1)) == -1                        # n_runs * capacity > 2^31 - 1
        assert call(runs=2, log=make_log(capacity=1 << 30)) == -1
    # ... and with generators what vrt_physics_run_batch_draws refuses of them
    call, make_log, _ = contacts_call(L, True)
    assert call(rng=fake + 2) == -1 and call(rng=fake + 1) == -1 and call(tick_draws=fake + 4) == -1
