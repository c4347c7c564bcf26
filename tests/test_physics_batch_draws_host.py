"""What-if runs with the reference's random draws (run_many(rng=), vrt_physics_run_batch_draws), without a GPU: the host form
(world.run_many(rng=)) against world.run(rng=) on hand-made twins, bit for bit, with the caller's objects and generators left alone;
the condition that makes K seeds of one variant worth running (they end in different places); what `rng` refuses; BatchRunResult's
new fields; the C ABI's new symbol, what it refuses before any HIP call, its place in the build; and the compiler's resource report
of python_raytracer_amd/csrc/vrt_physics_batch_draws.hip against the saved one."""
import inspect
import os
import random
import re

import numpy as np
import pytest

import kernel_report
import physics_batch_draws_report
import physics_batch_util as bu
import physics_run_draw_scenes as rd
import physics_run_util as ru
import physics_scenes as ps
from python_raytracer_amd import _native as nat
from python_raytracer_amd import world
from python_raytracer_amd.lib import vec3

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vrt.h")
# the Monte-Carlo scene of tests/test_gpu_physics_batch_draws.py: `wade` as recorded, without its clock, for its 20 ticks
MONTE_CARLO_SEEDS = 16


def scene(name):
    """(objects, settings, camera, followed object or None, ticks): `wade` without its clock and with follow, or `fluid` for 8 of
    its 24 ticks (a tick of `fluid` makes about 1500 draws: eight of them regenerate the generator's state some twenty times)."""
    if name == "wade":
        _, spec, objects, _, st, who = rd.fresh("wade")
        return objects, st, vec3(*spec["cam"]), who, spec["ticks"]
    _, spec = ps.load_fixture(name)
    objects, _, _, st = ps.project_scene(spec)
    ps.clear_redraw(objects)
    return objects, st, vec3(*spec["cam"]), None, 8


def six_generators(seed):
    """Six generators in different states: three fresh seeds, one part-way through its first state, two far along."""
    gens = [random.Random(seed + i) for i in range(6)]
    for g, n in zip(gens[3:], (100, 5000, 70001)):
        for _ in range(n):
            g.getrandbits(32)
    assert len({g.getstate() for g in gens}) == 6
    return gens


def copy_of(g):
    c = random.Random()
    c.setstate(g.getstate())
    return c


def same_state(a, b):
    sa, sb = ps.state(a), ps.state(b)
    return all(sa[f].tobytes() == sb[f].tobytes() for f in sa)


def twin_run(objects, change, cam, st, ticks, who, gen):
    """world.run(rng=) on a hand-made twin with `change` applied and a copy of `gen`: (twin, counters, states, draws per tick, the
    copy after the run).  The draws of each tick come from a second twin stepped tick by tick with a counting callable."""
    twin, g = bu.altered(objects, change), copy_of(gen)
    follow = twin[objects.index(who)] if who is not None else None
    counters, states = world.run(twin, cam, st, ticks, follow=follow, trace=True, rng=g.random)
    again, g2, made = bu.altered(objects, change), copy_of(gen), []

    def draw():
        made[-1] += 1
        return g2.random()
    follow = again[objects.index(who)] if who is not None else None
    for _ in range(ticks):
        made.append(0)
        world.run(again, follow.cam_pos if follow is not None else cam, st, 1, rng=draw)
    assert same_state(twin, again) and g.getstate() == g2.getstate()
    return twin, counters, states, made, g


# ---- 1. the host form is the loop of run(rng=) on twins ----------------------------------------------------------------------
@pytest.mark.parametrize("name", ["wade", "fluid"])
def test_host_run_many_with_rng_is_run_with_rng_on_twins(name):
    objects, st, cam, who, ticks = scene(name)
    entry = ps.state(objects)
    changes = bu.changes(objects, cam.tuple())
    assert len(changes) == 6 and changes[0] == {}
    gens = six_generators(411)
    before = [g.getstate() for g in gens]
    variants = [bu.mapping(objects, c) for c in changes]
    got = world.run_many(objects, cam, st, ticks, variants, follow=who, trace=True, rng=gens)
    assert len(got) == 6 and all(len(item) == 5 for item in got)
    after = ps.state(objects)
    assert all(entry[f].tobytes() == after[f].tobytes() for f in entry)      # the caller's objects: untouched
    assert [g.getstate() for g in gens] == before                             # ... and all six generators
    total = 0
    for k, (change, (copies, counters, states, draws, state)) in enumerate(zip(changes, got)):
        twin, want_counters, want_states, want_draws, g = twin_run(objects, change, cam, st, ticks, who, gens[k])
        assert ru.same_records(counters, want_counters) and ru.same_records(states, want_states), (name, k)
        assert same_state(copies, twin), (name, k)
        assert draws.dtype == np.uint64 and draws.tolist() == want_draws, (name, k)
        assert state == g.getstate() and np.array_equal(np.array(state[1], np.uint32), rd.state_words(g)), (name, k)
        total += sum(want_draws)
    assert total > 0
    # one generator for all: six copies of it
    one = world.run_many(objects, cam, st, ticks, variants, follow=who, trace=True, rng=gens[4])
    six = world.run_many(objects, cam, st, ticks, variants, follow=who, trace=True, rng=[copy_of(gens[4]) for _ in range(6)])
    same = world.run_many(objects, cam, st, ticks, variants, follow=who, trace=True, rng=[gens[4]] * 6)    # the same object six times
    for a, b, c in zip(one, six, same):
        assert ru.same_records(a[1], b[1]) and ru.same_records(a[2], b[2]) and a[3].tolist() == b[3].tolist() and a[4] == b[4]
        assert ru.same_records(a[2], c[2]) and a[3].tolist() == c[3].tolist() and a[4] == c[4]
    assert gens[4].getstate() == before[4]
    # without rng the tuples are as they were
    plain = world.run_many(objects, cam, st, 1, variants[:1], follow=who)
    assert len(plain[0]) == 3


# ---- 2. K seeds of one variant are K futures ---------------------------------------------------------------------------------
def test_sixteen_seeds_of_wade_end_in_different_places():
    """The condition of the Monte-Carlo test on the device, shown from world.run alone: `wade` as it stands ({}), without its clock,
    for its 20 recorded ticks, under 16 seeds."""
    finals, draws = set(), set()
    for seed in range(MONTE_CARLO_SEEDS):
        objects, st, cam, who, ticks = scene("wade")
        assert ticks == 20
        g = random.Random(seed)
        _, states = world.run(objects, cam, st, ticks, follow=who, trace=True, rng=g.random)
        finals.add(states[-1].tobytes())
        draws.add(g.getstate())
    assert len(finals) >= 2 and len(draws) == MONTE_CARLO_SEEDS, len(finals)


# ---- 3. what rng refuses -----------------------------------------------------------------------------------------------------
def test_rng_argument_errors():
    objects, st, cam, who, _ = scene("wade")
    before = ps.state(objects)
    g = random.Random(1)
    state = g.getstate()
    for bad in (5, "random", object(), g.random, [g, 5], [g, g.random], (g, None)):
        with pytest.raises(TypeError, match="rng"):
            world.run_many(objects, cam, st, 1, [{}, {}], follow=who, rng=bad)
        with pytest.raises(TypeError, match="rng"):
            world._generators(bad, 2, "DeviceWorld.run_many()")              # the one check both forms make
    for bad in ([], [g], [g, g, g]):
        with pytest.raises(ValueError, match="generators"):
            world.run_many(objects, cam, st, 1, [{}, {}], follow=who, rng=bad)
        with pytest.raises(ValueError, match="generators"):
            world._generators(bad, 2, "DeviceWorld.run_many()")
    assert world._generators(g, 3, "x") == [g, g, g] and world._generators((g, g), 2, "x") == [g, g]
    # animation inside a batch stays out: neither form takes a clock
    with pytest.raises(TypeError):
        world.run_many(objects, cam, st, 1, [{}], follow=who, rng=g, clock=(0, 50))
    for f in (world.run_many, world.DeviceWorld.run_many):
        names = list(inspect.signature(f).parameters)
        assert "clock" not in names and names[-1] == "rng" and inspect.signature(f).parameters["rng"].default is None
    assert list(inspect.signature(world.DeviceWorld.run_many).parameters)[:10] == [
        "self", "objects", "pos_cam", "settings", "ticks", "variants", "follow", "trace", "budget", "time_kernel"]
    after = ps.state(objects)
    assert all(before[f].tobytes() == after[f].tobytes() for f in before) and g.getstate() == state
    assert "vrt_physics_run_batch_draws" in world.DeviceWorld.run_many.__doc__


def test_batch_result_has_the_draws_and_the_generators():
    from python_raytracer_amd.results import BatchRunResult
    records = np.zeros((2, 3), np.dtype(nat.BODY_FIELDS))
    plain = BatchRunResult(records, records.copy(), [[], []], None, np.array([4, 4]), 1, None, (2, 4, 3))
    assert plain.draws is None and plain.draws_per_tick is None and plain.rng_state(0) is None
    handed = [random.Random(3), random.Random(4)]
    handed[1].gauss(0, 1)                                          # (leaves a gauss_next behind, which is carried through)
    starts = [g.getstate() for g in handed]
    assert starts[1][2] is not None
    ends = [random.Random(5), random.Random(6)]
    words = np.array([g.getstate()[1] for g in ends], np.uint32)
    per_tick = np.array([[5, 0, 7, 1], [0, 0, 2048, 9]], np.uint64)
    r = BatchRunResult(records, records.copy(), [[], []], None, np.array([4, 4]), 1, None, (2, 4, 3), None, per_tick, words, starts)
    assert r.draws.tolist() == [13, 2057] and r.draws.dtype == np.uint64 and r.draws_per_tick is per_tick
    assert r.rng_state(0) == ends[0].getstate() and r.rng_state(1) == (3, ends[1].getstate()[1], starts[1][2])
    objects, *_ = scene("wade")
    g = random.Random(9)
    r.apply(1, objects, rng=g)
    assert g.getstate() == r.rng_state(1) and [h.getstate() for h in handed] == starts
    with pytest.raises(TypeError, match="rng"):
        r.apply(0, objects, rng=g.random)
    # a batch that did not draw leaves the generator alone
    state = g.getstate()
    plain.apply(0, objects, rng=g)
    assert g.getstate() == state


# ---- 4. the C ABI ------------------------------------------------------------------------------------------------------------
def test_symbol_and_units():
    text = open(HEADER).read()
    assert "#define VRT_ABI_VERSION 9" in text
    L = nat.lib()
    assert L.vrt_abi_version() == 9 and nat.ABI_VERSION == 9      # the change only adds a symbol
    assert L.vrt_physics_run_batch_draws is not None and nat.EXPORTS.count("vrt_physics_run_batch_draws") == 1
    assert list(L.vrt_physics_run_batch_draws.argtypes) == list(L.vrt_physics_run_batch.argtypes) + [L.vrt_physics_run_batch.argtypes[0]] * 2
    assert re.search(r"int vrt_physics_run_batch_draws\(vrt_body\* d_bodies, int32_t n_runs, int32_t n_bodies, const uint8_t\* d_models, int64_t models_bytes,\s+"
                     r"const uint8_t\* d_remap, int32_t remap_bytes, const double\* d_matphys, int32_t n_materials,\s+"
                     r"const vrt_physics_params\* params, const vrt_physics_run_params\* run, int32_t\* d_ticks_done,\s+"
                     r"vrt_body_sample\* d_trace, uint64_t\* d_stats, void\* stream, uint32_t\* d_rng, uint64_t\* d_tick_draws\);", text)
    # the per-run rules are stated where the symbol is declared
    doc = text[text.index("/* vrt_physics_run_batch with the reference's random draws"):text.index("int vrt_physics_run_batch_draws(")]
    for phrase in ("a run that is done", "not its d_rng", "VRT_S_PHYSICS_BATCH_BADTICK", "before\n *     the generator is read",
                   "VRT_S_PHYSICS_RNG_INVALID", "n_bodies == 0", "a NULL d_rng", "[n_runs][625] uint32", "ABSOLUTE tick"):
        assert phrase in doc, phrase
    # the statistics words of a drawing run collide with neither flag
    words = {nat.S_PHYSICS_WORK, nat.S_PHYSICS_TICKS, nat.S_PHYSICS_DRAWS, nat.S_PHYSICS_BODIES, nat.S_PHYSICS_REFUSED, nat.S_PHYSICS_STEPS,
             nat.S_PHYSICS_BLOCKED, nat.S_PHYSICS_CONTACTS, nat.S_PHYSICS_TRANSFERS, nat.S_PHYSICS_CAPPED}
    assert len(words) == 10 and not words & {nat.S_PHYSICS_BATCH_BADTICK, nat.S_PHYSICS_RNG_INVALID}
    assert (nat.S_PHYSICS_BATCH_BADTICK, nat.S_PHYSICS_RNG_INVALID) == (4, 7)
    # the build: a unit of its own in the one library, counted by needs_build(), and in the variant build
    assert [os.path.basename(u) for u in nat.PHYSICS_BATCH_DRAWS_UNITS] == ["vrt_physics_batch_draws.hip"]
    assert set(nat.PHYSICS_BATCH_DRAWS_UNITS) <= set(nat.SOURCES) and all(os.path.exists(u) for u in nat.PHYSICS_BATCH_DRAWS_UNITS)
    others = nat.UNITS + nat.PHYSICS_UNITS + nat.PHYSICS_DRAWS_UNITS + nat.PHYSICS_RUN_UNITS + nat.PHYSICS_ANIM_UNITS + \
        nat.PHYSICS_RUN_DRAWS_UNITS + nat.CHUNK_LISTS_UNITS + nat.PHYSICS_BATCH_UNITS
    assert len(others) == 9 and not set(nat.PHYSICS_BATCH_DRAWS_UNITS) & set(others)
    assert "csrc/vrt_physics_batch_draws.hip" in open(os.path.join(ROOT, "tools", "build_variant.sh")).read()


def test_physics_run_batch_draws_rejects_bad_arguments_without_a_device():
    """Everything the entry point can refuse is refused before its first HIP call: these calls carry made-up device pointers,
    which nothing reads."""
    L = nat.lib()
    fake = 0x1000

    class WithGoodGenerators:
        """vrt_physics_run_batch_draws under the batch's name, with good d_rng and d_tick_draws: every refusal of the batch"""
        @staticmethod
        def vrt_physics_run_batch(*args):
            return L.vrt_physics_run_batch_draws(*args, fake, fake)
    bu.assert_refusals(WithGoodGenerators)
    # ... and its own: the generators' words and the per-tick counts
    call, run_params, _ = bu.batch_call(type("Own", (), {"vrt_physics_run_batch": staticmethod(lambda *a: a)}))
    args = call()

    def own(rng=fake, tick_draws=fake):
        return L.vrt_physics_run_batch_draws(*args, rng, tick_draws)
    assert own(rng=None) == -1 and own(rng=fake + 2) == -1 and own(rng=fake + 1) == -1 and own(rng=fake + 3) == -1
    assert own(tick_draws=fake + 4) == -1 and own(tick_draws=fake + 1) == -1
    assert own(rng=None, tick_draws=None) == -1 and own(rng=fake + 2, tick_draws=None) == -1


# ---- 5. the compiler's report of the new translation unit --------------------------------------------------------------------
def test_physics_batch_draws_report_is_the_saved_one():
    if not os.path.exists(kernel_report.HIPCC):
        pytest.skip("no hipcc")
    fresh = kernel_report.parse(physics_batch_draws_report.compile_report())
    saved = physics_batch_draws_report.saved()
    assert list(fresh) == list(saved) and fresh == saved
    names = [n for n in fresh if "physics_batch_draws_kernel" in n]
    assert len(names) == 1 and len(fresh) == 1               # one kernel: one launch for all runs, the statistics cleared inside it
    fig = fresh[names[0]]
    # the conditions: a workgroup of 16 waves launches without scratch and without a vector register spilled
    assert fig["ScratchSize [bytes/lane]"] == 0 and fig["VGPRs Spill"] == 0, fig
    assert fig["VGPRs"] <= 128 and fig["Occupancy [waves/SIMD]"] == 4, fig
    assert 0 < fig["LDS Size [bytes/block]"] <= 64 * 1024     # within what every launch may ask for without opting in
    # the LDS of the drawing run without sprite tables and the ticks done at entry: a batch adds a grid, not shared state
    import physics_run_draws_report
    run = [v for n, v in physics_run_draws_report.saved().items() if "ILb0E" in n]
    assert len(run) == 1 and run[0]["LDS Size [bytes/block]"] <= fig["LDS Size [bytes/block]"] <= run[0]["LDS Size [bytes/block]"] + 16
