"""The drawing physics tick at its limits, without a GPU: the three runs recorded from the real reference for the sizes
vrt_physics_draws.hip dimensions itself for (tests/physics_draw_scenes.py, tests/golden/make_physics_draws.py) -- `brim`: passes
of 1024 tests that all draw twice, that are all undecided, that are all contacts; `classes`: the solidities at which the number of
draws changes; `crowd_fluid`: undecided tests in candidates on both sides of body 1024 -- against the host path (world.tick with a
seeded generator), what the files say the runs reached, and, from the recorded classes, which pass of `brim` first needs the
eighth state of the generator's row from which start index (tests/test_gpu_physics_draws_edges.py starts there)."""
import json
import math
import os
import random
import re

import numpy as np
import pytest

import physics_draw_scenes as pds
import physics_scenes as ps
from python_raytracer_amd import _native as nat
from python_raytracer_amd import world
from python_raytracer_amd.lib import vec3

NAMES = ("brim", "classes", "crowd_fluid")
STATE, PASS, ROW = 624, 1024, 8          # VRT_MT_N, VRT_PHYS_BLOCK, VRT_MT_BLOCKS of vrt_physics_draws.hip
START_INDICES = (0, 1, 272, 273, 274, 623, 624)


def reached(z):
    return json.loads(bytes(z["reached"]).decode())


@pytest.mark.parametrize("name", NAMES)
def test_host_tick_with_the_seeded_generator_is_the_references(name):
    z, spec = ps.load_fixture(name)
    assert json.dumps(pds.SCENES[name]) == json.dumps(spec)            # made from the scene as it is described now (NaN != NaN: as text)
    objects, _, _, st = ps.project_scene(spec)
    gen = random.Random(spec["seed"])
    made = [0]

    def draw():
        made[0] += 1
        return gen.random()

    assert z["draws"].dtype == np.int64 and len(z["draws"]) == spec["ticks"] == len(z["pos"])
    cam = spec["cam"]
    for k in range(spec["ticks"]):
        ps.clear_redraw(objects)
        cam = ps.apply_script(spec, k, objects, vec3, cam)
        before = made[0]
        world.tick(objects, vec3(*cam), st, rng=draw)
        ps.assert_tick(z, k, objects, name)
        assert made[0] - before == z["draws"][k], k
    twin = random.Random(spec["seed"])
    for _ in range(int(z["draws"].sum())):
        twin.random()
    assert gen.getstate() == twin.getstate()
    # another seed, another run
    objects, _, _, _ = ps.project_scene(spec)
    other = random.Random(spec["seed"] + 1).random
    path, cam = [], spec["cam"]
    for k in range(spec["ticks"]):
        cam = ps.apply_script(spec, k, objects, vec3, cam)
        world.tick(objects, vec3(*cam), st, rng=other)
        path.append(ps.state(objects)["vel"])
    assert not np.array_equal(np.array(path), z["vel"]) and reached(z)["fields_another_seed_changes"] >= 1


def test_brim_reaches_what_it_is_for():
    """What make_physics_draws.py demanded before it wrote the file: (a) a pass of 1024 tests of two draws from output 624 on, (b) a
    pass of 1024 undecided tests that went both ways, (c) one whose tests all made a second draw, (d) a pass of 1024 contacts, (e)
    only steps of whole passes -- and the passes as recorded say the same."""
    z, spec = ps.load_fixture("brim")
    r = reached(z)
    for key in ("passes_of_1024_two_from_624", "passes_of_1024_open_both_ways", "passes_of_1024_open_all_passed", "passes_of_1024_contacts",
                "passes_of_2048_draws", "order_dependent_sums", "blocked_steps"):
        assert r[key] >= 1, (key, r)
    assert r["steps"] == r["steps_of_whole_passes"] == 9 and r["outside"] == 0
    assert len(spec["objects"]) == 6 and spec["ticks"] == 3 and [m["solidity"] for m in spec["materials"]] == [1, 0.5, 0.75, pds.NEAR, pds.NEAR]
    assert pds.NEAR < 1.0 and math.nextafter(pds.NEAR, 2.0) == 1.0
    tick, obj, step, number, one, two, passed, failed = z["passes"].T
    assert len(tick) == 18 and (one + two + passed + failed == PASS).all() and (one == 0).all()       # every test of every pass drew
    assert two[0] == PASS and (tick[0], obj[0], number[0]) == (0, 1, 0)                                 # the first pass: 624 .. 4719
    assert ((passed + failed == PASS) & (passed > 0) & (failed > 0)).sum() == r["passes_of_1024_open_both_ways"]
    assert (passed == PASS).sum() == r["passes_of_1024_open_all_passed"] == r["passes_of_1024_contacts"]
    assert np.array_equal(np.bincount(tick, weights=one + 2 * two + 2 * passed + failed).astype(np.int64), z["draws"])
    assert (z["pos"] == np.array([o["pos"] for o in spec["objects"]])).all()                            # no plate ever moves


def test_classes_reaches_what_it_is_for():
    z, spec = ps.load_fixture("classes")
    r = reached(z)
    got = [m["solidity"] for m in spec["materials"][:10]]
    assert np.array(got).tobytes() == np.array(pds.STRIPES).tobytes()                                  # NaN and -0.0 survive the JSON
    assert pds.STRIPES[2] == math.nextafter(1.0, 2.0) and pds.STRIPES[8] == 2.0 ** -53 and pds.STRIPES[9] == math.ulp(0.0)
    assert math.isnan(got[4]) and math.copysign(1, got[6]) == -1 and got[3:6:2] == [math.inf, -math.inf]
    for i in range(10):
        assert r["stripe_%d_draws" % i] >= r["stripe_%d_tests" % i] >= 1, (i, r)
    for i in (4, 5, 6, 7, 9):                                                                           # one draw a test, which fails
        assert r["stripe_%d_draws" % i] == r["stripe_%d_tests" % i], (i, r)
    for i in (1, 2, 3):                                                                                 # two under the raft, one in its gap
        assert r["stripe_%d_tests" % i] < r["stripe_%d_draws" % i] < 2 * r["stripe_%d_tests" % i], (i, r)
    assert r["tests_of_two_draws_checked"] >= 3 and r["tests_of_one_draw_checked"] >= 5
    assert r["passes_of_six_stripes"] >= 1 and r["stripes_in_one_pass_max"] >= 6 and r["blocked_steps"] >= 1 and r["outside"] == 0
    assert r["open_passed"] >= 1 and r["open_failed"] >= 1
    assert (z["pos"][-1] == z["pos"][-2]).all() and z["draws"][-1] > PASS                               # the raft rests, and still draws


def test_crowd_fluid_reaches_what_it_is_for():
    z, spec = ps.load_fixture("crowd_fluid")
    r = reached(z)
    for key in ("steps_drawing_on_both_sides_of_1024", "steps_open_on_both_sides_of_1024", "open_passed", "open_failed", "blocked_steps"):
        assert r[key] >= 1, (key, r)
    crowd = json.loads(json.dumps(ps.CROWD))
    assert {k: v for k, v in spec.items() if k not in ("materials", "seed")} == {k: v for k, v in crowd.items() if k not in ("materials", "seed")}
    changed = [(i, a["solidity"], b["solidity"]) for i, (a, b) in enumerate(zip(crowd["materials"], spec["materials"])) if a != b]
    assert changed == [(3, 1, 0.5), (4, 1, 0.75)] and spec["seed"] not in (None, pds.SEED, pds.BRIM_SEED)
    assert len(spec["objects"]) > PASS and z["draws"].sum() > 0


def first_pass_needing_the_eighth_state(passes, index):
    """The number of the first recorded pass for which the kernel fills all eight states of its row, with the generator at word
    `index` when the run begins: the pass can consume outputs index .. index + 2 * (draws it may make) - 1 of the row, and needs
    state (that last position) // 624.  Walked only as far as the number of draws does not depend on what is drawn (no
    undecided test); None if no such pass comes before that."""
    for n, (_, _, _, _, one, two, passed, failed) in enumerate(passes.tolist()):
        if passed + failed:
            return None
        may = one + 2 * two
        if (index + 2 * may - 1) // STATE == ROW - 1:
            return n
        end = index + 2 * may
        index = end - ((end - 1) // STATE if end > STATE else 0) * STATE
    return None


def test_which_start_index_needs_the_eighth_state():
    """273 is the least start index from which a pass of 2048 draws reaches the eighth state (273 + 4095 = 4368 = 7 * 624), 272 the
    greatest from which it does not: brim's first pass is such a pass, and so is its second, whatever the first drew."""
    z, _ = ps.load_fixture("brim")
    assert (z["passes"][:2, 5] == PASS).all()
    first = {i: first_pass_needing_the_eighth_state(z["passes"], i) for i in START_INDICES}
    assert first == {0: 1, 1: 1, 272: 1, 273: 0, 274: 0, 623: 0, 624: 0}
    assert (273 + 4 * PASS - 1) // STATE == ROW - 1 and (272 + 4 * PASS - 1) // STATE == ROW - 2 and (STATE + 4 * PASS - 1) < ROW * STATE
    # the kernel's row is as long as that, and no longer: a shorter one would be written past its end by these very passes
    text = open(os.path.join(nat.HERE, "csrc", "vrt_physics_draws.hip")).read()
    define = lambda name: int(re.search(r"#define %s (\d+)\b" % name, text).group(1))  # noqa: E731
    assert (define("VRT_MT_N"), define("VRT_MT_BLOCKS")) == (STATE, ROW) and "s_mt[VRT_MT_BLOCKS * VRT_MT_N]" in text
    assert "s_open_more[VRT_PHYS_BLOCK + 1]" in text and "s_terms[VRT_PHYS_BLOCK][2]" in text
    common = open(os.path.join(nat.HERE, "csrc", "vrt_physics_common.h")).read()
    assert int(re.search(r"#define VRT_PHYS_BLOCK (\d+)\b", common).group(1)) == PASS
