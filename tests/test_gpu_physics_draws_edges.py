"""The drawing physics tick (DeviceWorld.tick(rng=), vrt_physics_tick_draws) at the sizes its kernel dimensions itself for: the
three runs recorded from the real reference for them (tests/physics_draw_scenes.py) -- `brim`: passes of 1024 tests that all draw
twice (4096 outputs, all eight states of the LDS row, s_draw[2047]), that are all undecided (s_open_more[1024]), that are all
contacts (s_terms[1023]), steps of exactly two passes; `classes`: the solidities at which the number of draws changes, NaN and the
infinities among them; `crowd_fluid`: undecided tests in candidates on both sides of body 1024 -- tick by tick and bit for bit
against the record and a host twin, the generator's state included; `brim` from the start indices on either side of the one at
which a pass first needs the eighth state (tests/test_physics_draws_edges_host.py works out which pass that is), and from index 0,
which only setstate() gives; host and device ticks taking turns on `brim`; and every recorded all-solid scene through the drawing
tick, where the draws decide nothing and are counted all the same."""
import random

import pytest

import physics_scenes as ps
from test_gpu_physics_draws import run_both
from test_physics_draws_edges_host import NAMES, START_INDICES

gpu = pytest.mark.gpu


def at_index(seed, index):
    """A generator whose next output is word `index` of its state: a fresh seed leaves 624, and 0 is reached by setstate() alone
    (the seeded state, not yet twisted, read from its first word)."""
    gen = random.Random(seed)
    if index == 0:
        version, words, gauss = gen.getstate()
        gen.setstate((version, words[:624] + (0,), gauss))
    elif index != 624:
        for _ in range(index):
            gen.getrandbits(32)
    assert gen.getstate()[1][-1] == index
    return gen


@gpu
@pytest.mark.parametrize("name", NAMES)
def test_device_tick_makes_the_references_draws_at_the_limits(name):
    z, spec = ps.load_fixture(name)
    _, _, total = run_both(name, random.Random(spec["seed"]), random.Random(spec["seed"]))
    assert total == z["draws"].sum() > 0


@gpu
@pytest.mark.parametrize("index", START_INDICES)
def test_brim_from_the_start_indices_about_the_eighth_state(index):
    """From 273 on brim's first pass fills all eight states, from 272 and below its second does; off 624 the draws are not the
    recorded ones, and the comparison is with the host twin alone."""
    _, spec = ps.load_fixture("brim")
    run_both("brim", at_index(spec["seed"], index), at_index(spec["seed"], index), record=index == 624)


@gpu
@pytest.mark.parametrize("first", [0, 1])
def test_host_and_device_ticks_interleave_on_brim(first):
    _, spec = ps.load_fixture("brim")
    run_both("brim", random.Random(spec["seed"]), random.Random(spec["seed"]), device_turn=lambda k: k % 2 == first)


@gpu
@pytest.mark.parametrize("name", ps.DEVICE_SCENES)
def test_every_solid_scene_draws_and_still_equals_its_record(name):
    """Rotation, cells of lod 1, invisible and sleeping neighbours, teleports, the ghost of solidity 0 and the pile meet the
    counting of draws: the count is the host's, the generator ends where the host's does, the run is the recorded one."""
    run_both(name, random.Random(12), random.Random(12))
