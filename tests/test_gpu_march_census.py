"""Every march instance a launch can select, launched by name and compared with the oracle.

tests/test_march_variant.py pins, on the CPU, which instance the launch policy (march_choose) picks for given plain inputs;
the parity suite pins, on the GPU, that frames equal the oracle's under many knobs.  Every instance is meant to give the same
bits, so nothing in a frame says which of them rendered it: a leg "of the resolution-1 kernel" that ends up in the generic
one stays green.  Here each leg names the instances it must launch, reads the library's launch census
(_native.launch_census: host-side counters next to the launches) before and after its render, and asserts that exactly the
named ones were launched -- then compares the frame with the oracle and asserts the one thing in the statistics or the
scene that shows the instance's distinguishing feature at work.

VRT_SPEC_DEEP and VRT_LOOKUP are read once per process: one child process per pair of them (GROUPS), one test per child,
the children one after another.  The other knobs are read at every launch and change from leg to leg inside a child.
A leg: (scene, settings, per-launch knobs, render arguments, what to observe, the instances it launches).  The names are
written out, as ROWS of tests/test_march_variant.py are; test_legs_cover_every_selectable_instance (no GPU needed) checks
them against that list and against the table in the source.

Every frame launches its two re-trace tiers behind the march (they return at once when their lists are empty): RETRACE is
part of every leg's set, RETRACE_REC of the legs that keep ray records.  The legs marked "retrace1" / "retrace2" are the
ones whose rays really run out of draws, so that those launches have work."""
import os
import re
import subprocess
import sys
import time

import numpy as np
import pytest

import kernel_report
from test_march_variant import ROWS

RETRACE = ('march_kernel<4,2,false,true,0,4,false,false,1>', 'march_kernel<4,2,false,true,0,4,false,false,2>')
RETRACE_REC = ('march_kernel<4,2,true,true,0,4,false,false,1>', 'march_kernel<4,2,true,true,0,4,false,false,2>')

# ---- per-launch knobs (every one of PER_LAUNCH is cleared before a leg sets its own) -------------------------------------------
PER_LAUNCH = ("VRT_POOL", "VRT_POOL_MIN_RAYS", "VRT_WADDR", "VRT_TRAV_LDS", "VRT_TRAV_WINDOW", "VRT_DEFER_VISIT", "VRT_TILED",
              "VRT_FUSE_RAYGEN")
# (read once per process: a child starts without them, but for its group's two)
ONCE = ("VRT_SPEC_DEEP", "VRT_LOOKUP", "VRT_RESMODE", "VRT_DENSE", "VRT_CHUNK", "VRT_MARCH_GRID", "VRT_BATCH_LOG2")
LANES = {"VRT_POOL": "0", "VRT_WADDR": "0"}                               # march_kernel: one ray per lane
POOL = {"VRT_POOL": "1", "VRT_POOL_MIN_RAYS": "0", "VRT_WADDR": "0"}      # march_pool_kernel, whatever the launch's size
LANES_W = {"VRT_POOL": "0", "VRT_WADDR": "1"}                             # ... looking ahead across chunk borders (W)
POOL_W = {"VRT_POOL": "1", "VRT_POOL_MIN_RAYS": "0", "VRT_WADDR": "1"}
DEFER = {"VRT_TRAV_LDS": "0", "VRT_DEFER_VISIT": "2"}                     # no settled bitmap, keys compared behind the voxel reads
TILED = {"VRT_TRAV_LDS": "0", "VRT_DEFER_VISIT": "2", "VRT_TILED": "2"}   # ... and the rays handed out as tiles

# ---- render arguments: Camera.render's, but cache_draws / fast_draws, which are set on the camera --------------------------------
FRAME = dict(want_ray_rgba=True)
UNCACHED = dict(want_ray_rgba=True, cache_draws=False)     # no cached ray table: the march may make the records itself (PERPIX 3)
RECORDS = dict(want_ray_rgba=True, want_rays=True)
FRAME32 = dict(want_ray_rgba=True, fast_draws=32)          # 32 draws per seed in the first pass (the re-trace scenes)
RECORDS32 = dict(want_ray_rgba=True, want_rays=True, fast_draws=32)

# ---- settings: 96 x 54 at 2 samples and 4 bounces; one record per ray slot ("slots": dof and the LOD jitters on) or per pixel ----
PER_PIXEL = dict(dof=0.0, lod_random=0.0, lod_samples=0.0)
SETTINGS = {
    "slots": dict(width=96, height=54, samples=2, max_bounces=4.0, chunk_size=16, dist_max=48),
    "perpix": dict(width=96, height=54, samples=2, max_bounces=4.0, chunk_size=16, dist_max=48, **PER_PIXEL),
    # a window of test_tiled_hand_out_gives_the_same_frame: 128 rays per hand-out are 32 pixels, which divide the height
    "tiles": dict(width=96, height=64, samples=4, max_bounces=4.0, chunk_size=16, dist_max=48),
    "tiles-perpix": dict(width=96, height=64, samples=4, max_bounces=4.0, chunk_size=16, dist_max=48, **PER_PIXEL),
    "retrace1": dict(width=64, height=48, samples=1, max_bounces=5, lod_bounces=0.05),           # test_rng_retrace_path
    "retrace2": dict(width=40, height=30, samples=2, max_bounces=16.0, chunk_size=16, dist_max=200, falloff=0.0, max_light=100.0,
                     lod_bounces=0.0),                                                             # test_third_retrace_tier_many_rough_hits
}
# scene -> the highest resolution among its chunks (asserted when the scene is built: the resolution mode follows from it)
SCENES = {"res1": 1, "res2": 2, "res3": 3, "retrace1": 2, "retrace2": 1}

GROUPS = {  # name -> the once-per-process knobs of its child
    "deep0-lookup0": {"VRT_SPEC_DEEP": "0", "VRT_LOOKUP": "0"},
    "deep0-lookup1": {"VRT_SPEC_DEEP": "0", "VRT_LOOKUP": "1"},
    "deep0-lookup2": {"VRT_SPEC_DEEP": "0", "VRT_LOOKUP": "2"},
    "deep1-lookup0": {"VRT_SPEC_DEEP": "1", "VRT_LOOKUP": "0"},
    "deep1-lookup1": {"VRT_SPEC_DEEP": "1", "VRT_LOOKUP": "1"},
    "deep1-lookup2": {"VRT_SPEC_DEEP": "1", "VRT_LOOKUP": "2"},
}

# What a leg observes besides the census and the frame: "lanes" stats[12] == 0 | "pool" stats[12] & 0xffffffff > 0 | "ahead"
# stats[14] > 0 | "fused" stats[15] > 0 | "tiled" stats[12] >> 32 > 0 | "keys" the frame has traversed keys and no settled bitmap
# | "occ" the scene has an occupancy table | "retrace1" rays beyond the first pass's draws, all finished | "retrace2" rays beyond
# the second tier's 113 draws, all finished | "records" every ray record equals the oracle's.  (The resolutions a leg's scene
# holds -- "a scene with resolution-2 chunks", "resolution-3 chunks that overhang the 16-cell chunk" -- are SCENES' figures.)
LEGS = {
    "deep0-lookup0": [
        ("res1", "slots", LANES, FRAME, ("lanes",), ('march_kernel<4,0,false,false,0,0,false,false,0>',) + RETRACE),
        ("res1", "perpix", LANES, FRAME, ("lanes",), ('march_kernel<4,0,false,false,0,2,false,false,0>',) + RETRACE),
        ("res2", "slots", LANES, FRAME, ("lanes",), ('march_kernel<4,1,false,false,0,0,false,false,0>',) + RETRACE),
        ("res2", "perpix", LANES, FRAME, ("lanes",), ('march_kernel<4,1,false,false,0,2,false,false,0>',) + RETRACE),
        ("res3", "slots", LANES, FRAME, ("lanes",), ('march_kernel<4,2,false,false,0,0,false,false,0>',) + RETRACE),
        ("res3", "perpix", LANES, FRAME, ("lanes",), ('march_kernel<4,2,false,false,0,2,false,false,0>',) + RETRACE),
        ("res1", "slots", POOL, FRAME, ("pool",), ('march_pool_kernel<4,0,0,false,false,false>',) + RETRACE),
        ("res1", "perpix", POOL, FRAME, ("pool",), ('march_pool_kernel<4,0,1,false,false,false>',) + RETRACE),
        ("res2", "slots", POOL, FRAME, ("pool",), ('march_pool_kernel<4,1,0,false,false,false>',) + RETRACE),
        ("res2", "perpix", POOL, FRAME, ("pool",), ('march_pool_kernel<4,1,1,false,false,false>',) + RETRACE),
        ("res3", "slots", POOL, FRAME, ("pool",), ('march_pool_kernel<4,2,0,false,false,false>',) + RETRACE),
        ("res3", "perpix", POOL, FRAME, ("pool",), ('march_pool_kernel<4,2,1,false,false,false>',) + RETRACE),
        # records (want_rays) and the two re-trace tiers, with and without records: one generic instance each, whatever the scene
        ("res3", "slots", LANES, RECORDS, ("lanes", "records"), ('march_kernel<4,2,true,false,0,4,false,false,0>',) + RETRACE_REC),
        ("retrace1", "retrace1", LANES, FRAME32, ("lanes", "retrace1"), ('march_kernel<4,1,false,false,0,0,false,false,0>',) + RETRACE),
        ("retrace2", "retrace2", LANES, FRAME32, ("lanes", "retrace2"), ('march_kernel<4,0,false,false,0,0,false,false,0>',) + RETRACE),
        ("retrace1", "retrace1", LANES, RECORDS32, ("lanes", "records", "retrace1"),
         ('march_kernel<4,2,true,false,0,4,false,false,0>',) + RETRACE_REC),
        ("retrace2", "retrace2", LANES, RECORDS32, ("lanes", "records", "retrace2"),
         ('march_kernel<4,2,true,false,0,4,false,false,0>',) + RETRACE_REC),
    ],
    "deep0-lookup1": [
        ("res1", "slots", LANES, FRAME, ("lanes", "occ"), ('march_kernel<4,0,false,false,1,0,false,false,0>',) + RETRACE),
        ("res1", "perpix", LANES, FRAME, ("lanes", "occ"), ('march_kernel<4,0,false,false,1,2,false,false,0>',) + RETRACE),
        ("res2", "slots", LANES, FRAME, ("lanes", "occ"), ('march_kernel<4,1,false,false,1,0,false,false,0>',) + RETRACE),
        ("res2", "perpix", LANES, FRAME, ("lanes", "occ"), ('march_kernel<4,1,false,false,1,2,false,false,0>',) + RETRACE),
    ],
    "deep0-lookup2": [
        ("res1", "slots", LANES, FRAME, ("lanes", "occ"), ('march_kernel<4,0,false,false,2,0,false,false,0>',) + RETRACE),
        ("res1", "perpix", LANES, FRAME, ("lanes", "occ"), ('march_kernel<4,0,false,false,2,2,false,false,0>',) + RETRACE),
        ("res2", "slots", LANES, FRAME, ("lanes", "occ"), ('march_kernel<4,1,false,false,2,0,false,false,0>',) + RETRACE),
        ("res2", "perpix", LANES, FRAME, ("lanes", "occ"), ('march_kernel<4,1,false,false,2,2,false,false,0>',) + RETRACE),
    ],
    "deep1-lookup0": [
        # one ray per lane, 8 positions: plain (the generic resolution included), look-ahead, late key comparison, no ray table
        ("res1", "slots", LANES, FRAME, ("lanes",), ('march_kernel<8,0,false,false,0,0,false,false,0>',) + RETRACE),
        ("res1", "perpix", LANES, FRAME, ("lanes",), ('march_kernel<8,0,false,false,0,2,false,false,0>',) + RETRACE),
        ("res2", "slots", LANES, FRAME, ("lanes",), ('march_kernel<8,1,false,false,0,0,false,false,0>',) + RETRACE),
        ("res2", "perpix", LANES, FRAME, ("lanes",), ('march_kernel<8,1,false,false,0,2,false,false,0>',) + RETRACE),
        ("res3", "slots", LANES, FRAME, ("lanes",), ('march_kernel<8,2,false,false,0,0,false,false,0>',) + RETRACE),
        ("res3", "perpix", LANES, FRAME, ("lanes",), ('march_kernel<8,2,false,false,0,2,false,false,0>',) + RETRACE),
        ("res1", "slots", LANES_W, FRAME, ("lanes", "ahead"), ('march_kernel<8,0,false,false,0,0,true,false,0>',) + RETRACE),
        ("res1", "perpix", LANES_W, FRAME, ("lanes", "ahead"), ('march_kernel<8,0,false,false,0,2,true,false,0>',) + RETRACE),
        ("res2", "slots", LANES_W, FRAME, ("lanes", "ahead"), ('march_kernel<8,1,false,false,0,0,true,false,0>',) + RETRACE),
        ("res2", "perpix", LANES_W, FRAME, ("lanes", "ahead"), ('march_kernel<8,1,false,false,0,2,true,false,0>',) + RETRACE),
        ("res1", "slots", {**LANES, **DEFER}, FRAME, ("lanes", "keys"), ('march_kernel<8,0,false,false,0,0,false,true,0>',) + RETRACE),
        ("res1", "perpix", {**LANES, **DEFER}, FRAME, ("lanes", "keys"), ('march_kernel<8,0,false,false,0,2,false,true,0>',) + RETRACE),
        ("res1", "slots", {**LANES, **DEFER}, UNCACHED, ("lanes", "keys", "fused"), ('march_kernel<8,0,false,false,0,3,false,true,0>',) + RETRACE),
        ("res2", "slots", {**LANES, **DEFER}, FRAME, ("lanes", "keys"), ('march_kernel<8,1,false,false,0,0,false,true,0>',) + RETRACE),
        ("res2", "perpix", {**LANES, **DEFER}, FRAME, ("lanes", "keys"), ('march_kernel<8,1,false,false,0,2,false,true,0>',) + RETRACE),
        ("res2", "slots", {**LANES, **DEFER}, UNCACHED, ("lanes", "keys", "fused"), ('march_kernel<8,1,false,false,0,3,false,true,0>',) + RETRACE),
        ("res1", "slots", LANES, UNCACHED, ("lanes", "fused"), ('march_kernel<8,0,false,false,0,3,false,false,0>',) + RETRACE),
        ("res2", "slots", LANES, UNCACHED, ("lanes", "fused"), ('march_kernel<8,1,false,false,0,3,false,false,0>',) + RETRACE),
        # the ray pool, 8 positions: the same families, and the tiled hand-out of its DEFER instances
        ("res1", "slots", POOL, FRAME, ("pool",), ('march_pool_kernel<8,0,0,false,false,false>',) + RETRACE),
        ("res1", "perpix", POOL, FRAME, ("pool",), ('march_pool_kernel<8,0,1,false,false,false>',) + RETRACE),
        ("res2", "slots", POOL, FRAME, ("pool",), ('march_pool_kernel<8,1,0,false,false,false>',) + RETRACE),
        ("res2", "perpix", POOL, FRAME, ("pool",), ('march_pool_kernel<8,1,1,false,false,false>',) + RETRACE),
        ("res3", "slots", POOL, FRAME, ("pool",), ('march_pool_kernel<8,2,0,false,false,false>',) + RETRACE),
        ("res3", "perpix", POOL, FRAME, ("pool",), ('march_pool_kernel<8,2,1,false,false,false>',) + RETRACE),
        ("res1", "slots", POOL_W, FRAME, ("pool", "ahead"), ('march_pool_kernel<8,0,0,true,false,false>',) + RETRACE),
        ("res1", "perpix", POOL_W, FRAME, ("pool", "ahead"), ('march_pool_kernel<8,0,1,true,false,false>',) + RETRACE),
        ("res2", "slots", POOL_W, FRAME, ("pool", "ahead"), ('march_pool_kernel<8,1,0,true,false,false>',) + RETRACE),
        ("res2", "perpix", POOL_W, FRAME, ("pool", "ahead"), ('march_pool_kernel<8,1,1,true,false,false>',) + RETRACE),
        ("res1", "slots", {**POOL, **DEFER}, FRAME, ("pool", "keys"), ('march_pool_kernel<8,0,0,false,true,false>',) + RETRACE),
        ("res1", "perpix", {**POOL, **DEFER}, FRAME, ("pool", "keys"), ('march_pool_kernel<8,0,1,false,true,false>',) + RETRACE),
        ("res1", "slots", {**POOL, **DEFER}, UNCACHED, ("pool", "keys", "fused"), ('march_pool_kernel<8,0,3,false,true,false>',) + RETRACE),
        ("res2", "slots", {**POOL, **DEFER}, FRAME, ("pool", "keys"), ('march_pool_kernel<8,1,0,false,true,false>',) + RETRACE),
        ("res2", "perpix", {**POOL, **DEFER}, FRAME, ("pool", "keys"), ('march_pool_kernel<8,1,1,false,true,false>',) + RETRACE),
        ("res2", "slots", {**POOL, **DEFER}, UNCACHED, ("pool", "keys", "fused"), ('march_pool_kernel<8,1,3,false,true,false>',) + RETRACE),
        ("res1", "tiles", {**POOL, **TILED}, FRAME, ("pool", "keys", "tiled"), ('march_pool_kernel<8,0,0,false,true,true>',) + RETRACE),
        ("res1", "tiles-perpix", {**POOL, **TILED}, FRAME, ("pool", "keys", "tiled"), ('march_pool_kernel<8,0,1,false,true,true>',) + RETRACE),
        ("res2", "tiles", {**POOL, **TILED}, FRAME, ("pool", "keys", "tiled"), ('march_pool_kernel<8,1,0,false,true,true>',) + RETRACE),
        ("res2", "tiles-perpix", {**POOL, **TILED}, FRAME, ("pool", "keys", "tiled"), ('march_pool_kernel<8,1,1,false,true,true>',) + RETRACE),
        ("res1", "slots", POOL, UNCACHED, ("pool", "fused"), ('march_pool_kernel<8,0,3,false,false,false>',) + RETRACE),
        ("res2", "slots", POOL, UNCACHED, ("pool", "fused"), ('march_pool_kernel<8,1,3,false,false,false>',) + RETRACE),
    ],
    "deep1-lookup1": [
        ("res1", "slots", LANES, FRAME, ("lanes", "occ"), ('march_kernel<8,0,false,false,1,0,false,false,0>',) + RETRACE),
        ("res1", "perpix", LANES, FRAME, ("lanes", "occ"), ('march_kernel<8,0,false,false,1,2,false,false,0>',) + RETRACE),
        ("res2", "slots", LANES, FRAME, ("lanes", "occ"), ('march_kernel<8,1,false,false,1,0,false,false,0>',) + RETRACE),
        ("res2", "perpix", LANES, FRAME, ("lanes", "occ"), ('march_kernel<8,1,false,false,1,2,false,false,0>',) + RETRACE),
    ],
    "deep1-lookup2": [
        ("res1", "slots", LANES, FRAME, ("lanes", "occ"), ('march_kernel<8,0,false,false,2,0,false,false,0>',) + RETRACE),
        ("res1", "perpix", LANES, FRAME, ("lanes", "occ"), ('march_kernel<8,0,false,false,2,2,false,false,0>',) + RETRACE),
        ("res2", "slots", LANES, FRAME, ("lanes", "occ"), ('march_kernel<8,1,false,false,2,0,false,false,0>',) + RETRACE),
        ("res2", "perpix", LANES, FRAME, ("lanes", "occ"), ('march_kernel<8,1,false,false,2,2,false,false,0>',) + RETRACE),
    ],
}
# Rows of the table that no leg can reach through Camera, by name, each with the chain of conditions that excludes it.
EXEMPT = {}
OBSERVABLES = {"lanes", "pool", "ahead", "fused", "tiled", "keys", "occ", "retrace1", "retrace2", "records"}


# ---- the child ------------------------------------------------------------------------------------------------------------
def build_scene(name):
    """(oracle_lib.Scene, camera position, rotation, lens angle of a 90-degree field of view or the scene's own)."""
    import oracle_lib as ol
    from gpu_util import sparse_scene
    quarter = 90.0 * np.pi / 8
    if name in ("res1", "res2", "res3"):   # 3 x 3 x 3 chunks of 16 cells, some missing, resolutions 1..n
        sc, view = sparse_scene(10 + SCENES[name], SCENES[name], 16, (3, 3, 3)), (np.array([1.5, 2.25, -3.5]), np.array([0.0, 0.0, 0.0, 1.0]), quarter)
    elif name == "retrace1":               # the default scene with weakly absorbing rough materials (test_rng_retrace_path)
        d = ol.default_scene()
        mats = d.materials.copy()
        mats[:, 4] = np.minimum(mats[:, 4], 0.3)
        mats[:, 3] = np.maximum(mats[:, 3], 0.2)
        sc, view = ol.Scene(d.origin, d.dims, 16, d.present, d.res, d.grid, mats), (d.cam_pos, d.cam_rot, d.cam_lens)
    else:                                  # "retrace2": 2 x 2 x 2 dense rough chunks (test_third_retrace_tier_many_rough_hits)
        rng = np.random.default_rng(77)
        dims = np.array([2, 2, 2])
        mats = np.array([[200, 180, 160, 1.0, 0.05, 1.0, 0.0], [90, 120, 250, 0.5, 0.05, 0.5, 0.0]])
        grid = np.where(rng.random(tuple(dims * 16)) < 0.35, rng.integers(1, 3, tuple(dims * 16)), 0).astype(np.uint8)
        sc = ol.Scene(np.array([-16, -16, -16], np.int64), dims, 16, np.ones(tuple(dims), np.uint8), np.ones(tuple(dims), np.uint8), grid, mats)
        view = (np.array([0.5, 0.5, 0.5]), np.array([0.0, 0.0, 0.0, 1.0]), quarter)
    assert int(sc.res[sc.present != 0].max()) == SCENES[name], name
    return (sc,) + view


def run_leg(nat, made, leg):
    """One leg in this process: knobs, census, render, census; then the three assertions."""
    import oracle_lib as ol
    from gpu_util import active, camera_for, frame_equals_oracle, settings_store
    scene, settings, knobs, render, observe, launches = leg
    assert set(observe) <= OBSERVABLES and set(knobs) <= set(PER_LAUNCH)
    key = (scene, settings)
    if key not in made:   # the camera and the oracle's frame: once per (scene, settings), shared by the legs
        sc, pos, rot, lens = build_scene(scene)
        st = ol.make_settings(**SETTINGS[settings])
        cam = camera_for(sc, settings_store(st), pos, rot, lens)
        px = ol.pixel_lists(st["width"], st["height"], 1)[0]
        made[key] = (cam, st, ol.render(sc, st, pos, rot, lens, px, libm=ol.LIBM_PORTABLE))
    cam, st, o = made[key]
    for k in PER_LAUNCH:
        os.environ.pop(k, None)
    os.environ.update(knobs)
    args = dict(render)
    cam.cache_draws = args.pop("cache_draws", True)
    first_draws = cam.fast_draws = args.pop("fast_draws", cam.fast_draws)   # (a frame with many re-traces raises the camera's to 64)
    before = nat.launch_census()
    r = cam.render(0, **args)
    after = nat.launch_census()
    rose = {name for name in after if after[name] > before[name]}
    assert rose == set(launches), ("launched", sorted(rose), "expected", sorted(launches))
    assert np.array_equal(r.pixels, ol.pixel_lists(st["width"], st["height"], 1)[0])
    frame_equals_oracle(r, o, st["chunk_size"])
    stats = [int(v) for v in r.stats]
    groups, tiled_groups = stats[12] & 0xffffffff, stats[12] >> 32
    assert ("lanes" in observe) != ("pool" in observe)
    assert (groups > 0) == ("pool" in observe), stats
    assert (stats[14] > 0) == ("ahead" in observe), stats
    assert (stats[15] > 0) == ("fused" in observe), stats
    assert (tiled_groups > 0) == ("tiled" in observe) and tiled_groups in (0, groups), stats
    if "keys" in observe:
        assert r.traversed_keys is not None and len(o["traversed"]) > 8 and nat.last_plan()["trav_words"] == 0
    if "occ" in observe:
        assert cam._ensure_scene().device_tensors["occupancy"] is not None
    draws = o["rays"]["counters"][:, ol.COUNTERS.index("draw")]
    if "retrace1" in observe:   # rays that outrun the first pass's draws were re-traced, and none was left over
        assert first_draws == 32 and int((draws > 32).sum()) > 0 and stats[9] > 0 and stats[10] == 0, stats
    if "retrace2" in observe:   # ... and rays that outrun the second tier's 113 draws too: only the third tier can have finished them
        assert int((draws > 113).sum()) > 0 and stats[9] >= int((draws > 113).sum()) and stats[10] == 0, stats
    if "records" in observe:
        got = active(r)
        assert len(got) == len(o["rays"]) == stats[8]
        for f in ("x", "y", "s", "color", "alpha", "counters", "ntrav", "energy", "step", "life", "bounces", "pos", "vel"):
            assert np.array_equal(got[f], o["rays"][f]), f
    return sorted(rose)


def run_group(group):
    """The child's main: every leg of `group`, in order.  A leg that fails an assertion is reported and the next one runs; any
    other error (the runtime's included) ends the child there."""
    from python_raytracer_amd import _native as nat
    assert all(os.environ.get(k) == v for k, v in GROUPS[group].items()) and "VRT_RESMODE" not in os.environ
    t0 = time.time()
    made, failed = {}, 0
    for i, leg in enumerate(LEGS[group]):
        try:
            print("LEG", group, i, leg[0], leg[1], " ".join(run_leg(nat, made, leg)), flush=True)
        except AssertionError as e:
            failed += 1
            print("FAILED-LEG", group, i, leg[:2], leg[2], leg[3], repr(e)[:1500], flush=True)
    print("CENSUS-CHILD", group, len(LEGS[group]), failed, "%.2f" % (time.time() - t0), flush=True)
    sys.exit(1 if failed else 0)


# ---- the tests ------------------------------------------------------------------------------------------------------------
_ended_badly = []   # a child that ended on a signal or at its time limit: no further child is started


@pytest.mark.gpu
@pytest.mark.parametrize("group", sorted(GROUPS))
def test_every_leg_launches_its_instances_and_meets_the_oracle(group):
    assert not _ended_badly, "an earlier child ended on a signal or at its limit: %s" % _ended_badly
    here = os.path.dirname(os.path.abspath(__file__))
    env = {k: v for k, v in os.environ.items() if k not in PER_LAUNCH + ONCE}
    env.update(GROUPS[group], PYTHONPATH=os.pathsep.join([here, os.path.dirname(here)]))
    t0 = time.time()
    try:
        out = subprocess.run([sys.executable, "-c", "import test_gpu_march_census as t; t.run_group(%r)" % group], cwd=here, env=env,
                             stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=240)
    except subprocess.TimeoutExpired as e:
        _ended_badly.append((group, "time limit"))
        raise AssertionError((group, "time limit", str(e.stdout)[-2000:]))
    print("census child %s: %.1f s wall" % (group, time.time() - t0))
    print(out.stdout)
    if out.returncode < 0 or out.returncode in (134, 137, 139):
        _ended_badly.append((group, out.returncode))
    assert out.returncode == 0, (group, out.returncode, out.stdout[-6000:])
    done = [l.split() for l in out.stdout.splitlines() if l.startswith("CENSUS-CHILD")]
    assert len(done) == 1 and done[0][1:4] == [group, str(len(LEGS[group])), "0"], done
    assert len([l for l in out.stdout.splitlines() if l.startswith("LEG ")]) == len(LEGS[group])


def test_legs_cover_every_selectable_instance():
    """The union of the legs' sets is the table's selectable rows (all but the record / re-trace variant that neither records
    nor re-traces) less EXEMPT, every name is one ROWS knows, and every family is there.  With the per-leg equality of the GPU
    test: every selectable instance was launched and compared with the oracle.  Needs no GPU."""
    src = open(kernel_report.SRC).read()
    table = re.findall(r"^    X\((\d), (\w+), (\d), (\w+), (\w+), (\d), (\d), (\w+), (\w+), (\w+), (\d)\)", src, re.M)
    spec = {"VRT_SPEC": "4", "VRT_SPEC_DEEP": "8", "8": "8"}
    selectable = set()
    for pool, s, res, rec, lst, lk, pp, w, d, t, seed in table:
        if (rec, lst, pp) == ("false", "false", "4"):
            continue
        selectable.add("march_pool_kernel<%s>" % ",".join((spec[s], res, pp, w, d, t)) if pool == "1" else
                       "march_kernel<%s>" % ",".join((spec[s], res, rec, lst, lk, pp, w, d, seed)))
    assert len(table) == 74 and len(selectable) == 73
    known = {name for _, _, name, _ in ROWS if name}
    assert set(LEGS) == set(GROUPS)
    covered = set()
    for group, legs in LEGS.items():
        for scene, settings, knobs, render, observe, launches in legs:
            assert scene in SCENES and settings in SETTINGS and set(knobs) <= set(PER_LAUNCH) and set(observe) <= OBSERVABLES
            assert len(set(launches)) == len(launches) == 3 and set(launches) <= known, (group, launches)
            covered |= set(launches)
    assert not set(EXEMPT) & covered and set(EXEMPT) <= selectable
    assert covered | set(EXEMPT) == selectable, sorted(selectable ^ (covered | set(EXEMPT)))
    assert len(EXEMPT) == 0

    def args(name):
        return name[:-1].split("<")[1].split(",")
    lanes = [args(n) for n in covered if n.startswith("march_kernel<")]
    pools = [args(n) for n in covered if n.startswith("march_pool_kernel<")]
    # no family is missing as a whole: W, DEFER, TILE, LK 1, LK 2, PERPIX 3, records, each re-trace tier
    assert any(a[6] == "true" for a in lanes) and any(a[3] == "true" for a in pools)
    assert any(a[7] == "true" for a in lanes) and any(a[4] == "true" for a in pools)
    assert any(a[5] == "true" for a in pools)
    assert any(a[4] == "1" for a in lanes) and any(a[4] == "2" for a in lanes)
    assert any(a[5] == "3" for a in lanes) and any(a[2] == "3" for a in pools)
    assert any(a[2] == "true" for a in lanes)
    assert {a[8] for a in lanes if a[3] == "true"} == {"1", "2"}
