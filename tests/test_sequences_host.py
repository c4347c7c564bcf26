"""The scripts of tests/sequences.py reach what their steps are named for: asserted on the CPU, from the oracle and the host
world alone, so that nothing here is measured on the code under test.  tests/test_gpu_sequences.py runs the same scripts on
one long-lived Camera and one long-lived DeviceWorld."""
import numpy as np
import pytest

import cast_ref as cr
import oracle_lib as ol
import owner_ref as orf
import sequences as sq
from python_raytracer_amd.data import PixelList, finalize_settings
from python_raytracer_amd.lib import store
from python_raytracer_amd.world import World

_frames = {}


def walk_frames():
    """(shot, the oracle's frame) of every shot of walk A, computed once."""
    if "a" not in _frames:
        sc = ol.default_scene()
        _frames["a"] = [(s, ol.render(sc, s.st, s.pos, s.rot, s.lens, s.pixels, libm=ol.LIBM_PORTABLE, seed_nonce=s.nonce,
                                      has_background=s.background)) for s in sq.walk_a()]
    return _frames["a"]


def packed(o):
    rays = o["rays"]
    return (rays["color"][:, 0].astype(np.uint32) | (rays["color"][:, 1].astype(np.uint32) << 8) |
            (rays["color"][:, 2].astype(np.uint32) << 16) | (rays["alpha"].astype(np.uint32) << 24))


def by_step(step):
    return [(s, o) for s, o in walk_frames() if s.step == step]


# ---------------------------------------------------------------------------------------------------------------- walk A
def test_walk_a_changes_every_setting_the_library_reads():
    """Every field of vrt_settings the store can change takes at least two values along the walk (chunk_size and its radius
    belong to the scene); has_background and the seed nonce change in steps 16 and 14."""
    shots = sq.walk_a()
    for key in ("width", "height", "samples", "proportions", "shutter", "falloff", "dof", "dist_min", "dist_max", "max_light",
                "max_bounces", "lod_bounces", "lod_samples", "lod_random", "lod_edge", "static", "threads"):
        assert len({s.st[key] for s in shots}) >= 2, key
    assert {s.background for s in shots} == {True, False} and len({s.nonce for s in shots}) == 2
    assert {s.cache_draws for s in shots} == {True, False}
    assert sorted({s.step for s in shots}) == list(range(18))
    assert len({s.lens for s in shots}) == 2 and len({s.pos for s in shots}) == 2


def test_walk_a_flips_the_ray_table_layout_in_steps_3_and_4():
    flips = [sq.per_pixel(s.st) for s in sq.walk_a()]
    shots = sq.walk_a()
    (s3,), (s4,) = [s for s in shots if s.step == 3], [s for s in shots if s.step == 4]
    assert sq.per_pixel(s3.st) and not sq.per_pixel(s4.st) and s4.st["lod_random"] == 0 and s4.st["lod_samples"] == 0
    assert flips.count(True) == 1 and not flips[shots.index(s3) - 1]


def test_walk_a_step_7_has_pixels_with_fewer_samples():
    (s, o) = by_step(7)[0]
    counts = np.bincount(o["rays"]["y"] * s.st["width"] + o["rays"]["x"], minlength=s.st["width"] * s.st["height"])
    assert counts.max() == s.st["samples"] and 1 <= counts.min() < s.st["samples"] and len(set(counts.tolist())) >= 3


def test_walk_a_steps_8_and_9_keep_the_pixel_count():
    (s7, _), (s8, _), (s9, _) = by_step(7)[0], by_step(8)[0], by_step(9)[0]
    assert len(s7.pixels) == len(s8.pixels) == 1200 and s8.st["proportions"] == s7.st["proportions"]
    assert s9.windows == ((64, 16, 1), (16, 64, 1)) and len(s9.pixels) == 1024 == 64 * 16
    # the pixel coordinates of the window before would not fit the new one: a stale list is a wrong frame, not a lucky one
    assert ol.pixel_lists(64, 16, 1)[0][:, 0].max() >= s9.st["width"]


def test_walk_a_step_11_gives_three_traversed_lists():
    lists = [tuple(map(tuple, o["traversed"].tolist())) for _, o in by_step(11)]
    assert len(lists) == 3 and len(set(lists)) == 3
    assert len({(s.st["dist_min"], s.st["dist_max"]) for s, _ in by_step(11)}) == 3


def test_walk_a_step_12_has_at_least_8_pow_bases():
    """The memo of a falloff is indexed by the base 1 + bounces at shading time.  The oracle's ray records hold a ray's
    bounces only as it ended, not at each voxel it shaded -- but with a background every ray ends in lib.material_background,
    whose pow has exactly that base (oracle/vrt_oracle.c, shade_background after the loop): every distinct final count is a
    base that was used at shading time, and the bases of the voxels shaded before can only add to them.  A lower bound."""
    for s, o in by_step(12):
        assert s.background
        b = o["rays"]["bounces"]
        assert len(np.unique(1.0 + b)) >= 8, (s, np.unique(b))
    assert [s.st["falloff"] for s, _ in by_step(12)] == [3.0, 0.0, 0.25]


def test_walk_a_step_13_changes_a_quarter_of_the_colours():
    frames = walk_frames()
    k = [s.step for s, _ in frames].index(13)
    before, after = packed(frames[k - 1][1]), packed(frames[k][1])
    assert before.shape == after.shape and (before != after).mean() >= 0.25


def test_walk_a_every_frame_differs_from_the_one_before_and_hits():
    frames = walk_frames()
    for (sa, a), (sb, b) in zip(frames, frames[1:]):
        same = a["pix_mean"].shape == b["pix_mean"].shape and np.array_equal(a["pix_mean"], b["pix_mean"]) and \
            np.array_equal(packed(a), packed(b))
        assert same == sb.twin, (sa, sb)
    for s, o in frames:
        assert (o["rays"]["counters"][:, ol.COUNTERS.index("hit")] > 0).mean() >= 0.30, s


def test_pixel_cache_key_must_not_outlive_its_list():
    """Camera._pixel_cache holds the uploaded pixels of settings.pixels[thread].  finalize_settings replaces those lists, and
    CPython hands a freed address out again: a key made of id(list) and its length -- what the cache was keyed on -- can equal
    the key of a list that is gone (64 x 16 and 16 x 64 have the same pixel count).  Shown here without a GPU: a second list
    of equal length at the address of a deleted one has the old key.  Camera._cached_pixels, the camera's rule, holds the list
    itself and must miss for every list but that one."""
    from python_raytracer_amd.camera import Camera, DevicePixels
    first = PixelList(ol.pixel_lists(64, 16, 1)[0])
    entry = (first, DevicePixels(None, first.array))
    assert Camera._cached_pixels(entry, first) is entry[1] and Camera._cached_pixels(None, first) is None
    other = ol.pixel_lists(16, 64, 1)[0]
    # (a) while the entry lives, so does its list: no other list can have its address
    second = PixelList(other)
    assert len(second) == len(first) and Camera._cached_pixels(entry, second) is None
    # (b) the key the cache used to keep: free the list, and the address comes back
    old_key = (0, id(first), len(first))
    del entry, first
    found, keep = None, []
    for _ in range(10000):
        cand = PixelList(other)
        if (0, id(cand), len(cand)) == old_key:
            found = cand
            break
        keep.append(cand)          # (held for a while, so that the allocator moves on)
        if len(keep) > 4:
            keep.pop(0)
    if found is None:
        print("no address came back within 10 000 tries: that an id() key can hit a new list was not shown here")
    else:
        print("a 16 x 64 list got the address, and with it the old key, of the deleted 64 x 16 list")
    # a list that changed its length under the same identity misses too
    grown = [(0, 0), (1, 0)]
    entry = (grown, DevicePixels(None, np.array(grown, np.int32)))
    assert Camera._cached_pixels(entry, grown) is entry[1]
    grown.append((2, 0))
    assert Camera._cached_pixels(entry, grown) is None


def test_finalize_settings_replaces_the_pixel_lists():
    s = store(width=64, height=16, threads=1, chunk_size=16)
    finalize_settings(s)
    a = s.pixels[0]
    s.width, s.height = 16, 64
    finalize_settings(s)
    assert s.pixels[0] is not a and len(s.pixels[0]) == len(a) and not np.array_equal(s.pixels[0].array, a.array)


# --------------------------------------------------------------------------------------------------------------- script B
def script_ticks():
    """Script B on the host, tick by tick, computed once: dict(exp, grid, own, world, rows, origin, dims, stale, frame, fresh,
    hits, owners)."""
    if "b" in _frames:
        return _frames["b"]
    from python_raytracer_amd.scene import material_row
    S, cam = sq.ScriptB(), sq.CameraB()
    cs = S.cs
    out, rays = [], None
    for k in range(sq.N_TICKS_B):
        exp = S.run(k)
        S.done()
        w, grid, own = S.host_world()
        rows = np.array([material_row(m)[:7] for m in w.materials], np.float64).reshape(-1, 7)
        origin, dims = S.origin.copy(), S.dims.copy()
        present = sq.present_of(grid, cs)
        if exp["full"]:
            cam.new_scene()
        if k == 0:
            rays = S.make_rays()
            cam.traversed = sq.render_b(k, cam.scene(origin, dims, cs, grid, rows))["traversed"]
        if k % sq.SELECT_EVERY == 0:
            cam.select(k, origin, dims, cs, present)
        stale = cam.table is not None and cam.selected_at != k
        scene = cam.scene(origin, dims, cs, grid, rows)
        frame = sq.render_b(k, scene)
        fresh = None
        if stale:
            table = sq.fresh_selection(k, origin, dims, cs, present, cam.traversed)
            other = sq.CameraB()
            other.table = table
            fresh = sq.render_b(k, other.scene(origin, dims, cs, grid, rows))
        cam.traversed = frame["traversed"]
        hits = cr.march_records(scene, round(cs / 2), *rays)
        host = World(origin, dims, cs, present, grid, w.materials, own)
        owners = orf.expect_owners(scene, host, exp["order"], hits)[0]["object"][hits["material"] > 0]
        out.append(dict(exp=exp, grid=grid, own=own, world=w, origin=origin, dims=dims, stale=stale, frame=frame, fresh=fresh,
                        hits=hits, owners=owners, mats=[S.mats.index(m) for m in w.materials]))
    _frames["b"] = out
    return out


def test_script_b_runs_every_operation_twice_and_every_combination():
    ticks = script_ticks()
    ops = [op for t in ticks for op in t["exp"]["ops"]]
    for op in sq.OPERATIONS:
        assert ops.count(op) >= 2, op
    for op in sq.COMBINATIONS:
        assert ops.count(op) >= 1, op
    assert all(1 <= len([op for op in t["exp"]["ops"] if op in sq.OPERATIONS]) <= 3 for t in ticks[1:]
               if "no_operation" not in t["exp"]["ops"])
    assert ticks[sq.QUIET_TICKS[0]]["exp"]["ops"] == ["no_operation"]
    # the tick after a new material is the rebuild; the hidden object's edit is shown three ticks later
    k = [i for i, t in enumerate(ticks) if "rebuild_after_new_material" in t["exp"]["ops"]][0]
    assert "new_material" in ticks[k - 1]["exp"]["ops"] and ticks[k]["exp"]["full"]
    k = [i for i, t in enumerate(ticks) if "edit_hidden" in t["exp"]["ops"]][0]
    assert "show" in ticks[k + 3]["exp"]["ops"]


def test_script_b_the_grid_changes_on_every_tick_but_the_quiet_ones():
    ticks = script_ticks()
    for k in range(1, len(ticks)):
        a, b = ticks[k - 1], ticks[k]
        same = a["grid"].shape == b["grid"].shape and np.array_equal(a["origin"], b["origin"]) and \
            np.array_equal(a["grid"], b["grid"]) and a["mats"] == b["mats"]
        assert same == (k in sq.QUIET_TICKS), k


def test_script_b_rebuild_counts():
    ticks = script_ticks()
    total = [int(np.prod(t["dims"])) for t in ticks]
    full = [k for k, t in enumerate(ticks) if k and t["exp"]["full"]]
    assert len(full) >= 3, full
    assert sum(0 < t["exp"]["chunks"] < n / 4 for t, n in zip(ticks, total)) >= 10
    assert [k for k, t in enumerate(ticks) if t["exp"]["chunks"] == 0] == list(sq.QUIET_TICKS)
    assert max(total) <= 6 * 6 * 6 and max(int(d) for t in ticks for d in t["dims"]) <= 8, (max(total))


def test_script_b_materials_reach_ten_and_are_renumbered():
    ticks = script_ticks()
    assert len(ticks[0]["mats"]) == 8 and max(len(t["mats"]) for t in ticks) == 10
    renumbered = [k for k, t in enumerate(ticks) if k and t["exp"]["full"]
                  and [m for m in t["mats"] if m in ticks[k - 1]["mats"]] != [m for m in ticks[k - 1]["mats"] if m in t["mats"]]]
    assert renumbered, "no full rebuild changed the first-use order of the materials"
    k = [i for i, t in enumerate(ticks) if "rebuild_after_new_material" in t["exp"]["ops"]][0]
    assert len(ticks[k]["mats"]) == 10


def test_script_b_owner_rays_find_many_objects_and_seldom_miss():
    ticks = script_ticks()
    many = 0
    for k, t in enumerate(ticks):
        miss = (t["hits"]["material"] <= 0).mean()
        assert miss < 0.20, (k, miss)
        assert (t["owners"] >= 0).all()
        many += len(set(t["owners"].tolist())) >= 6
    assert many >= len(ticks) / 2, many


def test_script_b_stale_tables_show():
    """On the ticks between two selections the camera marches the table of the last one over a world that has changed: the
    frame it must give differs from the frame a selection of that very tick would give."""
    ticks = script_ticks()
    stale = [k for k, t in enumerate(ticks) if t["stale"]]
    assert len(stale) >= 15 and all(k % sq.SELECT_EVERY for k in stale)
    differ = [k for k in stale if not np.array_equal(ticks[k]["frame"]["pix_mean"], ticks[k]["fresh"]["pix_mean"])]
    assert len(differ) >= 3, differ
    # ... and no frame is empty: the wide lens leaves the objects a fifth of the window, never less than a tenth
    hit = [(t["frame"]["rays"]["counters"][:, ol.COUNTERS.index("hit")] > 0).mean() for t in ticks]
    assert min(hit) >= 0.1, hit
