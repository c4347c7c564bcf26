"""The first-hit pass (Camera.first_hit / first_hit_views -> vrt_first_hit / vrt_first_hit_views, first_hit_kernel): depth,
voxel and material per primary ray, bit for bit against the CPU oracle.

The oracle needs no change: the state of a ray before its first hit does not depend on any material, so the oracle renders
the same geometry with every material replaced by albedo (id, 0, 0), roughness 0, absorption 1, ior 0, energy 0, with
max_bounces = 0 and no background.  Every ray then breaks at its first voxel (init.py:85); a hit does not move pos or step,
so the oracle's end state IS the first-hit state: pos, step as they are, material = color[0] where the ray counted a hit,
else 0, cell = floor(pos).  Every comparison is exact: the pass does the colour path's own binary64 operations.

Each oracle comparison first asserts that it is not vacuous: more than 10 % of the rays hit, more than 10 % miss, at least 3
distinct materials are hit."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as ol
from gpu_util import HANDOUT_KNOBS, camera_for, launches_of, run_children, settings_store
from python_raytracer_amd import _native as nat

gpu = pytest.mark.gpu

W, H, SAMPLES = 32, 24, 4
IDENTITY = (0.0, 0.0, 0.0, 1.0)
HIT_DTYPE = np.dtype(nat.HIT_FIELDS)
PER_PIXEL = dict(dof=0.0, lod_random=0.0, lod_samples=0.0)   # settings under which the ray table holds one record per pixel


def instance(res_max, per_pixel, views=False):
    """The first_hit_kernel instance a pass runs, with every template argument -- what the launch census must show for the call:
    8 positions at resolution mode 0 / 1 for scenes of resolutions <= 1 / <= 2, 4 at the generic mode 2; the ray table's layout;
    one camera or several."""
    return "first_hit_kernel<%s,%d,%s>" % ({1: "8,0", 2: "8,1", 3: "4,2"}[res_max], bool(per_pixel), "true" if views else "false")


def lens_of(st):
    return st["fov"] * np.pi / 8


def id_materials(n):
    """n material records whose albedo is (id, 0, 0): a ray that breaks at its first voxel carries the voxel's id as its red."""
    mats = np.zeros((n, 7))
    mats[:, 0] = np.arange(1, n + 1)
    mats[:, 4] = 1.0
    return mats


def id_scene(sc):
    return ol.Scene(sc.origin, sc.dims, sc.chunk_size, sc.present, sc.res, sc.grid,
                    id_materials(max(int(sc.grid.max()), len(sc.materials))))


def max_samples(st):
    return max(1, round(st["samples"] * (1 - min(st["lod_edge"], 0.0))))   # vrt_max_samples (init.py:133-134)


def oracle_hits(sc, st, pos, rot, lens, px, vacuous_ok=False):
    """The expected vrt_hit records of pixel list `px`, one per ray slot p * max_samples + s; slots the oracle traced no
    ray for are unused: material -1, everything else 0."""
    o = ol.render(id_scene(sc), dict(st, max_bounces=0.0), pos, rot, lens, px, libm=ol.LIBM_PORTABLE, has_background=False,
                  want_traversed=False)
    rays = o["rays"]
    hit = rays["counters"][:, 4] == 1
    assert (rays["counters"][:, 4] <= 1).all() and (rays["bounces"][~hit] == 0).all()
    assert (rays["step"][~hit] >= rays["life"][~hit]).all()
    if not vacuous_ok:
        assert 0.1 < hit.mean() < 0.9, hit.mean()
        assert len(set(rays["color"][hit, 0].tolist())) >= 3, set(rays["color"][hit, 0].tolist())
    smax = max_samples(st)
    where = {(int(x), int(y)): i for i, (x, y) in enumerate(px)}
    slot = np.array([where[(int(x), int(y))] for x, y in zip(rays["x"], rays["y"])], np.int64) * smax + rays["s"]
    exp = np.zeros(len(px) * smax, HIT_DTYPE)
    exp["material"] = -1
    exp["step"][slot] = rays["step"]
    exp["pos"][slot] = rays["pos"]
    exp["cell"][slot] = np.floor(rays["pos"]).astype(np.int32)
    exp["material"][slot] = np.where(hit, rays["color"][:, 0], 0)
    return exp


def assert_records_equal(got, exp):
    """Bit for bit, field by field (the doubles as their 64-bit patterns: -0.0 is not 0.0 here)."""
    assert got.shape == exp.shape
    assert np.array_equal(got["material"], exp["material"])
    assert np.array_equal(got["cell"], exp["cell"])
    assert np.array_equal(got["step"].view(np.uint64), exp["step"].view(np.uint64))
    assert np.array_equal(got["pos"].view(np.uint64), exp["pos"].view(np.uint64))


def check_against_oracle(sc, st, pos, rot, lens, runs=None, grid=None, vacuous_ok=False):
    """runs: the instance the pass must launch, and no other (None: not asserted)."""
    cam = camera_for(id_scene(sc), settings_store(st), pos, rot, lens, grid=grid)
    h, ran = launches_of(lambda: cam.first_hit(0, all_samples=True))
    assert runs is None or ran == {runs}, (ran, runs)
    exp = oracle_hits(sc, st, pos, rot, lens, h.pixels, vacuous_ok)
    got = h.numpy()
    assert_records_equal(got, exp)
    used = exp["material"] >= 0
    assert int(h.stats[8]) == int(used.sum()) and int(h.stats[4]) == int((exp["material"] > 0).sum())
    assert (np.delete(h.stats, [4, 8]) == 0).all(), h.stats
    return cam, h, exp


def raised_default():
    sc = ol.default_scene()
    return sc, sc.cam_pos + np.array([0.0, 20.0, 0.0]), sc.cam_rot, sc.cam_lens


# the reference of cases 1, 6, 7 and 8: computed once, never changed
_case1 = {}


def case1(per_pixel=False):
    if per_pixel not in _case1:
        sc, pos, rot, lens = raised_default()
        st = ol.make_settings(width=W, height=H, samples=SAMPLES, **(PER_PIXEL if per_pixel else {}))
        cam, h, exp = check_against_oracle(sc, st, pos, rot, lens, instance(2, per_pixel), grid=sc.grid_lod0)
        exp.setflags(write=False)
        _case1[per_pixel] = (cam, st, h, exp)
    return _case1[per_pixel]


# ---- 1. oracle parity ------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("per_pixel", [False, True])
def test_default_scene_against_the_oracle(per_pixel):
    """The raised default camera: resolutions 1 and 2, missing chunks, the chunk table in LDS.  Default settings: one ray
    record per slot; dof = lod_random = lod_samples = 0: one per pixel.  lod_edge thins the samples: unused slots carry -1."""
    cam, st, h, exp = case1(per_pixel)
    assert int(cam._c_scene(cam._ensure_scene()).max_resolution) == 2
    assert (exp["material"] == -1).any() and (exp["material"].reshape(-1, max_samples(st))[:, 0] >= 0).all()
    assert h.samples == h.max_samples == max_samples(st)


@gpu
@pytest.mark.parametrize("per_pixel", [False, True])
def test_synth64_against_the_oracle(per_pixel):
    """A dense world at resolution 1 whose table is an identity table: the entries are computed, not read."""
    sc = ol.synth64_scene()
    st = ol.make_settings(width=W, height=H, samples=SAMPLES, **(PER_PIXEL if per_pixel else {}))
    cam, h, exp = check_against_oracle(sc, st, sc.cam_pos, sc.cam_rot, sc.cam_lens, instance(1, per_pixel))
    c = cam._c_scene(cam._ensure_scene())
    assert int(c.max_resolution) == 1 and (int(c.flags) & nat.SCENE_TABLE_IS_IDENTITY)
    assert len(set(exp["material"][exp["material"] > 0].tolist())) == 13


# ---- 2. generic resolution instance and void skipping ----------------------------------------------------------------
def hand_scene():
    """Four chunks of 8^3 in a box of 4 x 3 x 2: one at resolution 3, one at 2, two at 1, holes between them."""
    cs = 8
    dims = np.array([4, 3, 2])
    origin = np.array([-16, -8, 0], np.int64)
    present = np.zeros(tuple(dims), np.uint8)
    res = np.ones(tuple(dims), np.uint8)
    for cell, r in (((0, 1, 0), 3), ((3, 1, 1), 1), ((1, 2, 1), 2), ((2, 0, 0), 1)):
        present[cell] = 1
        res[cell] = r
    rng = np.random.default_rng(77)
    shape = tuple(dims * cs)
    grid = np.where(rng.random(shape) < 0.5, rng.integers(1, 6, shape), 0).astype(np.uint8)
    return ol.Scene(origin, dims, cs, present, res, ol.Scene.camera_grid(grid, origin, dims, cs, present, res), id_materials(5))


HAND_POSE = ((2.3, 3.6, -14.45), IDENTITY)   # outside the box, looking at it


@gpu
def test_generic_resolutions_and_void_skipping():
    sc = hand_scene()
    st = ol.make_settings(width=W, height=H, samples=SAMPLES, chunk_size=8, dist_max=64)
    cam, h, exp = check_against_oracle(sc, st, *HAND_POSE, lens_of(st), instance(3, False))
    assert int(cam._c_scene(cam._ensure_scene()).max_resolution) == 3


@gpu
def test_generic_resolutions_with_one_ray_record_per_pixel():
    """(the generic instance that reads one record per pixel: no other test runs it)"""
    sc = hand_scene()
    st = ol.make_settings(width=W, height=H, samples=SAMPLES, chunk_size=8, dist_max=64, **PER_PIXEL)
    cam, h, exp = check_against_oracle(sc, st, *HAND_POSE, lens_of(st), instance(3, True))
    assert int(cam._c_scene(cam._ensure_scene()).max_resolution) == 3


# ---- 3. chunk table read from memory ---------------------------------------------------------------------------------
def big_table_scene():
    """17 x 16 x 16 chunks of 8^3, one removed: 4 352 table cells -- more than the march keeps in LDS -- and no identity."""
    cs = 8
    dims = np.array([17, 16, 16])
    origin = -(dims // 2) * cs
    present = np.ones(tuple(dims), np.uint8)
    res = np.ones(tuple(dims), np.uint8)
    present[9, 8, 10] = 0
    rng = np.random.default_rng(78)
    shape = tuple(dims * cs)
    grid = np.where(rng.random(shape) < 0.012, rng.integers(1, 6, shape), 0).astype(np.uint8)
    return ol.Scene(origin, dims, cs, present, res, ol.Scene.camera_grid(grid, origin, dims, cs, present, res), id_materials(5))


@gpu
def test_chunk_table_read_from_memory():
    sc = big_table_scene()
    st = ol.make_settings(width=16, height=12, samples=1, chunk_size=8, dist_max=64)
    cam, h, exp = check_against_oracle(sc, st, (4.3, 0.6, -20.45), IDENTITY, lens_of(st), instance(1, False))
    c = cam._c_scene(cam._ensure_scene())
    assert int(np.prod(sc.dims)) == 4352 > 4096 and not (int(c.flags) & nat.SCENE_TABLE_IS_IDENTITY)


# ---- 4. rotated camera and dist_min > 0 ------------------------------------------------------------------------------
@gpu
def test_rotated_camera_and_dist_min():
    """The golden `rot` pose with dist_min = 3.  At its own position that camera sees a voxel with 97 % of its rays, of two
    materials only (measured on the CPU oracle): it is compared as it is, and once more raised by 10 (68 % hits, three
    materials), where the comparison is not vacuous."""
    g = ol.load_render("rot")
    sc = ol.default_scene()
    st = ol.make_settings(width=W, height=H, samples=SAMPLES, dist_min=3)
    check_against_oracle(sc, st, g["cam_pos"], g["cam_rot"], g["cam_lens"][0], instance(2, False), grid=sc.grid_lod0, vacuous_ok=True)
    check_against_oracle(sc, st, g["cam_pos"] + np.array([0.0, 10.0, 0.0]), g["cam_rot"], g["cam_lens"][0], instance(2, False), grid=sc.grid_lod0)


# ---- 5. consistency with the colour frame ----------------------------------------------------------------------------
@gpu
def test_consistent_with_the_colour_frame():
    """The real materials, default settings: a ray found a voxel in the first-hit pass exactly if the colour frame's ray
    counted a hit, and both passes traced the same rays."""
    sc, pos, rot, lens = raised_default()
    st = ol.make_settings(width=W, height=H, samples=SAMPLES)
    cam = camera_for(sc, settings_store(st), pos, rot, lens, grid=sc.grid_lod0)
    h = cam.first_hit(0, all_samples=True)
    r = cam.render(0, want_rays=True)
    got = h.numpy()
    used = r.rays["s"] >= 0
    assert np.array_equal(got["material"] >= 0, used)
    no_hit = r.rays["counters"][:, nat.COUNTER_NAMES.index("hit")] == 0
    assert np.array_equal(got["material"][used] == 0, no_hit[used])
    assert 0.1 < (got["material"][used] > 0).mean() < 0.9
    assert int(h.stats[4]) == int((used & ~no_hit).sum())
    assert int(h.stats[8]) == int(r.stats[8]) == int(used.sum())
    # ... and the records are those of the same geometry under any materials (case 1's reference)
    assert_records_equal(got, case1()[3])


# ---- 6. all_samples=False and the images -----------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("per_pixel", [False, True])
def test_first_samples_and_images(per_pixel):
    cam, st, h_all, exp = case1(per_pixel)
    smax = max_samples(st)
    h = cam.first_hit(0)
    assert h.samples == 1 and h.max_samples == smax
    first = exp[::smax]
    assert_records_equal(h.numpy(), first)
    assert int(h.stats[8]) == len(first) and int(h.stats[4]) == int((first["material"] > 0).sum())
    # a pixel list that leaves pixels out: they read inf / -1
    keep = np.array([i for i, (x, y) in enumerate(h.pixels) if (x + 2 * y) % 3 != 0])
    sub = cam.first_hit(0, pixels=h.pixels[keep])
    assert_records_equal(sub.numpy(), first[keep])
    depth = sub.depth_image().cpu().numpy()
    mat = sub.material_image().cpu().numpy()
    assert depth.shape == mat.shape == (H, W) and depth.dtype == np.float64 and mat.dtype == np.int32
    e_depth = np.full((H, W), np.inf)
    e_mat = np.full((H, W), -1, np.int32)
    xs, ys = h.pixels[keep][:, 0], h.pixels[keep][:, 1]
    e_depth[ys, xs] = np.where(first["material"][keep] > 0, first["step"][keep], np.inf)
    e_mat[ys, xs] = first["material"][keep]
    assert np.array_equal(depth, e_depth) and np.array_equal(mat, e_mat)
    assert (mat == -1).sum() == H * W - len(keep) and np.isfinite(depth).sum() == (first["material"][keep] > 0).sum()
    # the images of an all-samples result are sample 0's too
    assert np.array_equal(h_all.material_image().cpu().numpy(), h.material_image().cpu().numpy())
    assert np.array_equal(h_all.depth_image().cpu().numpy(), h.depth_image().cpu().numpy())
    # without cached tables (cache_draws unset) they are built for the call and retired after it
    dp = cam._pixels_tensor(0, None)
    assert dp.ray_table is not None
    cam.cache_draws = False
    try:
        uncached = cam.first_hit(0)
    finally:
        cam.cache_draws = True
    assert dp.ray_table is None and dp.draw_table is None
    assert_records_equal(uncached.numpy(), first)
    assert_records_equal(cam.first_hit(0).numpy(), first)


# ---- 7. views --------------------------------------------------------------------------------------------------------
def set_pose(cam, pose):
    from python_raytracer_amd.lib import vec3, quaternion
    cam.pos = vec3(*[float(v) for v in pose[0]])
    cam.rot = quaternion(*[float(v) for v in pose[1]])


def default_poses(n, seed):
    """Poses moved and turned about the raised default camera."""
    sc, pos, rot, lens = raised_default()
    rng = np.random.default_rng(seed)
    poses = [(tuple(pos), tuple(rot))]
    for _ in range(n - 1):
        q = np.array(IDENTITY) + rng.normal(size=4) * 0.25
        poses.append((tuple(pos + rng.uniform(-12, 12, 3)), tuple(q / np.linalg.norm(q))))
    return poses


@gpu
@pytest.mark.parametrize("per_pixel,all_samples", [(False, True), (True, True), (False, False)])
def test_views_equal_single_passes(per_pixel, all_samples):
    cam, st, h0, exp = case1(per_pixel)
    keep = (cam.pos, cam.rot)
    poses = default_poses(5, 5)
    try:
        single = []
        for p in poses:
            set_pose(cam, p)
            single.append(cam.first_hit(0, all_samples=all_samples))
        set_pose(cam, poses[3])   # (the camera's own pose plays no part in a batch)
        got, ran = launches_of(lambda: cam.first_hit_views(poses, all_samples=all_samples))
    finally:
        cam.pos, cam.rot = keep
    assert ran == {instance(2, per_pixel, views=True)}, ran
    assert len(got) == 5
    for b, s in zip(got, single):
        assert_records_equal(b.numpy(), s.numpy())
    assert_records_equal(got[0].numpy(), exp if all_samples else exp[::max_samples(st)])   # the oracle's, for the first view
    assert len({tuple(s.numpy()["material"].tolist()) for s in single}) == 5                # five different views
    assert got[0].stats is not None and int(got[0].stats[8]) == sum(int(s.stats[8]) for s in single)
    assert int(got[0].stats[4]) == sum(int(s.stats[4]) for s in single)
    assert (np.delete(got[0].stats, [4, 8]) == 0).all()


@gpu
@pytest.mark.parametrize("per_pixel", [False, True])
@pytest.mark.parametrize("res_max", [1, 3])
def test_views_of_the_other_resolution_modes_against_the_oracle(res_max, per_pixel):
    """The batched instances no other test runs -- resolution mode 0 (synth64: resolution 1 throughout) and the generic mode
    (the hand scene: resolutions 1, 2 and 3), with either layout of the ray table: three views each, every record of every view
    against the oracle's, the first view's asserted not to be vacuous."""
    if res_max == 1:
        sc = ol.synth64_scene()
        first, lens, kw = (tuple(sc.cam_pos), tuple(sc.cam_rot)), sc.cam_lens, {}
    else:
        sc = hand_scene()
        first, kw = HAND_POSE, dict(chunk_size=8, dist_max=64)
        lens = lens_of(ol.make_settings())
    st = ol.make_settings(width=W, height=H, samples=SAMPLES, **kw, **(PER_PIXEL if per_pixel else {}))
    rng = np.random.default_rng(50 + res_max)
    poses = [first]
    for _ in range(2):   # moved by a few cells and turned a little
        q = np.array(first[1]) + rng.normal(size=4) * 0.1
        poses.append((tuple(np.array(first[0]) + rng.uniform(-3, 3, 3)), tuple(q / np.linalg.norm(q))))
    cam = camera_for(id_scene(sc), settings_store(st), *first, lens)
    assert int(cam._c_scene(cam._ensure_scene()).max_resolution) == res_max
    got, ran = launches_of(lambda: cam.first_hit_views(poses, all_samples=True))
    assert ran == {instance(res_max, per_pixel, views=True)}, ran
    assert len(got) == 3
    for v, (pos, rot) in enumerate(poses):
        assert_records_equal(got[v].numpy(), oracle_hits(sc, st, pos, rot, lens, got[v].pixels, vacuous_ok=v > 0))
    assert len({tuple(g.numpy()["material"].tolist()) for g in got}) == 3   # three different views


@gpu
def test_more_views_than_lds_holds():
    """100 views of 8 x 6 x 1: more than the 96 view records staged in LDS (the rest is read from memory); 48 slots per
    view, so a wave holds rays of two views."""
    sc, pos, rot, lens = raised_default()
    st = ol.make_settings(width=8, height=6, samples=1, lod_edge=0.0)
    cam = camera_for(id_scene(sc), settings_store(st), pos, rot, lens, grid=sc.grid_lod0)
    poses = default_poses(100, 100)
    got = cam.first_hit_views(poses, all_samples=True)
    assert len(got) == 100 and got[0].records.numel() == 48 * 48
    for v in (0, 1, 47, 95, 96, 99):   # against the oracle directly ...
        exp = oracle_hits(sc, st, poses[v][0], poses[v][1], lens, got[v].pixels, vacuous_ok=True)
        assert_records_equal(got[v].numpy(), exp)
    for v, p in enumerate(poses):       # ... and every view against the single pass
        set_pose(cam, p)
        assert_records_equal(got[v].numpy(), cam.first_hit(0, all_samples=True).numpy())
    mats = np.concatenate([g.numpy()["material"] for g in got])
    assert 0.1 < (mats > 0).mean() < 0.9 and len(set(mats[mats > 0].tolist())) >= 3


# ---- the hand-out of first_hit_kernel ----------------------------------------------------------------------------------
def _handout_child():
    """The 64^3 synthetic scene at 31 x 23: every sample, first samples only, and a batch of 3 poses, with one ray record per
    slot and one per pixel; prints one digest, the rays traced and the voxels found per call."""
    import hashlib
    sc = ol.synth64_scene()
    words = []
    for per_pixel in (False, True):
        st = ol.make_settings(width=31, height=23, samples=SAMPLES, **(dict(dof=0.0, lod_random=0.0, lod_samples=0.0) if per_pixel else {}))
        cam = camera_for(id_scene(sc), settings_store(st), sc.cam_pos, sc.cam_rot, sc.cam_lens)
        rng = np.random.default_rng(31)
        poses = [(tuple(sc.cam_pos), tuple(sc.cam_rot))]
        for _ in range(2):
            q = np.array(sc.cam_rot) + rng.normal(size=4) * 0.25
            poses.append((tuple(np.array(sc.cam_pos) + rng.uniform(-6, 6, 3)), tuple(q / np.linalg.norm(q))))
        every = cam.first_hit(0, all_samples=True)
        assert every.numpy().size % 64 != 0 and (every.numpy()["material"] == -1).any(), "no unused sample slot"
        first = cam.first_hit(0, all_samples=False)
        assert first.numpy().size == 31 * 23
        views = cam.first_hit_views(poses, all_samples=True)
        for recs, stats in ((every.numpy(), every.stats), (first.numpy(), first.stats),
                            (np.concatenate([v.numpy() for v in views]), views[0].stats)):
            words += [hashlib.sha256(np.ascontiguousarray(recs).tobytes()).hexdigest(), str(int(stats[8])), str(int(stats[4]))]
    print("HANDOUT", " ".join(words))


@gpu
def test_first_hit_does_not_depend_on_the_hand_out():
    """first_hit_kernel, one camera and several, both ray-table layouts, under the scheduling knobs the frame kernels are tested
    with: the records, the rays traced and the voxels found are the same (the default setting is pinned to the oracle above)."""
    lines = run_children("import test_gpu_first_hit as t; t._handout_child()", HANDOUT_KNOBS, "HANDOUT")
    assert len(lines[0]) == 1 + 2 * 3 * 3
    for knobs, words in zip(HANDOUT_KNOBS, lines):
        print(knobs, [w[:12] for w in words[1:]])
    for knobs, words in zip(HANDOUT_KNOBS[1:], lines[1:]):
        assert words == lines[0], (knobs, words, lines[0])


# ---- 8. graph capture ------------------------------------------------------------------------------------------------
@gpu
def test_first_hit_is_graph_capturable():
    import torch
    cam, st, h0, exp = case1(False)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        cam.first_hit(0, all_samples=True)       # (warm-up on the capturing side: plan, tables, allocator)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        h = cam.first_hit(0, all_samples=True)
    for _ in range(2):
        h.records.zero_()
        h._stats_dev.fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        assert_records_equal(h.numpy(), exp)
        stats = h._stats_dev.cpu().numpy()
        assert int(stats[8]) == int((exp["material"] >= 0).sum()) and int(stats[4]) == int((exp["material"] > 0).sum())
        assert (np.delete(stats, [4, 8]) == 0).all()


# ---- 9. fail-loud ----------------------------------------------------------------------------------------------------
@gpu
def test_first_hit_fails_loudly():
    import torch
    cam, st, h0, exp = case1(False)
    keep = (cam.pos, cam.rot)
    try:
        set_pose(cam, ((float(1 << 28), 0.0, 0.0), IDENTITY))
        with pytest.raises(nat.VrtError, match="vrt_first_hit"):
            cam.first_hit(0)
    finally:
        cam.pos, cam.rot = keep
    poses = default_poses(3, 9)
    far = list(poses)
    far[1] = ((0.0, -float(1 << 28), 0.0), IDENTITY)
    with pytest.raises(ValueError, match="outside the range"):
        cam.first_hit_views(far)
    rec = np.array([list(p) + list(q) + [float(cam.lens)] for p, q in poses])
    rec[2, 7] *= 1.5
    with pytest.raises(ValueError, match="lens"):
        cam.first_hit_views(rec)
    with pytest.raises(ValueError, match="at least one pose"):
        cam.first_hit_views([])
    # the C ABI: a pose out of range and a null ray table are VRT_ERR_ARG, and nothing was launched for them
    L = nat.lib()
    cst = cam._c_settings(0)
    csc = cam._c_scene(cam._ensure_scene())
    dp = cam._pixels_tensor(0, None)
    rtab = dp.ray_table
    assert rtab is not None and dp.plan is not None
    hits = torch.zeros(len(dp.array) * nat.HIT_BYTES, dtype=torch.uint8, device="cuda")
    stats = torch.full((nat.NSTATS,), 7, dtype=torch.int64, device="cuda")

    def call(c, table):
        return L.vrt_first_hit(C.byref(csc), C.byref(cst), C.byref(c), dp.tensor.data_ptr(), len(dp.array), dp.plan.data_ptr(),
                               dp.n_distinct, table, 1, hits.data_ptr(), stats.data_ptr(), None)

    c = cam._c_camera()
    assert call(c, None) == -1
    c.pos[0] = float(1 << 28)
    assert call(c, rtab.data_ptr()) == -1
    torch.cuda.synchronize()
    assert (stats.cpu().numpy() == 7).all() and not hits.any()
    assert call(cam._c_camera(), rtab.data_ptr()) == 0      # ... and the same call with a camera in range runs
    torch.cuda.synchronize()
    assert_records_equal(hits.cpu().numpy().view(HIT_DTYPE), exp[::max_samples(st)])
    # the camera still works
    assert_records_equal(cam.first_hit(0, all_samples=True).numpy(), exp)
