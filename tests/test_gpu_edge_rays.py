"""The explicit-ray family -- first_hit_kernel, cast_kernel, shade_kernel, path_kernel, pixel_rays_kernel -- over the edge
scenes of tests/edge_scenes.py, where only the frame kernels had been: chunk sizes 8, 32 and 64, resolutions up to 9, worlds
2^26 to 2^27 cells from the origin, origins beside the +-2^28 limit, max_bounces 0.5 and 16 (paths of more than 64 hits, rows
of 348 draws), falloff 0 and 3, 19 materials, dense and sparse grids, no background.

(a) tests/edge_rays.py's ray sets against the oracle: cast_rays, shade_rays and path_rays on 600 arbitrary rays per case.
(b) the frame's own primary rays (Camera.pixel_rays) through the same calls against the frame itself, which is asserted
    against the oracle here and is pinned to the real reference in tests/test_gpu_reference_edges.py.
(c) first_hit against the oracle for every case and camera; the far cases' two cameras as one batch of views.
tests/test_edge_rays_host.py asserts on the CPU what (a) relies on.  Doubles are compared as bit patterns.  The calls have one
schedule: no VRT_* variable is set."""
import numpy as np
import pytest

import edge_rays as er
import oracle_lib as ol
import path_ref as pr
import shade_ref as sr
from edge_scenes import EDGE_CASES, edge_scene
from gpu_util import active, camera_for, launches_of, settings_store
from python_raytracer_amd import _native as nat
from test_gpu_cast import CAST_INSTANCE
from test_gpu_edges import RAY_FIELDS, edge_oracle
from test_gpu_first_hit import assert_records_equal as assert_hits_equal
from test_gpu_first_hit import check_against_oracle, instance, set_pose
from test_gpu_paths import check_paths, unused
from test_gpu_shade import SHADE_INSTANCE, background, cam_for, check_result, rgba_of

pytestmark = pytest.mark.gpu

# the resolution mode a call's kernel instance is compiled for, by the scene's highest resolution: 0 for <= 1, 1 for <= 2, 2
# (the generic instance) beyond; the census names are keyed 1, 2, 3 (SHADE_INSTANCE, CAST_INSTANCE)
RES_MODE = {name: 0 if name == "bounces16" else 2 if name == "res9" else 1 for name in er.ALL_CASES}
RES_MAX = {name: 1 if name == "bounces16" else 9 if name == "res9" else 2 for name in er.ALL_CASES}
FRAMES = [(name, k) for name in er.ALL_CASES for k in range(len(edge_scene(name)[2]))]
FRAME_IDS = ["%s-cam%d" % f for f in FRAMES]


def set_cam(name):
    """The camera a set's rays go through: the case's scene with its own materials and the case's own settings (its pose
    plays no part in an explicit-ray call)."""
    sc, st = er.edge_ray_set(name)[:2]
    cam = cam_for(sc, st, ("edge", name))
    assert int(cam._c_scene(cam._ensure_scene()).max_resolution) == RES_MAX[name]
    return cam


def span_of(st):
    return float(st["dist_max"]) - float(st["dist_min"])


def only_path_kernels(ran):
    """vrt_path_rays' launches are not in the launch census (launch_path): a path_rays call must raise no other family's
    count; its instance is launch_shade's choice for the scene's max_resolution, which set_cam asserts."""
    return not {n for n in ran if not n.startswith("path_kernel")}


# ---- (a) the sets against the oracle -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", er.ALL_CASES)
def test_cast_rays_against_the_oracle(name):
    """The first record of every path, and for a ray that hits nothing the oracle's end state with material 0."""
    sc, st, has_bg, origins, vels, lives, draws, exp, trav = er.edge_ray_set(name)
    rec, counts, paths = er.edge_path_set(name)
    cam = set_cam(name)
    res, ran = launches_of(lambda: cam.cast_rays(origins, vels, lives, max_life=span_of(st)))
    assert ran == {CAST_INSTANCE[RES_MODE[name] + 1]}, (name, ran)
    got = res.numpy()
    found = counts > 0
    want = pr.rows(paths, counts, 1)[:, 0]
    want["step"][~found], want["pos"][~found], want["material"][~found] = exp["step"][~found], exp["pos"][~found], 0
    want["cell"][~found] = np.floor(exp["pos"][~found]).astype(np.int32)
    pr.assert_rows_equal(got, want)
    assert np.array_equal(res.hit_mask().cpu().numpy(), found) and not res.rejected_mask().any()
    stats = res.stats
    assert int(stats[8]) == len(exp) and int(stats[4]) == int(found.sum()) and (np.delete(stats, [4, 8]) == 0).all(), stats


@pytest.mark.parametrize("name", er.ALL_CASES)
def test_shade_rays_against_the_oracle(name):
    """Records, colours and statistics; then the same colours and statistics without records."""
    sc, st, has_bg, origins, vels, lives, draws, exp, trav = er.edge_ray_set(name)
    cam = set_cam(name)
    with background(has_bg):
        res, ran = launches_of(lambda: cam.shade_rays(origins, vels, lives, draws=draws, max_life=span_of(st)))
        assert ran == {SHADE_INSTANCE[RES_MODE[name] + 1, True]}, (name, ran)
        check_result(res, exp)
        assert int(res.stats[11]) == 0 and int(res.stats[9]) == 0 and int(res.stats[10]) == 0
        lean, ran = launches_of(lambda: cam.shade_rays(origins, vels, lives, draws=draws, max_life=span_of(st), want_records=False))
        assert ran == {SHADE_INSTANCE[RES_MODE[name] + 1, False]}, (name, ran)
    assert lean.records is None and np.array_equal(rgba_of(lean), rgba_of(res)) and np.array_equal(rgba_of(lean), sr.packed(exp))
    assert np.array_equal(lean.stats[:11], res.stats[:11])
    if not has_bg:      # a ray that hits nothing stays black: the set ran without a background
        assert (exp["color"][exp["counters"][:, sr.C_HIT] == 0] == 0).all()


@pytest.mark.parametrize("max_hits", [4, 64])
@pytest.mark.parametrize("name", er.ALL_CASES)
def test_path_rays_against_the_oracle(name, max_hits):
    """Every record, count, colour and statistic.  For bounces16 max_hits = 64 truncates: counts still report every hit
    (up to 119), and stats[VRT_S_PATH_TRUNCATED] / [VRT_S_PATH_RECORDS] follow (check_paths)."""
    sc, st, has_bg, origins, vels, lives, draws, exp, trav = er.edge_ray_set(name)
    rec, counts, paths = er.edge_path_set(name)
    cam = set_cam(name)
    with background(has_bg):
        res, ran = launches_of(lambda: cam.path_rays(origins, vels, lives, draws=draws, max_hits=max_hits, max_life=span_of(st)))
    assert only_path_kernels(ran), ran
    check_paths(res, exp, counts, paths, max_hits)
    over = int((counts > max_hits).sum())
    assert int(res.stats[nat.S_PATH_TRUNCATED]) == over and int(res.stats[nat.S_PATH_RECORDS]) == int(np.minimum(counts, max_hits).sum())
    if name == "bounces16" and max_hits == 64:
        got_counts = res.counts.cpu().numpy()
        assert over >= 1 and got_counts.max() == counts.max() > 64 and res.truncated_mask().any()
        full = res.numpy()[counts > 64]
        assert (full["material"] > 0).all()      # every slot of a truncated row is used
    if max_hits == 4:
        assert np.array_equal(res.hit(0).numpy()["material"] > 0, counts > 0) and unused(res.hit(0).numpy()[counts == 0]).all()


def test_bounces16_rows_cut_to_the_median_draw_count():
    """Exactly the rays whose oracle draw count exceeds the width are marked -3 (shade_rays' records, path_rays' counts,
    colour 0, stats[10]); every other ray is unchanged; cast_rays, which takes no draws, is unchanged throughout."""
    name = "bounces16"
    sc, st, has_bg, origins, vels, lives, draws, exp, trav = er.edge_ray_set(name)
    rec, counts, paths = er.edge_path_set(name)
    cam = set_cam(name)
    used = exp["counters"][:, sr.C_DRAW]
    width = int(np.median(used))
    out = used > width
    assert 0 < out.sum() < len(out) and width >= 3
    want, want_counts = exp.copy(), counts.copy()
    want[out] = sr.marker(-3)
    want_counts[out] = -3
    want_paths = [[] if o else p for o, p in zip(out, paths)]
    cut = np.ascontiguousarray(draws[:, :width])
    kw = dict(draws=cut, n_draws=width, max_life=span_of(st))
    res = cam.shade_rays(origins, vels, lives, **kw)
    check_result(res, want)
    assert int(res.stats[10]) == int(out.sum()) and int(res.stats[8]) == int((~out).sum()) and (rgba_of(res)[out] == 0).all()
    assert np.array_equal(res.exhausted_mask().cpu().numpy(), out)
    lean = cam.shade_rays(origins, vels, lives, want_records=False, **kw)
    assert np.array_equal(rgba_of(lean), sr.packed(want)) and np.array_equal(lean.stats[:11], res.stats[:11])
    for max_hits in (4, 64):
        p = cam.path_rays(origins, vels, lives, max_hits=max_hits, **kw)
        check_paths(p, want, want_counts, want_paths, max_hits)
        assert unused(p.numpy()[out]).all() and (rgba_of(p)[out] == 0).all() and int(p.stats[10]) == int(out.sum())
    cast = cam.cast_rays(origins, vels, lives, max_life=span_of(st))
    assert np.array_equal(cast.hit_mask().cpu().numpy(), counts > 0)
    pr.assert_rows_equal(cast.numpy()[counts > 0], pr.rows(paths, counts, 1)[:, 0][counts > 0])


@pytest.mark.parametrize("name", ["far_neg", "res9"])
def test_traversed_box(name):
    """shade_rays with a box over everything the set's rays cross: the order-preserving union of the oracle's per-ray lists,
    the keys' first rays, nothing outside the box."""
    sc, st, has_bg, origins, vels, lives, draws, exp, trav = er.edge_ray_set(name)
    cam = set_cam(name)
    cs = sc.chunk_size
    want = sr.union_in_order(trav)
    lo, hi = want.min(0), want.max(0)
    box = ([int(v) for v in lo], [int(v) for v in (hi - lo) // cs + 1])
    assert len(want) > 20 and np.prod(box[1]) < (1 << 20)
    res = cam.shade_rays(origins, vels, lives, draws=draws, max_life=span_of(st), want_traversed=box)
    check_result(res, exp)
    assert np.array_equal(np.array(res.traversed(cs), np.int64).reshape(-1, 3), want)
    assert np.array_equal(res.numpy()["ntrav"], [len(t) for t in trav]) and int(res.stats[11]) == 0
    keys = res.traversed_keys.cpu().numpy()
    first = {tuple(p): k for k, t in reversed(list(enumerate(trav))) for p in t.tolist()}     # chunk -> its first ray
    cell = (want - lo) // cs
    idx = (cell[:, 0] * box[1][1] + cell[:, 1]) * box[1][2] + cell[:, 2]
    assert np.array_equal(keys[idx] >> 12, [first[tuple(p)] for p in want.tolist()]) and (keys != -1).sum() == len(want)
    lean = cam.shade_rays(origins, vels, lives, draws=draws, max_life=span_of(st), want_traversed=box, want_records=False)
    assert np.array_equal(lean.traversed_keys.cpu().numpy(), keys)


# ---- (b) the frame's own rays against the frame ------------------------------------------------------------------------
_frame_oracle = {}


def frame_oracle(name, k, pixels):
    if name != "no_background":
        return edge_oracle(name, k, pixels)
    if (name, k) not in _frame_oracle:
        sc, st, cams, lens = edge_scene(name)
        _frame_oracle[name, k] = ol.render(sc, st, cams[k][0], cams[k][1], lens, pixels, libm=ol.LIBM_PORTABLE, has_background=False)
    return _frame_oracle[name, k]


def u64(a):
    return np.ascontiguousarray(a).view(np.uint64)


@pytest.mark.parametrize("name,k", FRAMES, ids=FRAME_IDS)
def test_pixel_rays_of_the_edge_frames(name, k):
    """The frame against the oracle (as test_gpu_edges.test_edge_scene_bit_exact asserts it), then its primary rays as
    explicit rays: cast_rays is first_hit, shade_rays gives the frame's own ray records and colours, path_rays the same
    colours, the records' hit counters and first_hit's voxel as its first record.
    Ray slots / used slots, the largest hit count and the largest draw count of a ray, per frame (printed by the test):
        cs64 2400 / 2400, 6, 21;  far_pos 2400 / 2400, 7, 24 and 8, 24;  far_neg 7, 18 and 7, 21;  far_mixed 7, 21 and 8, 24;
        limit_28_pos 6, 21;  limit_28_neg 9, 30;  res9 8, 21;  fov179 1152 / 1152, 9, 27;  fov20 7, 18;  bounces_half 12, 39;
        bounces16 134, 393;  lod_full 15552 / 11689, 9, 24;  dof10 6, 18;  near4 1, 6;  rough25_abs7 12, 39;  fill_sparse 4, 15;
        fill_dense 7, 24;  w1 72 / 72, 3, 12;  h1 96 / 96, 5, 18;  one_pixel 9 / 7, 1, 6;  no_background 5, 18
    (2400 / 2400 where no slots are given; with max_hits = 8 the longer paths truncate, and counts still hold every hit)."""
    import torch
    sc, st, cams, lens = edge_scene(name)
    cs = st["chunk_size"]
    pos, q = cams[k]
    has_bg = name != "no_background"
    cam = camera_for(sc, settings_store(st), pos, q, lens)
    with background(has_bg):
        r = cam.render(0, want_rays=True, want_ray_rgba=True)
        o = frame_oracle(name, k, r.pixels)
        got, exp = active(r), o["rays"]
        assert len(got) == len(exp) == int(r.stats[8]) == o["n_rays"]
        for f in RAY_FIELDS:
            assert np.array_equal(got[f], exp[f]), (k, f, np.flatnonzero((got[f] != exp[f]).reshape(len(got), -1).any(1))[:5])
        assert np.array_equal(r.rgba_f32.cpu().numpy(), o["pix_mean"].astype(np.float32))
        assert np.array_equal(np.array(r.traversed(cs), np.int64).reshape(-1, 3), o["traversed"])
        assert (r.stats[:8] == o["counters"]).all(), (r.stats[:8], o["counters"])

        # the frame's rays as explicit rays
        rays, used_t = cam.pixel_rays(all_samples=True)
        frame = r.rays
        used = used_t.cpu().numpy()
        smax = r.max_samples
        assert len(frame) == len(used) == len(r.pixels) * smax and np.array_equal(used, frame["s"] >= 0)
        n_unused = int((~used).sum())
        span = span_of(st)
        fh = cam.first_hit(all_samples=True).numpy()
        cast = cam.cast_rays(rays, max_life=span)
        cgot = cast.numpy()
        pr.assert_rows_equal(cgot[used], fh[used])
        assert np.array_equal(fh["material"] == -1, ~used)
        assert (cgot["material"][~used] == nat.HIT_REJECTED).all() and int(cast.stats[9]) == n_unused

        # draw rows on the CPU: the row of random.seed((1 + x)(1 + y)(1 + s)) less what the ray generation consumed -- the
        # lod_random draw, and with dof != 0 the two lens draws; asserted from the oracle's draw counters
        first = 1 + 2 * (st["dof"] != 0)
        d = exp["counters"][:, sr.C_DRAW]
        nohit = exp["counters"][:, sr.C_HIT] == 0
        assert (d >= first).all() and ((d - first) % 3 == 0).all() and (d[nohit] == first).all()
        n = int(d.max())
        px = r.pixels.astype(np.int64)
        seeds = ((1 + px[:, 0]) * (1 + px[:, 1]))[:, None] * (1 + np.arange(smax))[None, :]
        rows = np.stack([ol.rng_draws(int(s), first + n) for s in seeds.reshape(-1)])
        drows = torch.from_numpy(np.ascontiguousarray(rows[:, first:])).cuda()

        shade = cam.shade_rays(rays, draws=drows, max_life=span)
        sgot = shade.numpy()
        assert (sgot["s"][used] == 0).all() and (sgot["s"][~used] == -2).all()
        assert int(shade.stats[9]) == n_unused and int(shade.stats[10]) == 0 and int(shade.stats[8]) == int(used.sum())
        a, b = sgot[used], frame[used]
        for f in ("color", "alpha", "ntrav"):
            assert np.array_equal(a[f], b[f]), (f, np.flatnonzero((a[f] != b[f]).reshape(len(a), -1).any(1))[:5])
        for f in ("energy", "step", "life", "bounces", "pos", "vel"):
            assert np.array_equal(u64(a[f]), u64(b[f])), (f, np.flatnonzero((u64(a[f]) != u64(b[f])).reshape(len(a), -1).any(1))[:5])
        shift = np.zeros(8, np.int32)
        shift[sr.C_DRAW] = first
        assert np.array_equal(a["counters"] + shift, b["counters"])
        want_rgba = r.ray_rgba.cpu().numpy().view(np.uint32)
        assert np.array_equal(rgba_of(shade)[used], want_rgba[used])
        want_stats = np.array(r.stats[:8], np.int64)
        want_stats[sr.C_DRAW] -= first * int(used.sum())
        assert np.array_equal(shade.stats[:8], want_stats), (shade.stats[:8], want_stats)

        path = cam.path_rays(rays, draws=drows, max_hits=8, max_life=span)
        counts = path.counts.cpu().numpy()
        assert (counts[~used] == -2).all() and np.array_equal(counts[used], b["counters"][:, sr.C_HIT])
        assert np.array_equal(rgba_of(path)[used], want_rgba[used])
        assert int(path.stats[9]) == n_unused and int(path.stats[10]) == 0 and np.array_equal(path.stats[:9], shade.stats[:9])
        found = used & (fh["material"] > 0)
        pr.assert_rows_equal(path.hit(0).numpy()[found], fh[found])
        assert np.array_equal(counts[used] == 0, fh["material"][used] == 0)
    print(name, k, "slots", len(used), "used", int(used.sum()), "largest hit count", int(b["counters"][:, sr.C_HIT].max()),
          "largest draw count", n)


# ---- (c) first_hit against the oracle ----------------------------------------------------------------------------------
ONE_MATERIAL = ("w1", "one_pixel", "bounces_half")                       # frames that show a single material
# frames whose every ray finds a voxel.  (far_neg's second camera misses with one ray of 2 400: it is held to the general rule)
ALL_HITS = {("fov20", 0), ("fill_dense", 0), ("w1", 0), ("bounces_half", 0), ("one_pixel", 0)}


@pytest.mark.parametrize("name,k", FRAMES, ids=FRAME_IDS)
def test_first_hit_against_the_oracle(name, k):
    """check_against_oracle of tests/test_gpu_first_hit.py (id materials, max_bounces 0) with the case's own condition in
    place of its general one; the values were computed from the oracle and are asserted, not discovered."""
    sc, st, cams, lens = edge_scene(name)
    cam, h, exp = check_against_oracle(sc, st, cams[k][0], cams[k][1], lens, instance(RES_MODE[name] + 1, False), vacuous_ok=True)
    assert int(cam._c_scene(cam._ensure_scene()).max_resolution) == RES_MAX[name]
    hit = exp["material"] > 0
    share = hit.sum() / (exp["material"] >= 0).sum()
    mats = set(exp["material"][hit].tolist())
    print(name, k, "share of rays that hit: %.4f" % share, "materials:", len(mats))
    assert (len(mats) == 1) if name in ONE_MATERIAL else (len(mats) > 1), mats
    assert (share == 1) if (name, k) in ALL_HITS else (0 < share < 1), share


@pytest.mark.parametrize("name", ["far_pos", "far_neg", "far_mixed"])
def test_far_cameras_as_views(name):
    """Both cameras of a far case in one first_hit_views batch and one render_views batch: each view is the single-pose call
    bit for bit, the traversed list and its keys included."""
    from test_gpu_views import assert_view_equals_single
    sc, st, cams, lens = edge_scene(name)
    assert len(cams) == 2
    poses = [(tuple(p), tuple(q)) for p, q in cams]
    cam = camera_for(sc, settings_store(st), *poses[0], lens)
    singles_h, singles_r = [], []
    for p in poses:
        set_pose(cam, p)
        singles_h.append(cam.first_hit(0, all_samples=True))
        singles_r.append(cam.render(0, want_ray_rgba=True))
    set_pose(cam, poses[1])      # (the camera's own pose plays no part in a batch)
    hv, ran = launches_of(lambda: cam.first_hit_views(poses, all_samples=True))
    assert ran == {instance(2, False, views=True)}, ran
    rv = cam.render_views(poses, want_ray_rgba=True)
    assert len(hv) == len(rv) == 2
    for v in range(2):
        assert_hits_equal(hv[v].numpy(), singles_h[v].numpy())
        assert_view_equals_single(rv[v], singles_r[v], st["chunk_size"])
        o = edge_oracle(name, v, rv[v].pixels)
        assert np.array_equal(rv[v].rgba_f32.cpu().numpy(), o["pix_mean"].astype(np.float32))
        assert np.array_equal(np.array(rv[v].traversed(st["chunk_size"]), np.int64).reshape(-1, 3), o["traversed"])
    assert int(hv[0].stats[8]) == sum(int(s.stats[8]) for s in singles_h) and int(hv[0].stats[4]) == sum(int(s.stats[4]) for s in singles_h)
    assert not np.array_equal(hv[0].numpy()["step"], hv[1].numpy()["step"])      # two different views
