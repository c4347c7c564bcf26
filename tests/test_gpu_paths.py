"""Hit paths (Camera.path_rays -> vrt_path_rays, path_kernel) and a frame's primary rays as explicit rays (Camera.pixel_rays ->
vrt_pixel_rays): every voxel a ray shades, bit for bit against tests/path_ref.py's restatement of Camera.trace's loop -- pinned
to the oracle in tests/test_path_host.py, which also asserts what the cases here rely on -- over shade_ref's six ray sets
(resolutions 1, 2 and 3: all three instances), against cast_rays, shade_rays, first_hit and render on the same rays.  Doubles
are compared as bit patterns."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as ol
import path_ref as pr
import shade_ref as sr
from gpu_util import camera_for, settings_store
from python_raytracer_amd import _native as nat
from test_gpu_shade import background, cam_of, rgba_of

gpu = pytest.mark.gpu

ALL_SETS = ["default_mb2", "default_mb8", "default_scaled_nobg", "synth64_mb4", "hand", "big_table"]
MAX_HITS = [4, 32, 1]        # truncating (every set has rays over 4 hits), nothing truncated (the longest path is 19), one
_runs = {}


def unused(rec):
    """Which of these vrt_hit records are exactly the unused record: material -1, every other bit 0."""
    zero = (np.ascontiguousarray(rec["step"]).view(np.uint64) == 0) & (np.ascontiguousarray(rec["pos"]).view(np.uint64) == 0).all(-1)
    return zero & (rec["cell"] == 0).all(-1) & (rec["material"] == -1)


def run(name, max_hits):
    """path_rays over a whole set with its full draw rows: run once per (set, max_hits), shared."""
    if (name, max_hits) not in _runs:
        sc, st, has_bg, origins, vels, lives, draws, exp, trav = sr.ray_set(name)
        with background(has_bg):
            _runs[name, max_hits] = cam_of(name).path_rays(origins, vels, lives, draws=draws, max_hits=max_hits)
    return _runs[name, max_hits]


def check_paths(res, exp, counts, paths, max_hits):
    """Every output of a call against the reference: exp the vrt_ray records (markers for rejected and exhausted rays), counts
    and paths as path_ref gives them."""
    got = res.numpy()
    assert got.shape == (len(exp), max_hits) and res.max_hits == max_hits
    pr.assert_rows_equal(got, pr.rows(paths, counts, max_hits))
    got_counts = res.counts.cpu().numpy()
    assert got_counts.dtype == np.int32 and np.array_equal(got_counts, counts)
    assert np.array_equal(rgba_of(res), sr.packed(exp))
    done = counts >= 0
    stats = res.stats
    print("stats", stats.tolist())
    assert np.array_equal(stats[:11], sr.stats_of(exp)), (stats, sr.stats_of(exp))
    assert int(stats[11]) == 0
    assert int(stats[nat.S_PATH_TRUNCATED]) == int((counts[done] > max_hits).sum())
    assert int(stats[nat.S_PATH_RECORDS]) == int(np.minimum(counts[done], max_hits).sum())
    assert (stats[14:] == 0).all(), stats
    assert np.array_equal(res.truncated_mask().cpu().numpy(), counts > max_hits)
    assert np.array_equal(res.rejected_mask().cpu().numpy(), counts == -2)
    assert np.array_equal(res.exhausted_mask().cpu().numpy(), counts == -3)


# ---- 1. the records, counts, colours and statistics against the restatement ---------------------------------------------
@gpu
@pytest.mark.parametrize("max_hits", MAX_HITS)
@pytest.mark.parametrize("name", ALL_SETS)
def test_against_trace_path(name, max_hits):
    """numpy() is the reference's first max_hits hits of every ray, unused slots exactly the unused record; counts, rgba,
    statistics and the masks."""
    exp, counts, paths = pr.path_set(name)
    res = run(name, max_hits)
    check_paths(res, exp, counts, paths, max_hits)
    if max_hits == 4:
        assert res.truncated_mask().any() and int(res.stats[nat.S_PATH_TRUNCATED]) >= 1
    if max_hits == 32:
        assert not res.truncated_mask().any() and int(res.stats[nat.S_PATH_RECORDS]) == int(counts.sum())
    flat = res.records.cpu().numpy().view(pr.HIT_DTYPE)
    assert flat.shape == (len(exp) * max_hits,)      # one flat buffer of vrt_hit records


# ---- 2. the first record is cast_rays's ------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", ALL_SETS)
def test_first_record_is_cast_rays(name):
    sc, st, has_bg, origins, vels, lives, draws, exp, trav = sr.ray_set(name)
    res = run(name, 1)
    cast = cam_of(name).cast_rays(origins, vels, lives).numpy()
    first = res.hit(0)
    got = first.numpy()
    found = cast["material"] > 0
    assert 0 < found.sum() < len(found) and got.shape == cast.shape
    pr.assert_rows_equal(got[found], cast[found])
    assert np.array_equal(res.counts.cpu().numpy() == 0, ~found)
    assert unused(got[~found]).all()
    assert np.array_equal(first.hit_mask().cpu().numpy(), found) and np.array_equal(first.material.cpu().numpy(), got["material"])
    assert np.array_equal(first.step.cpu().numpy().view(np.uint64), got["step"].view(np.uint64))
    with pytest.raises(IndexError):
        res.hit(1)
    # ... and of a longer row: record j of every ray
    deep = run(name, 4)
    for j in range(4):
        pr.assert_rows_equal(deep.hit(j).numpy(), deep.numpy()[:, j])


# ---- 3. colours and statistics are shade_rays's ----------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", ALL_SETS)
def test_against_shade_rays(name):
    sc, st, has_bg, origins, vels, lives, draws, exp, trav = sr.ray_set(name)
    with background(has_bg):
        shade = cam_of(name).shade_rays(origins, vels, lives, draws=draws, want_records=False)
        lean = cam_of(name).path_rays(origins, vels, lives, draws=draws, max_hits=8, want_rgba=False)
    for max_hits in MAX_HITS:
        res = run(name, max_hits)
        assert np.array_equal(rgba_of(res), rgba_of(shade)) and np.array_equal(res.stats[:11], shade.stats[:11])
    assert lean.rgba is None and np.array_equal(lean.counts.cpu().numpy(), run(name, 4).counts.cpu().numpy())
    pr.assert_rows_equal(lean.numpy()[:, :4], run(name, 4).numpy())


# ---- 4. rays whose draws run out -------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", ALL_SETS)
def test_exhausted_rays(name):
    """Six draws a row: a ray that meets a third rough voxel is not completed -- count -3, every slot unused (its first
    records were stored and are overwritten), rgba 0 -- and every other ray is unchanged."""
    sc, st, has_bg, origins, vels, lives, draws, exp, trav = sr.ray_set(name)
    full, counts, paths = pr.path_set(name)
    out = full["counters"][:, sr.C_DRAW] > 6
    assert 0 < out.sum() < len(out) and (counts[out] >= 3).all()
    want, want_counts = full.copy(), counts.copy()
    want[out] = sr.marker(-3)
    want_counts[out] = -3
    want_paths = [[] if o else p for o, p in zip(out, paths)]
    with background(has_bg):
        res = cam_of(name).path_rays(origins, vels, lives, draws=draws[:, :6], n_draws=6, max_hits=4)
    check_paths(res, want, want_counts, want_paths, 4)
    assert unused(res.numpy()[out]).all() and (rgba_of(res)[out] == 0).all()
    assert int(res.stats[10]) == int(out.sum()) and int(res.stats[8]) == int((~out).sum())


# ---- 5. rejected rays ------------------------------------------------------------------------------------------------
@gpu
def test_rejected_rays():
    sc, st, has_bg, origins, vels, lives, draws, exp, trav = sr.ray_set("default_mb2")
    full, counts, paths = pr.path_set("default_mb2")
    keep = np.nonzero(lives <= 64.0)[0][:100]                # (max_life is 64 below)
    assert len(keep) == 100
    big = float(1 << 28)
    nan = float("nan")
    bad = [([nan, 0, 0], [1, 0, 0], 10),                 # origin not finite
           ([1, 2, 3], [1, 0, 0], 64.5),                 # life > max_life
           ([0, big, 0], [0, 0, 1], 10),                 # origin at 2^28
           ([big - 90, 0, 0], [-1, 0.5, 0], 64),         # reach: 2^28 - 90 + (64 + 2 * 16 + 2) * 1 = 2^28 + 8
           ([1, 2, 3], [0.5, -nan, 0], 10)]              # a NaN that fmax would drop
    at = [0, 63, 64, 70, 104]                            # where the bad ones sit in the 105
    n = 105
    o, v, l, d = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros(n), np.zeros((n, sr.N_DRAWS))
    e, c, p = np.zeros(n, sr.RAY_DTYPE), np.zeros(n, np.int32), [[] for _ in range(n)]
    good = np.setdiff1d(np.arange(n), at)
    o[good], v[good], l[good], d[good], e[good], c[good] = origins[keep], vels[keep], lives[keep], draws[keep], full[keep], counts[keep]
    for i, k in zip(good, keep):
        p[i] = paths[k]
    for i, (bo, bv, bl) in zip(at, bad):
        o[i], v[i], l[i] = bo, bv, bl
        e[i] = sr.marker(-2)
        c[i] = -2
    for max_hits in (4, 1):
        res = cam_of("default_mb2").path_rays(o, v, l, draws=d, max_life=64.0, max_hits=max_hits)
        check_paths(res, e, c, p, max_hits)
        assert int(res.stats[9]) == 5 and int(res.stats[8]) == 100
        assert unused(res.numpy()[at]).all() and (rgba_of(res)[at] == 0).all()
        assert np.array_equal(np.nonzero(res.rejected_mask().cpu().numpy())[0], at)


# ---- 6. sizes --------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("n", [1, 63, 65, 600])
def test_sizes(n):
    import torch
    sc, st, has_bg, origins, vels, lives, draws, exp, trav = sr.ray_set("default_mb8")
    full, counts, paths = pr.path_set("default_mb8")
    cam = cam_of("default_mb8")
    for max_hits in (4, 3):
        res = cam.path_rays(origins[:n], vels[:n], lives[:n], draws=draws[:n], max_hits=max_hits)
        check_paths(res, full[:n], counts[:n], paths[:n], max_hits)
    if n == 600:      # ready records and device draws; another order
        perm = np.random.default_rng(5).permutation(600)
        rec = np.zeros((600, 8))
        rec[:, 0:3], rec[:, 3:6], rec[:, 6] = origins[perm], vels[perm], lives[perm]
        res = cam.path_rays(torch.from_numpy(rec).cuda(), draws=torch.from_numpy(draws[perm]).cuda(), max_hits=4)
        check_paths(res, full[perm], counts[perm], [paths[k] for k in perm], 4)
    if n == 1:        # the host-side checks, and n = 0 through the ABI: the statistics are zeroed and nothing else happens
        for bad in (lambda: cam.path_rays(origins[:5], vels[:5], max_hits=0), lambda: cam.path_rays(origins[:5], vels[:5], max_hits=65),
                    lambda: cam.path_rays(origins[:0], vels[:0]), lambda: cam.path_rays(origins[:5], vels[:4]),
                    lambda: cam.path_rays(origins[:5], vels[:5], seeds=np.arange(5), draws=draws[:5])):
            with pytest.raises(ValueError):
                bad()
        stats = torch.full((nat.NSTATS,), 7, dtype=torch.int64, device="cuda")
        ws = torch.zeros(8192, dtype=torch.uint8, device="cuda")
        cst, csc = cam._c_settings(0), cam._c_scene(cam._ensure_scene())
        assert nat.lib().vrt_path_rays(C.byref(csc), C.byref(cst), None, 0, 64.0, None, 0, 8, ws.data_ptr(), ws.numel(), None, None,
                                       None, stats.data_ptr(), None) == 0
        torch.cuda.synchronize()
        assert (stats.cpu().numpy() == 0).all()


@gpu
def test_records_at_an_address_that_is_only_8_byte_aligned():
    """The C ABI asks 8 bytes of d_hits (vrt_hit's alignment), torch hands out more.  The call through the ABI into an array 8
    bytes off a 16-byte boundary: the same records, and not a byte outside them; 4 bytes off is refused."""
    import torch
    from python_raytracer_amd.results import PathResult
    sc, st, has_bg, origins, vels, lives, draws, exp, trav = sr.ray_set("default_mb8")
    full, counts, paths = pr.path_set("default_mb8")
    cam = cam_of("default_mb8")
    n, max_hits = 600, 4
    rec = np.zeros((n, 8))
    rec[:, 0:3], rec[:, 3:6], rec[:, 6] = origins, vels, lives
    drec, ddraws = torch.from_numpy(rec).cuda(), torch.from_numpy(np.array(draws)).cuda()
    size = n * max_hits * nat.HIT_BYTES
    buf = torch.full((size + 16,), 0x5a, dtype=torch.uint8, device="cuda")
    hits = buf[8:8 + size]
    assert buf.data_ptr() % 16 == 0 and hits.data_ptr() % 16 == 8
    got_counts = torch.empty(n, dtype=torch.int32, device="cuda")
    rgba = torch.empty(n, dtype=torch.uint32, device="cuda")
    stats = torch.empty(nat.NSTATS, dtype=torch.int64, device="cuda")
    ws = torch.zeros(8192, dtype=torch.uint8, device="cuda")
    cst, csc = cam._c_settings(0), cam._c_scene(cam._ensure_scene())
    assert nat.lib().vrt_path_rays(C.byref(csc), C.byref(cst), drec.data_ptr(), n, 192.0, ddraws.data_ptr(), int(ddraws.shape[1]),
                                   max_hits, ws.data_ptr(), ws.numel(), hits.data_ptr(), got_counts.data_ptr(), rgba.data_ptr(),
                                   stats.data_ptr(), torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    check_paths(PathResult(hits, got_counts, rgba, stats, max_hits), full, counts, paths, max_hits)
    edge = buf.cpu().numpy()
    assert (edge[:8] == 0x5a).all() and (edge[-8:] == 0x5a).all()
    assert nat.lib().vrt_path_rays(C.byref(csc), C.byref(cst), drec.data_ptr(), n, 192.0, ddraws.data_ptr(), int(ddraws.shape[1]),
                                   max_hits, ws.data_ptr(), ws.numel(), hits.data_ptr() + 4, got_counts.data_ptr(), rgba.data_ptr(),
                                   stats.data_ptr(), torch.cuda.current_stream().cuda_stream) == -1


# ---- 7. owners of every record ---------------------------------------------------------------------------------------
@gpu
def test_owners_of_every_record():
    """The world of world_build.npz: DeviceWorld.owners takes the records as they are and names, for every used record, the
    object build_world(owners=True) has at that voxel; unused slots are OWNER_NONE."""
    import owner_ref as orf
    from python_raytracer_amd.world import build_world
    from test_gpu_owners import camera_scene, golden
    g = golden()
    dw, cam = g["dw"], g["cam"]
    order = list(dw.order)
    w = build_world(order, 16, owners=True)
    sc = camera_scene(cam, dw, w)
    origins, vels, lives = g["casts"]
    res = cam.path_rays(origins, vels, lives + 48.0, seeds=np.arange(len(lives)) + 1, max_hits=4)
    counts = res.counts.cpu().numpy()
    assert (counts >= 0).all() and (counts >= 2).sum() >= 20, np.bincount(counts)
    own = dw.owners(res.records, cam).numpy()
    h = res.numpy().reshape(-1)
    assert len(own) == len(h) == 4 * len(lives)
    exp, ambiguous = orf.expect_owners(sc, w, order, h)
    used = h["material"] > 0
    assert np.array_equal(used.reshape(-1, 4), np.arange(4)[None, :] < np.minimum(counts, 4)[:, None])
    assert not (exp["object"][used] < 0).any()
    for f in ("object", "resolution", "voxel", "local"):
        assert np.array_equal(own[f], exp[f]), f
    assert (own["object"][~used] == nat.OWNER_NONE).all() and (h["material"][~used] == -1).all()
    later = used.reshape(-1, 4)[:, 1:]
    assert len(set(own["object"].reshape(-1, 4)[:, 1:][later].tolist())) >= 2      # later hits name several objects


# ---- 8. graph capture ------------------------------------------------------------------------------------------------
@gpu
def test_paths_are_graph_capturable():
    import torch
    sc, st, has_bg, origins, vels, lives, draws, exp, trav = sr.ray_set("default_mb2")
    full, counts, paths = pr.path_set("default_mb2")
    cam = cam_of("default_mb2")
    rec = np.zeros((len(exp), 8))
    rec[:, 0:3], rec[:, 3:6], rec[:, 6] = origins, vels, lives
    drec, ddraws = torch.from_numpy(rec).cuda(), torch.from_numpy(draws).cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        cam.path_rays(drec, draws=ddraws, max_hits=4)       # (warm-up on the capturing side: the scene, the allocator, the pow table)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        res = cam.path_rays(drec, draws=ddraws, max_hits=4)
    for _ in range(2):
        res.records.fill_(0x5a)
        res.counts.fill_(77)
        res.rgba.view(torch.uint8).zero_()
        res._stats_dev.fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        res._stats = None
        check_paths(res, full, counts, paths, 4)


# ---- 9. a frame's primary rays ---------------------------------------------------------------------------------------
PIXEL_CASES = {"dof0": dict(dof=0.0), "dof": {}, "per_pixel": dict(dof=0.0, lod_random=0.0, lod_samples=0.0)}
_pixel_cams = {}


def pixel_cam(case):
    """The default scene with its own materials from the raised default camera, a 32 x 24 window with 4 samples."""
    if case not in _pixel_cams:
        sc = ol.default_scene()
        st = ol.make_settings(width=32, height=24, samples=4, **PIXEL_CASES[case])
        assert (st["dof"] != 0) == (case == "dof")
        cam = camera_for(sc, settings_store(st), sc.cam_pos + np.array([0.0, 20.0, 0.0]), sc.cam_rot, sc.cam_lens, grid=sc.grid_lod0)
        _pixel_cams[case] = (cam, st)
    return _pixel_cams[case]


@gpu
@pytest.mark.parametrize("case", list(PIXEL_CASES))
def test_pixel_rays_against_first_hit(case):
    """cast_rays(pixel_rays()) is first_hit() bit for bit on used slots; `used` is false exactly where first_hit marks -1, and
    those records are NaN (so every explicit-ray call rejects them).  With all samples and with the first sample only."""
    import torch
    cam, st = pixel_cam(case)
    for all_samples in (True, False):
        fh = cam.first_hit(all_samples=all_samples)
        want = fh.numpy()
        rays, used = cam.pixel_rays(all_samples=all_samples)
        assert rays.dtype == torch.float64 and rays.is_cuda and tuple(rays.shape) == (len(want), 8) and used.dtype == torch.bool
        u = used.cpu().numpy()
        assert np.array_equal(u, want["material"] != -1)
        if all_samples:
            assert 0 < (~u).sum() < u.sum()
        else:
            assert u.all()
        host = rays.cpu().numpy()
        assert np.isnan(host[~u]).all() and np.isfinite(host[u]).all() and (host[u, 7] == 0).all()
        cast = cam.cast_rays(rays, max_life=float(st["dist_max"]))
        got = cast.numpy()
        pr.assert_rows_equal(got[u], want[u])
        assert (got["material"][~u] == nat.HIT_REJECTED).all() and int(cast.stats[9]) == int((~u).sum())
        assert 0.1 < (want["material"][u] > 0).mean() < 0.95


@gpu
@pytest.mark.parametrize("case", list(PIXEL_CASES))
def test_pixel_rays_against_render(case):
    """The frame's own rays through path_kernel reproduce the frame's per-ray colours: row k of the draws is the row of
    random.seed((1 + x)(1 + y)(1 + s)) less the draws the frame's ray generation consumed -- lod_random's, and with dof != 0
    the two lens draws."""
    import torch
    cam, st = pixel_cam(case)
    first = 3 if case == "dof" else 1
    frame = cam.render(0, want_ray_rgba=True)
    rays, used = cam.pixel_rays(all_samples=True)
    px = frame.pixels.astype(np.int64)
    smax = frame.max_samples
    assert len(rays) == len(px) * smax
    seeds = ((1 + px[:, 0]) * (1 + px[:, 1]))[:, None] * (1 + np.arange(smax))[None, :]
    sd = torch.from_numpy(np.ascontiguousarray(seeds.reshape(-1))).cuda()
    n_draws = 64 + first
    rows = torch.empty((len(sd), n_draws), dtype=torch.float64, device="cuda")
    nat.check(nat.lib().vrt_rng_draws(sd.data_ptr(), len(sd), n_draws, rows.data_ptr(), torch.cuda.current_stream().cuda_stream),
              "vrt_rng_draws")
    res = cam.path_rays(rays, draws=rows[:, first:].contiguous(), max_hits=8, max_life=float(st["dist_max"]))
    u = used.cpu().numpy()
    counts = res.counts.cpu().numpy()
    assert (counts[~u] == -2).all() and (counts[u] >= 0).all() and (counts[u] >= 2).mean() > 0.1
    want = frame.ray_rgba.cpu().numpy().view(np.uint32)
    assert np.array_equal(rgba_of(res)[u], want[u])
    assert int(res.stats[8]) == int(u.sum()) == int(frame.stats[8]) and np.array_equal(res.stats[:5], frame.stats[:5])
    # the first record of every pixel ray is first_hit's
    fh = cam.first_hit(all_samples=True).numpy()
    found = u & (fh["material"] > 0)
    pr.assert_rows_equal(res.hit(0).numpy()[found], fh[found])
    assert np.array_equal(counts[u] == 0, fh["material"][u] == 0)
