"""The surface pass on the GPU (Camera.surfaces -> vrt_hit_surfaces, surface_kernel): how the surface lies at every hit record
of cast_rays(), path_rays() and first_hit().  Two references, both independent of the kernel: tests/surface_ref.py, which
tests/test_surface_host.py holds to the pinned restatement of the renderer's loop on the CPU, and the device's own
shade_kernel run to the step after each hit.  Section 2b holds the pass at the edges: the edge scenes' ray sets and frames, rays
that end on chunk faces, more records than one stride of the kernel's loop, hit records aligned to 8 bytes only."""
import numpy as np
import pytest

import cast_ref as cr
import shade_ref as sr
import surface_ref as sf
from gpu_util import camera_for, settings_store
from python_raytracer_amd import _native as nat

gpu = pytest.mark.gpu
IDENTITY = (0.0, 0.0, 0.0, 1.0)
SURFACE_WORDS = [nat.S_SURFACE_RESOLVED, nat.S_SURFACE_EXAMINED, nat.S_SURFACE_ORPHANS, nat.S_SURFACE_AMBIGUOUS, nat.S_SURFACE_INVALID,
                 nat.S_SURFACE_ENCLOSED]
MAX_LIFE = 256.0            # above every life of the cases (res9's reach 200)
_cams = {}


def case_camera(name, rough=False):
    """(case, camera over its scene), made once."""
    key = (name, rough)
    if key not in _cams:
        c = sf.case(name, rough)
        st = c["settings"]
        _cams[key] = (c, camera_for(c["scene"], settings_store(st), (0.0, 0.0, 0.0), IDENTITY, st["fov"] * np.pi / 8))
    return _cams[key]


def check_none_records(got, hits):
    """Every record that is no hit -- a miss, an unused sample slot, a rejected ray -- has status -1 and zero fields."""
    none = hits["material"] <= 0
    assert (got["status"][none] == nat.SURFACE_NONE).all() and (got["status"][~none] != nat.SURFACE_NONE).all()
    blank = got[got["status"] < 0].copy()
    blank["status"] = 0
    assert not np.frombuffer(blank.tobytes(), np.uint8).any()


def upload(a):
    import torch
    return torch.from_numpy(np.frombuffer(a.tobytes(), np.uint8).copy()).cuda()


def check_records(c, cam, least):
    """cast_rays, then surfaces, over the case's rays: the march's records are the restatement's, the surface records and the
    statistics words the reference's, byte for byte.  Returns (the SurfaceResult, its records)."""
    hits = cam.cast_rays(c["origins"], c["vels"], c["lives"], max_life=MAX_LIFE)
    h = hits.numpy()
    cr.assert_records_equal(h, c["hits"])                      # the march itself is the restatement's
    res = cam.surfaces(hits, (c["origins"], c["vels"]))
    got = res.numpy()
    exp, stats, recs = sf.expect(c["scene"], h, c["vels"])
    sf.assert_records_equal(got, exp)
    assert np.array_equal(res.stats, stats), (res.stats, stats)
    assert int(stats[nat.S_SURFACE_RESOLVED]) >= least and (np.delete(res.stats, SURFACE_WORDS) == 0).all()
    check_none_records(got, h)
    return res, got


# ---- 1. against the reference ------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("rough", [False, True])
@pytest.mark.parametrize("name", sf.CASES)
def test_records_equal_the_reference(name, rough):
    c, cam = case_camera(name, rough)
    res, got = check_records(c, cam, 100)
    if name == "lod":
        assert int(res.stats[nat.S_SURFACE_AMBIGUOUS]) == 1
    # the views of SurfaceResult are the record's fields
    for f in ("vel", "next", "normal", "status", "neighbour", "resolution", "reflect", "side", "fetched", "open"):
        assert np.array_equal(getattr(res, f).cpu().numpy(), got[f], equal_nan=True), f
    bits = res.reflect_mask().cpu().numpy()
    assert bits.shape == (len(got), 3) and np.array_equal(bits, (got["reflect"][:, None] >> np.arange(3)) & 1 == 1)
    assert np.array_equal(res.surface_mask().cpu().numpy(), got["status"] == 0)


# ---- 2. the device against the device ----------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", sf.CASES)
def test_pass_equals_the_shaded_ray_one_step_on(name):
    """shade_rays with the life that ends each ray with the step after its first hit: the end state's vel and pos are the
    pass's vel and next bit for bit.  The materials are smooth, so no draw is consumed."""
    c, cam = case_camera(name)
    hits = cam.cast_rays(c["origins"], c["vels"], c["lives"], max_life=MAX_LIFE)
    got = cam.surfaces(hits, (c["origins"], c["vels"])).numpy()
    check_one_step_on(c, cam, got, 100)


def check_one_step_on(c, cam, got, least):
    """The surface records `got` of the case's rays against shade_rays run to the step after each first hit."""
    hit = np.flatnonzero(got["status"] == 0)
    assert len(hit) >= least and np.array_equal(hit, np.flatnonzero(c["hits"]["material"] > 0))
    shaded = cam.shade_rays(c["origins"][hit], c["vels"][hit], c["end_lives"][hit], max_life=float(c["end_lives"].max()) + 1.0,
                            want_records=True)
    rec = shaded.numpy()
    assert (rec["s"] == 0).all() and (rec["counters"][:, 4] == 1).all()
    # a record two chunks explain differently may name the other chunk: the ray's own is only known to the march
    exp, stats, recs = sf.expect(c["scene"], c["hits"], c["vels"])
    known = np.array([recs[k]["chunk"] == c["truth"][k][3] for k in hit])
    assert int((~known).sum()) <= int(stats[nat.S_SURFACE_AMBIGUOUS])
    assert np.array_equal(rec["vel"][known].view(np.uint64), got["vel"][hit][known].view(np.uint64))
    assert np.array_equal(rec["pos"][known].view(np.uint64), got["next"][hit][known].view(np.uint64))


# ---- 2b. the edge scenes ---------------------------------------------------------------------------------------------------
EDGE_SETS = [("edge", n) for n in sf.edge_names()] + [("lattice", n) for n in sf.LATTICE_CASES]
EDGE_FRAMES = ("far_pos", "far_neg", "limit_28_pos", "limit_28_neg", "cs64", "fill_dense")


def edge_camera(kind, name):
    """(case, camera over its scene with the case's own settings), made once."""
    key = (kind, name)
    if key not in _cams:
        c = sf.edge_case(name) if kind == "edge" else sf.lattice_case(name)
        st = c["settings"]
        _cams[key] = (c, camera_for(c["scene"], settings_store(st), (0.0, 0.0, 0.0), IDENTITY, st["fov"] * np.pi / 8))
    return _cams[key]


@gpu
@pytest.mark.parametrize("kind,name", EDGE_SETS, ids=["%s-%s" % k for k in EDGE_SETS])
def test_edge_records_equal_the_reference(kind, name):
    """The pass over the edge scenes of tests/edge_scenes.py -- chunk sizes 8, 32 and 64, worlds 2^26 to 2^27 cells out on
    either side, beside +-2^28, resolutions up to 9, a dense and a 0.5 % grid -- with the rays of tests/edge_rays.py ("edge") and
    with rays that end exactly on chunk faces ("lattice": the candidates m = 1..7 of the chunk rule, chunk index -1, probes at
    index = dims; tests/test_surface_host.py counts them): the reference's bytes and statistics, then the device's own shaded
    ray one step on."""
    from edge_rays import SMALL
    c, cam = edge_camera(kind, name)
    least = 20 if name in SMALL else 150
    res, got = check_records(c, cam, least)
    check_one_step_on(c, cam, got, least)


@gpu
@pytest.mark.parametrize("name", EDGE_FRAMES)
def test_edge_frames(name):
    """first_hit(all_samples=True), pixel_rays and surfaces of the case's first camera (40 x 30 pixels of 2 samples: 2400
    sample slots, every one compared) over the case's scene with the smooth materials, against the reference.
    Resolved / enclosed records and the largest |pos| of a hit, as printed: far_pos 2376 / 60, 67108909.6; far_neg 2331 / 312,
    134217727.2; limit_28_pos 1809 / 248, 268433375.9; limit_28_neg 2035 / 0, 268433364.9; cs64 1207 / 67; fill_dense 2400 / 1149."""
    from edge_scenes import edge_scene
    c = sf.edge_case(name)
    sc = c["scene"]
    _, st, cams, lens = edge_scene(name)
    cam = camera_for(sc, settings_store(st), cams[0][0], cams[0][1], lens)
    frame = cam.first_hit(all_samples=True)
    rays, used = cam.pixel_rays(all_samples=True)
    res = cam.surfaces(frame, (rays, used))
    h, got = frame.numpy(), res.numpy()
    assert len(h) == len(frame.pixels) * frame.samples <= 20000 and np.array_equal(used.cpu().numpy(), h["material"] != -1)
    check_none_records(got, h)
    exp, stats, recs = sf.expect(sc, h, rays.cpu().numpy()[:, 3:6])
    sf.assert_records_equal(got, exp)
    assert np.array_equal(res.stats, stats), (res.stats, stats)
    resolved = int(stats[nat.S_SURFACE_RESOLVED])
    print(name, "slots", len(h), "resolved", resolved, "enclosed", int(stats[nat.S_SURFACE_ENCLOSED]),
          "largest |pos|", float(np.abs(h["pos"][h["material"] > 0]).max()))
    assert resolved > 100 and int(stats[nat.S_SURFACE_ORPHANS]) == 0 == int(stats[nat.S_SURFACE_INVALID])
    assert resolved == int((h["material"] > 0).sum())


def _source_define(name):
    import os
    import re
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "python_raytracer_amd", "csrc", "vrt_surface.hip")
    return int(re.search(r"^#define %s (\d+)$" % name, open(path).read(), re.M).group(1))


def _edited_lod():
    """The `lod` case's hit records and velocities with one record made an orphan (another material than its voxel's) and one
    refused (a cell that is not floor(pos)); the reference over them."""
    c, cam = case_camera("lod")
    h, vels = c["hits"].copy(), c["vels"]
    good = np.flatnonzero(h["material"] > 0)
    h["material"][good[5]] = h["material"][good[5]] % len(c["scene"].materials) + 1
    h["cell"][good[9], 1] += 1
    exp, stats, recs = sf.expect(c["scene"], h, vels)
    assert exp["status"][good[5]] == nat.SURFACE_ORPHAN and exp["status"][good[9]] == nat.SURFACE_INVALID
    assert recs[-1].get("ambiguous") and (h["material"] <= 0).sum() >= 10
    return c, cam, h, vels, exp, stats, recs


@gpu
def test_more_records_than_one_stride():
    """surface_kernel strides: at most VRT_SURFACE_GRID workgroups of VRT_BLOCK lanes loop over the records.  With
    n = 2 GRID BLOCK + 3 BLOCK + 37 records every workgroup takes a second trip, four a third, and the last of those is partial
    (37 lanes); the per-wave counts are summed across the trips.  The records are the edited `lod` set tiled on the device."""
    import torch
    grid, block = _source_define("VRT_SURFACE_GRID"), _source_define("VRT_BLOCK")
    n = 2 * grid * block + 3 * block + 37
    assert (grid, block, n) == (2048, 256, 1049381)
    c, cam, h, vels, exp, stats, recs = _edited_lod()
    m = len(h)
    idx = torch.arange(n, device="cuda") % m
    d_hits = upload(h).view(m, nat.HIT_BYTES)[idx].reshape(-1)
    one = torch.zeros((m, 8), dtype=torch.float64, device="cuda")
    one[:, 3:6] = torch.from_numpy(vels.copy()).cuda()
    d_rays = one[idx].contiguous()
    res = cam.surfaces(d_hits, d_rays)
    out = res.records.view(n, nat.SURFACE_BYTES)
    first = out[:m]
    got = first.cpu().numpy().reshape(-1).view(sf.SURFACE_DTYPE)
    sf.assert_records_equal(got, exp)
    full = n // m
    assert full >= 1000
    tiles = out[: full * m].view(full, m * nat.SURFACE_BYTES)
    assert torch.equal(tiles, tiles[:1].expand_as(tiles))
    assert torch.equal(out[full * m:], first[: n - full * m]) and 0 < n - full * m < m
    # the six words: the per-record counts of the reference summed over the n records
    ok = exp["status"] == 0
    per = {nat.S_SURFACE_EXAMINED: h["material"] > 0, nat.S_SURFACE_RESOLVED: ok, nat.S_SURFACE_ORPHANS: exp["status"] == nat.SURFACE_ORPHAN,
           nat.S_SURFACE_AMBIGUOUS: np.array([bool(r.get("ambiguous")) for r in recs]), nat.S_SURFACE_INVALID: exp["status"] == nat.SURFACE_INVALID,
           nat.S_SURFACE_ENCLOSED: ok & ~exp["normal"].any(1)}
    want = np.zeros(nat.NSTATS, np.int64)
    for word, flags in per.items():
        assert int(flags.sum()) == int(stats[word]) >= 1
        want[word] = full * int(flags.sum()) + int(flags[: n - full * m].sum())
    assert np.array_equal(res.stats, want), (res.stats, want)


@gpu
def test_hit_records_aligned_to_8_bytes_only():
    """d_hits may be 8-byte aligned only: the same records at byte offset 8 of a 64-byte aligned buffer, through
    Camera.surfaces, give the aligned call's bytes and statistics."""
    import torch
    c, cam, h, vels, exp, stats, recs = _edited_lod()
    nbytes = len(h) * nat.HIT_BYTES
    aligned = upload(h)
    assert aligned.data_ptr() % 64 == 0
    want = cam.surfaces(aligned, (c["origins"], vels))
    sf.assert_records_equal(want.numpy(), exp)
    buf = torch.zeros(nbytes + 128, dtype=torch.uint8, device="cuda")
    at = (-buf.data_ptr()) % 64 + 8
    view = buf[at:at + nbytes]
    view.copy_(aligned)
    assert view.data_ptr() % 16 == 8 and view.data_ptr() % 64 == 8
    got = cam.surfaces(view, (c["origins"], vels))
    assert torch.equal(got.records, want.records) and np.array_equal(got.stats, want.stats) and np.array_equal(got.stats, stats)


# ---- 3. a frame --------------------------------------------------------------------------------------------------------------
def check_frame(cam, dw, w):
    from test_gpu_owners import camera_scene
    frame = cam.first_hit(all_samples=True)
    rays, used = cam.pixel_rays(all_samples=True)
    res = cam.surfaces(frame, (rays, used))
    h, got = frame.numpy(), res.numpy()
    assert (h["material"] == -1).sum() > 100 and (h["material"] > 0).sum() > 100
    assert np.array_equal(used.cpu().numpy(), h["material"] != -1)
    check_none_records(got, h)
    sc = camera_scene(cam, dw, w)
    mats = cam._ensure_scene().device_tensors["materials"].cpu().numpy().reshape(-1, 8)[:, :7]
    sc = sr.with_materials(sc, mats)
    exp, stats, recs = sf.expect(sc, h, rays.cpu().numpy()[:, 3:6])
    sf.assert_records_equal(got, exp)
    assert np.array_equal(res.stats, stats)
    img = res.normal_image(frame).cpu().numpy()
    assert img.shape == (frame.height, frame.width, 3) and img.dtype == np.int8
    want = np.zeros(img.shape, np.int8)
    want[frame.pixels[:, 1], frame.pixels[:, 0]] = got["normal"][:: frame.samples]
    assert np.array_equal(img, want)
    # 0 exactly where the depth image has no hit -- or where the hit is enclosed, whose normal is (0, 0, 0) by definition
    first = got[:: frame.samples]
    enclosed = np.zeros(img.shape[:2], bool)
    enclosed[frame.pixels[:, 1], frame.pixels[:, 0]] = (first["status"] == 0) & (first["open"] == 0)
    no_hit = ~np.isfinite(frame.depth_image().cpu().numpy())
    assert np.array_equal(~img.any(2), no_hit | enclosed) and (np.abs(img).sum(2) <= 1).all()
    assert not (no_hit & enclosed).any() and (~no_hit & ~enclosed).sum() > 50
    return sc, int(stats[nat.S_SURFACE_ENCLOSED])


@gpu
def test_frame_and_normal_image():
    from python_raytracer_amd import make_settings
    from python_raytracer_amd.world import build_world
    from test_gpu_owners import golden, world_camera
    g = golden()
    st = make_settings(width=48, height=36, samples=4, lod_edge=0.5, dist_max=192, chunk_lod=0)
    st.culling = False
    cam = world_camera(st, g["ps"], g["z"]["cam_pos"])
    w = build_world(list(g["dw"].order), 16, owners=True)
    sc, _ = check_frame(cam, g["dw"], w)
    assert set(np.unique(sc.res[sc.present != 0]).tolist()) == {1}
    # ... and after a chunk_update that selects LODs: the pass follows the camera's current table
    cam.settings.chunk_lod = 2
    cam.chunk_update(None)
    sc, _ = check_frame(cam, g["dw"], w)
    assert len(set(np.unique(sc.res[sc.present != 0]).tolist())) >= 2


# ---- 4. bad input ------------------------------------------------------------------------------------------------------------
@gpu
def test_bad_records_get_their_status_and_leave_their_neighbours_alone():
    import torch
    c, cam = case_camera("sparse")
    h = c["hits"].copy()
    vels = c["vels"].copy()
    clean = cam.surfaces(upload(h), (c["origins"], vels)).numpy()
    good = np.flatnonzero(clean["status"] == 0)
    bad = {int(good[3 + 7 * i]): what for i, what in enumerate(("nan_pos", "inf_pos", "limit", "cell", "material", "rejected", "foreign",
                                                                   "nan_vel", "inf_vel"))}
    foreign = sf.case("res9")["hits"]
    foreign = foreign[(foreign["material"] > 0) & (np.abs(foreign["pos"]).max(1) > 40)][0]      # (outside this scene's box)
    for k, what in bad.items():
        if what == "nan_pos":
            h["pos"][k, 1] = np.nan
        elif what == "inf_pos":
            h["pos"][k, 2] = -np.inf
        elif what == "limit":
            h["pos"][k, 0], h["cell"][k, 0] = float(1 << 28), 1 << 28
        elif what == "cell":
            h["cell"][k, 2] += 1
        elif what == "material":
            h["material"][k] = 300
        elif what == "rejected":
            h[k] = np.zeros(1, cr.HIT_DTYPE)[0]
            h["material"][k] = nat.HIT_REJECTED
        elif what == "foreign":
            h[k] = foreign
        elif what == "nan_vel":
            vels[k, 0] = np.nan
        elif what == "inf_vel":
            vels[k, 2] = np.inf
    res = cam.surfaces(upload(h), (c["origins"], vels))
    got = res.numpy()
    exp, stats, recs = sf.expect(c["scene"], h, vels)
    status = {"rejected": nat.SURFACE_NONE, "foreign": nat.SURFACE_ORPHAN}
    for k, what in bad.items():
        assert int(got["status"][k]) == status.get(what, nat.SURFACE_INVALID) == int(exp["status"][k]), (k, what, got[k])
    sf.assert_records_equal(got, exp)
    assert np.array_equal(res.stats, stats)
    n_invalid = len(bad) - 2
    assert int(res.stats[nat.S_SURFACE_INVALID]) == n_invalid and int(res.stats[nat.S_SURFACE_ORPHANS]) == 1
    assert int(res.stats[nat.S_SURFACE_EXAMINED]) == len(good) - 1
    assert int(res.stats[nat.S_SURFACE_RESOLVED]) == len(good) - len(bad)
    keep = np.ones(len(h), bool)
    keep[list(bad)] = False
    assert got[keep].tobytes() == clean[keep].tobytes()
    check_none_records(got, h)
    # length mismatches are refused before any launch
    with pytest.raises(ValueError, match="hit records but"):
        cam.surfaces(upload(h), (c["origins"][:-1], vels[:-1]))
    with pytest.raises(ValueError, match="hit records but"):
        cam.surfaces(upload(h[:-1]), torch.zeros((len(h), 8), dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError, match="no whole number of 48-byte"):
        cam.surfaces(upload(h)[:100], (c["origins"], vels))


# ---- 5. n = 0, streams, graphs, continuation rays ----------------------------------------------------------------------------
@gpu
def test_empty_call_side_stream_and_graph():
    import torch
    c, cam = case_camera("lod")
    empty = cam.surfaces(torch.empty(0, dtype=torch.uint8, device="cuda"), torch.empty((0, 8), dtype=torch.float64, device="cuda"))
    assert empty.records.numel() == 0 and not empty.stats.any()
    hits = cam.cast_rays(c["origins"], c["vels"], c["lives"], max_life=MAX_LIFE)
    rays = torch.zeros((len(c["vels"]), 8), dtype=torch.float64, device="cuda")
    rays[:, 3:6] = torch.from_numpy(c["vels"].copy()).cuda()
    exp = cam.surfaces(hits, rays)
    exp_records, exp_stats = exp.numpy(), exp.stats.copy()
    assert int(exp_stats[nat.S_SURFACE_RESOLVED]) >= 100
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    on_side = cam.surfaces(hits, rays, stream=side)               # (also the warm-up on the capturing side: the allocator)
    torch.cuda.current_stream().wait_stream(side)
    assert on_side.numpy().tobytes() == exp_records.tobytes() and np.array_equal(on_side.stats, exp_stats)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        res = cam.surfaces(hits, rays)
    res.records.zero_()
    res._stats_dev.fill_(-1)
    graph.replay()
    torch.cuda.synchronize()
    assert res.numpy().tobytes() == exp_records.tobytes()
    assert np.array_equal(res._stats_dev.cpu().numpy(), exp_stats)


@gpu
def test_continuation_rays_and_path_rows():
    import torch
    c, cam = case_camera("sparse")
    hits = cam.cast_rays(c["origins"], c["vels"], c["lives"], max_life=MAX_LIFE)
    res = cam.surfaces(hits, (c["origins"], c["vels"]))
    got = res.numpy()
    rays = res.rays(24.0)
    assert rays.shape == (len(got), 8) and rays.dtype == torch.float64 and rays.data_ptr() % 64 == 0
    r = rays.cpu().numpy()
    ok = got["status"] == 0
    assert np.isnan(r[~ok]).all() and ok.sum() >= 100 and (~ok).sum() >= 10
    assert np.array_equal(r[ok, 0:3].view(np.uint64), got["next"][ok].view(np.uint64))      # copied, never computed with
    assert np.array_equal(r[ok, 3:6].view(np.uint64), got["vel"][ok].view(np.uint64))
    assert (r[ok, 6] == 24.0).all() and (r[ok, 7] == 0.0).all()
    lives = np.linspace(1.0, 30.0, len(got))
    assert np.array_equal(res.rays(lives).cpu().numpy()[ok, 6], lives[ok])
    with pytest.raises(ValueError, match="lives for"):
        res.rays(lives[:-1])
    # cast_rays takes the array as it is, rejects the NaN records and marches the others from `next` along `vel`
    onward = cam.cast_rays(rays, max_life=MAX_LIFE)
    assert np.array_equal(onward.rejected_mask().cpu().numpy(), ~ok)
    radius = round(c["scene"].chunk_size / 2)
    exp = cr.march_records(c["scene"], radius, got["next"][ok], got["vel"][ok], np.full(int(ok.sum()), 24.0))
    cr.assert_records_equal(onward.numpy()[ok], exp)
    # row 0 of path_rays is the first hit: the same surfaces (a ray that hits nothing has material -1 there, 0 here: no surface)
    path = cam.path_rays(c["origins"], c["vels"], c["lives"], max_hits=4, max_life=MAX_LIFE)
    assert (path.counts.cpu().numpy() >= 0).all()
    again = cam.surfaces(path.hit(0), (c["origins"], c["vels"]))
    assert again.numpy().tobytes() == got.tobytes()
