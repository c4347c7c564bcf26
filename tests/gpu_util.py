"""Helpers shared by the GPU parity tests, smoke() and bench.py: build a python_raytracer_amd.Camera from the
dense fixture scenes and from oracle-style settings dicts; the frame-march check the GPU test modules share."""
import os

import numpy as np

from python_raytracer_amd import Camera, PackedScene
from python_raytracer_amd.data import finalize_settings
from python_raytracer_amd.lib import store, vec3, quaternion


def settings_store(d):
    """oracle_lib.make_settings() dict -> python_raytracer_amd settings store (with the pixel partition)."""
    s = store(**{k: v for k, v in d.items() if k not in ("proportions", "chunk_radius")})
    if not hasattr(s, "culling"):
        s.culling = False
    return finalize_settings(s)


def camera_for(scene, settings, pos, rot, lens, grid=None, device=None):
    """Camera over a dense oracle_lib.Scene.  grid defaults to the scene's camera grid."""
    cam = Camera(settings=settings, device=device)
    cam.pos = vec3(*[float(v) for v in pos])
    cam.rot = quaternion(*[float(v) for v in rot])
    cam.lens = float(lens)
    g = scene.grid if grid is None else grid
    cam.set_packed_scene(PackedScene.from_dense(scene.origin, scene.dims, scene.chunk_size, scene.present, scene.res,
                                                g, scene.materials))
    return cam


def bitmap_window(cam_pos, chunk_size, trav_origin, trav_dims):
    """Where vrt_render_tile puts the 32^3-cell settled-bitmap window of a traversed box that gets no bitmap of its own
    (include/vrt.h, vrt_traversed; VRT_TRAV_WINDOW): the window's lowest cell per axis, as an index into the box -- centred
    on the camera's cell, pushed back inside the box -- or None for a box that cannot have one (a side below 32 cells or
    of 1024 + 32 and more)."""
    import math
    if any(d < 32 or d >= 1024 + 32 for d in trav_dims):
        return None
    return [min(max(int(math.floor(p / chunk_size)) - int(o) // chunk_size - 16, 0), int(d) - 32)
            for p, o, d in zip(cam_pos, trav_origin, trav_dims)]


def window_split(traversed, chunk_size, trav_origin, window):
    """Boolean mask over a traversed list ([n, 3] chunk positions): which of the chunks lie inside the bitmap window."""
    import numpy as np
    cells = (np.asarray(traversed, np.int64).reshape(-1, 3) - np.asarray(trav_origin, np.int64)) // chunk_size
    lo = np.asarray(window, np.int64)
    return ((cells >= lo) & (cells < lo + 32)).all(1)


def sparse_scene(seed, res_max, chunk_size=8, dims=(6, 6, 6), fill=0.02):
    """A small sparse world of `dims` chunks centred on the origin (some chunks missing, resolutions 1..res_max, four
    materials): most rays leave it and cross empty chunk cells until dist_max ends them, so a frame visits traversed cells
    far from the camera as well as near it."""
    import numpy as np
    import oracle_lib as ol
    rng = np.random.default_rng(seed)
    dims = np.array(dims)
    cs = int(chunk_size)
    origin = np.array([-(d // 2) * cs for d in dims], np.int64)
    present = (rng.random(tuple(dims)) < 0.85).astype(np.uint8)
    res = rng.integers(1, res_max + 1, tuple(dims)).astype(np.uint8)
    mats = np.array([[200, 40, 40, 0.0, 0.5, 0.0, 0.0], [40, 200, 40, 0.5, 1.0, 0.75, 0.0], [40, 40, 200, 0.1, 0.25, 0.25, 0.5],
                     [220, 220, 220, 1.0, 2.0, 1.0, 0.0]])
    grid = np.where(rng.random(tuple(dims * cs)) < fill, rng.integers(1, 5, tuple(dims * cs)), 0).astype(np.uint8)
    return ol.Scene(origin, dims, cs, present, res, ol.Scene.camera_grid(grid, origin, dims, cs, present, res), mats)


# LDS of a frame-march workgroup (tests/test_gpu_lds_room.py).  A CU has 160 KiB and the march kernels
# are built for VRT_WAVES_PER_SIMD = 4 workgroups of 256 threads on it.  Static LDS per kernel from the compiler's resource
# report of the shipped source, by whether the instance looks ahead across chunk borders (W: its per-axis offset tables are
# part of the world-axis tables in dynamic LDS); tests/test_kernel_resources.py pins both on the CPU.
BUDGET_LDS = 160 * 1024 // 4
STATIC_LDS = {False: 8032, True: 4976}
POOL_LDS = 4 * 18 * 8 * 48      # 4 waves x 18 words x 8 bytes x 48 parked rays


def march_dyn_lds(n_materials, ct_cells, bitmap_words, wt_cells, pool):
    """Dynamic LDS bytes of a frame-march launch, restated from the documented sizes: 64 bytes per material, 4 per chunk-table
    cell kept in LDS, 4 per word of the settled bitmap, rounded up to 16; then (cells + 64) * 4 bytes per world-table axis
    (wt_cells: the world's cells per axis, or None without the look-ahead); then the ray pools; then 16 bytes."""
    n = 64 * n_materials + 4 * ct_cells + 4 * bitmap_words
    n = (n + 15) // 16 * 16
    if wt_cells is not None:
        n += sum((int(c) + 64) * 4 for c in wt_cells)
    return n + (POOL_LDS if pool else 0) + 16


def frame_equals_oracle(r, o, cs):
    """A frame rendered with want_ray_rgba against the oracle's (oracle_lib.render with its rays): fp32 means, event counters,
    the traversed list in the reference's order and every sample's packed colour."""
    assert np.array_equal(r.rgba_f32.cpu().numpy(), o["pix_mean"].astype(np.float32))
    assert (r.stats[:8] == o["counters"]).all(), (r.stats[:8], o["counters"])
    assert np.array_equal(np.array(r.traversed(cs), np.int64).reshape(-1, 3), np.asarray(o["traversed"]).reshape(-1, 3))
    rays = o["rays"]
    where = {(int(x), int(y)): i for i, (x, y) in enumerate(r.pixels)}
    slot = np.array([where[(int(x), int(y))] for x, y in zip(rays["x"], rays["y"])], np.int64) * r.max_samples + rays["s"]
    packed = (rays["color"][:, 0].astype(np.uint32) | (rays["color"][:, 1].astype(np.uint32) << 8) |
              (rays["color"][:, 2].astype(np.uint32) << 16) | (rays["alpha"].astype(np.uint32) << 24))
    got = r.ray_rgba.cpu().numpy().view(np.uint32)
    assert np.array_equal(got[slot], packed)


def launches_of(call):
    """(call(), the kernel instances it launched): the names, with every template argument, whose count in the library's
    launch census (_native.launch_census: host-side counters next to the launches) rose across the call."""
    from python_raytracer_amd import _native as nat
    before = nat.launch_census()
    out = call()
    after = nat.launch_census()
    return out, {name for name in after if after[name] > before[name]}


def check_frame_march(cam, o, cs, which, lookahead=None, window=None, expect_pool=None, **kw):
    """The same frame WITHOUT ray records: `want_rays` selects the recording march_kernel whatever VRT_POOL says, so this is
    the render that runs the frame kernel the fixture names -- march_pool_kernel under "pool" (asserted: its workgroups
    count themselves in stats[12]), march_kernel under "lanes".  Per-sample colours, fp32 means, event counters and the
    traversed list against the oracle.
    window: what the VRT_TRAV_WINDOW=2 leg below must have been able to do -- True: the traversed box is one that gets the
    32^3-cell bitmap window (every side of 32 cells and more) AND the oracle's list has chunks both inside that window
    (the settled bit) and outside it (the key read at every visit); False: the box is too small for a window.  The result
    says which it was (`window`: the window's lowest cell, or None).
    expect_pool: for scenes whose materials and tables leave the ray pools no room in LDS (tests/test_gpu_lds_room.py) -- False:
    march_kernel runs although the leg asks for the pool; None: the leg's own rule."""
    r = cam.render(0, want_ray_rgba=True, **kw)
    groups = int(r.stats[12]) & 0xffffffff     # (bits 32+: the workgroups that took their rays as tiles)
    if expect_pool is None:
        expect_pool = which.startswith("pool")
    assert not expect_pool or which.startswith("pool"), (which, expect_pool)
    assert (groups > 0) if expect_pool else (groups == 0), (which, groups)
    if lookahead is not None:   # did the march step look ahead across chunk borders (march_step_w)?
        assert (int(r.stats[14]) > 0) == bool(lookahead), (lookahead, int(r.stats[14]))
    frame_equals_oracle(r, o, cs)
    # ... and once more without the settled-cell bitmap (VRT_TRAV_LDS=0, read at every launch): what traversed boxes too large
    # for one get -- every visit reads its cell's key, and the kernel instances that compare it after the voxel reads run
    # -- and, where the window's geometry allows (the pool kernel, a power-of-two run of pixels per hand-out that divides the
    # height), with the rays handed out as square tiles in Morton order from eight heads (VRT_TILED=2: tile_ticket)
    os.environ["VRT_TRAV_LDS"], os.environ["VRT_DEFER_VISIT"], os.environ["VRT_TILED"] = "0", "2", "2"   # (2: also over scenes that fit the caches)
    try:
        r2 = cam.render(0, want_ray_rgba=True, **kw)
    finally:
        del os.environ["VRT_TRAV_LDS"], os.environ["VRT_DEFER_VISIT"], os.environ["VRT_TILED"]
    assert np.array_equal(r2.ray_rgba.cpu().numpy(), r.ray_rgba.cpu().numpy()) and (r2.stats[:9] == r.stats[:9]).all()
    assert np.array_equal(r2.traversed_keys.cpu().numpy(), r.traversed_keys.cpu().numpy())
    # ... with the settled bitmap of boxes too large for one of their own: over the 32^3 cells around the camera only
    # (VRT_TRAV_WINDOW=2 uses it for every box of at least 32^3 cells; smaller boxes render as before)
    # -- together with the key comparison behind the voxel reads, as scenes beyond the caches run it
    os.environ["VRT_TRAV_WINDOW"], os.environ["VRT_DEFER_VISIT"] = "2", "2"
    try:
        r4 = cam.render(0, want_ray_rgba=True, **kw)
    finally:
        del os.environ["VRT_TRAV_WINDOW"], os.environ["VRT_DEFER_VISIT"]
    assert np.array_equal(r4.ray_rgba.cpu().numpy(), r.ray_rgba.cpu().numpy()) and (r4.stats[:9] == r.stats[:9]).all()
    assert np.array_equal(r4.traversed_keys.cpu().numpy(), r.traversed_keys.cpu().numpy())
    # (could that leg use the window at all?  From the box it was handed, not from anything the library reports)
    assert r4.trav_origin == r.trav_origin and r4.trav_dims == r.trav_dims
    r.window = bitmap_window([float(cam.pos.x), float(cam.pos.y), float(cam.pos.z)], cs, r4.trav_origin, r4.trav_dims)
    if window is not None:
        assert (r.window is not None) == bool(window), (r4.trav_dims, r.window)
    if window:
        inside = window_split(o["traversed"], cs, r4.trav_origin, r.window)
        assert inside.any() and (~inside).any(), (int(inside.sum()), int((~inside).sum()))
    # ... and once without the cached ray table (Camera.cache_draws = False): the frame's draws are seeded anew and the march
    # works out every ray's lens quaternion and life itself instead of reading raygen_tile_kernel's records -- asserted where
    # the library has such a march (stats[15]: not for resolutions > 2, the look-ahead variant or one record per pixel)
    s = cam._settings()
    fused = (not which.endswith("-ahead") and 1 <= int(cam._c_scene(cam._ensure_scene()).max_resolution) <= 2 and
             (float(s.dof) != 0.0 or float(s.lod_random) != 0.0 or float(s.lod_samples) != 0.0))
    cached, cam.cache_draws = cam.cache_draws, False
    try:
        r3 = cam.render(0, want_ray_rgba=True, **kw)
    finally:
        cam.cache_draws = cached
    if fused:
        assert int(r3.stats[15]) > 0, r3.stats
    assert np.array_equal(r3.ray_rgba.cpu().numpy(), r.ray_rgba.cpu().numpy()) and (r3.stats[:9] == r.stats[:9]).all()
    assert np.array_equal(r3.traversed_keys.cpu().numpy(), r.traversed_keys.cpu().numpy())
    return r


def active(r):
    rays = r.rays
    return rays[rays["s"] >= 0]


def check_tile_plan(dp, st):
    """A built tile plan (DevicePixels.plan: the static distinct-seed index of include/vrt.h, vrt_plan_build) against a
    numpy restatement, for every pixel and sample slot of the list: the header's counts, the sorted distinct seeds and
    the seed index of every slot (0xFFFFFFFF for a slot the pixel's sample count leaves unused).  st: the oracle-style
    settings dict the plan was built for.  Returns the header words."""
    import ctypes as C
    import oracle_lib as ol
    px = dp.array.astype(np.int64)
    ost = ol._orc_settings(st)
    L = ol.lib()
    ns = np.array([L.orc_pixel_samples(C.byref(ost), int(x), int(y)) for x, y in px], np.int64).reshape(-1)
    raw = dp.plan.cpu().numpy()
    hdr = raw[:64].view(np.uint64)
    smax = max(1, round(st["samples"] * (1 - min(st["lod_edge"], 0.0))))           # vrt_max_samples (init.py:133-134)
    assert ns.max(initial=1) <= smax
    used = np.arange(smax)[None, :] < ns[:, None]                                   # [n_px, smax]: the slots that hold a ray
    seeds = ((1 + px[:, 0]) * (1 + px[:, 1]))[:, None] * (1 + np.arange(smax))[None, :]
    distinct = np.unique(seeds[used])
    assert dp.n_distinct == len(distinct)
    slots = len(px) * smax
    assert hdr[1] == len(px) and hdr[2] == slots and hdr[3] == len(distinct)
    seed_list = raw[64:64 + 4 * slots].view(np.uint32)[: len(distinct)]
    assert np.array_equal(seed_list.astype(np.int64), distinct)                    # sorted, unique
    off = 64 + ((4 * slots + 255) // 256) * 256
    idx = raw[off:off + 4 * slots].view(np.uint32).reshape(len(px), smax)
    assert (idx[~used] == 0xFFFFFFFF).all()
    assert (idx[used] < len(distinct)).all()
    assert np.array_equal(seed_list[idx[used]].astype(np.int64), seeds[used])
    return hdr


# the hand-out's operating points besides the shipped one: the static range per wave, with the usual and an odd small grid;
# small chunks over an odd grid; one workgroup that takes every chunk
HANDOUT_KNOBS = [{}, {"VRT_CHUNK": "0"}, {"VRT_CHUNK": "0", "VRT_MARCH_GRID": "3"}, {"VRT_CHUNK": "64", "VRT_MARCH_GRID": "7"},
                 {"VRT_MARCH_GRID": "1"}]


def run_children(call, knob_sets, tag):
    """`call` (python source) in one child process per set of scheduling knobs -- they are read once per process --, all at
    once; returns each child's line that begins with `tag`, split into words."""
    import os
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))   # (tests/: the children import the test modules)
    base = {k: v for k, v in os.environ.items() if k not in ("VRT_CHUNK", "VRT_MARCH_GRID")}
    procs = [subprocess.Popen([sys.executable, "-c", call], cwd=here, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                              env=dict(base, PYTHONPATH=os.pathsep.join([here, os.path.dirname(here)]), **knobs))
             for knobs in knob_sets]
    lines = []
    try:
        for knobs, proc in zip(knob_sets, procs):
            out = proc.communicate(timeout=120)[0]
            assert proc.returncode == 0, (knobs, out)
            lines.append([l for l in out.splitlines() if l.startswith(tag)][0].split())
    finally:   # (a failure leaves no child behind on the GPU)
        for proc in procs:
            if proc.poll() is None:
                proc.kill()
            proc.wait()
    return lines
