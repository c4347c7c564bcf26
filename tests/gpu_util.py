"""Helpers shared by the GPU parity tests, smoke() and bench.py: build a python_raytracer_amd.Camera from the
dense fixture scenes and from oracle-style settings dicts."""
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
