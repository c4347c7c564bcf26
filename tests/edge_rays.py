"""Explicit-ray sets over the edge scenes of tests/edge_scenes.py: what holds first_hit_kernel's siblings -- cast_kernel,
shade_kernel, path_kernel -- to the oracle where the frame kernels already are (chunk sizes 8, 32 and 64, resolutions up to
9, worlds 2^26 to 2^27 cells out, origins beside the +-2^28 limit, max_bounces 0.5 and 16, falloff 0 and 3, 19 materials,
dense and sparse grids, no background).  Plain definitions: no pytest marks, nothing of the GPU is imported.

One set per case of EDGE_CASES plus "no_background", made by shade_ref.oracle_shade: one oracle call per ray (LIBM_PORTABLE),
nonce 1000 + k, the case's own falloff, shutter, lod_bounces, max_light, max_bounces and dist_min passed through, the row of
draws as wide as the oracle's largest draw counter of the set.  The settings of a set are the case's own settings dict, which
is also what the GPU camera of tests/test_gpu_edge_rays.py gets.  tests/test_edge_rays_host.py asserts on the CPU what the GPU
comparison relies on: that path_ref.trace_paths gives the oracle's records, that the range rule rejects no ray, and that every
set reaches the edge it is named after."""
import numpy as np

import cast_ref as cr
import path_ref as pr
import shade_ref as sr
from edge_scenes import EDGE_CASES, edge_scene

ALL_CASES = list(EDGE_CASES) + ["no_background"]
SMALL = ("w1", "h1", "one_pixel")          # the window plays no part in an explicit ray: these three repeat the default box
N_RAYS, N_SMALL = 600, 64
SCALED = ("far_mixed", "fov179")           # quaternions of norm 0.5 .. 1.5: |vel| varies
LIMIT_CASES = ("limit_28_pos", "limit_28_neg")
EXTRA = ("falloff", "shutter", "lod_bounces")
GROW = 4.0
_sets, _paths = {}, {}


def n_rays(name):
    return N_SMALL if name in SMALL else N_RAYS


def far_axes(name):
    """The axes a far case displaces by 2^20 chunks (less one) and more: every origin of its set lies at 2^20 chunk sizes and
    beyond on them."""
    sc = edge_scene(name)[0]
    return [a for a in range(3) if abs(int(sc.origin[a])) >= ((1 << 20) - 1) * sc.chunk_size]


def filled_cells(sc):
    """World coordinates [m, 3] of the voxels a lookup can find: non-zero cells of the camera grid in present chunks."""
    cells = np.argwhere(sc.grid != 0)
    chunk = cells // sc.chunk_size
    keep = sc.present[chunk[:, 0], chunk[:, 1], chunk[:, 2]] != 0
    return cells[keep] + sc.origin, sc.res[chunk[keep, 0], chunk[keep, 1], chunk[keep, 2]].astype(np.int64)


def edge_ray_set(name):
    """(scene, settings, has_background, origins, vels, lives, draws, expected records, traversed lists) of a case: the
    tuple of shade_ref.ray_set.  600 rays (64 for w1, h1 and one_pixel), deterministic, built once, never changed.

    The oracle's camera positions are uniform over the scene's chunk box grown by 4 cells (the ray's origin is that position
    moved by vel * dist_min, which is 0 everywhere but in near4); unit quaternions from cast_ref.unit_quats, scaled to norms
    0.5 .. 1.5 for far_mixed and fov179; lives uniform in [span / 12, span] with span = dist_max - dist_min.  Four kinds of set
    are made otherwise:
      far_pos, far_mixed   the box starts one chunk (far_pos) or 4 cells (far_mixed) below 2^20 chunk sizes on the displaced
                           axes: positions are uniform over the part of the grown box at 2^20 chunk sizes and beyond there,
                           so that every origin has the magnitude the case is named after (the rays still cross the rest).
      limit_28_pos / _neg  positions within 8 cells of the case's camera, never farther from 0 than it on any axis.
      near4                dist 3 .. 4: a ray looks up the one cell of its origin, so 5 % of uniform rays hit.  Every second
                           ray's origin is put inside a voxel a lookup finds (a cell of the camera grid in a present chunk,
                           0.1 .. 0.9 of the chunk's resolution into it); its position is that point less vel * dist_min.
      fill_sparse          0.5 % fill: 5 % of uniform rays hit.  Every second ray starts 1 .. 8 whole velocities in front of
                           such a point, so that its unit steps land on it where no coarser chunk or hole lies between."""
    if name in _sets:
        return _sets[name]
    sc, st, cams, lens = edge_scene(name)
    has_bg = name != "no_background"
    n = n_rays(name)
    rng = np.random.default_rng(5000 + (121 if name == "no_background" else EDGE_CASES[name]["seed"]))
    cs = sc.chunk_size
    lo = np.asarray(sc.origin, np.float64) - GROW
    hi = np.asarray(sc.origin + sc.dims * cs, np.float64) + GROW
    if name in ("far_pos", "far_mixed"):
        for a in far_axes(name):
            lo[a] = max(lo[a], float((1 << 20) * cs))
        assert (lo < hi).all()
    q = cr.unit_quats(rng, n)
    if name in SCALED:
        q = q * rng.uniform(0.5, 1.5, (n, 1))
    span = float(st["dist_max"]) - float(st["dist_min"])
    lives = rng.uniform(span / 12, span, n)
    if name in LIMIT_CASES:
        cam = np.asarray(cams[0][0], np.float64)
        pos = cam - np.sign(cam) * rng.uniform(0, 8, (n, 3))
        assert (np.abs(pos) <= np.abs(cam)).all()
    else:
        pos = rng.uniform(lo, hi, (n, 3))
    if name in ("near4", "fill_sparse"):
        cells, res = filled_cells(sc)
        pick = rng.integers(0, len(cells), n)
        point = cells[pick] + rng.uniform(0.1, 0.9, (n, 3)) * res[pick][:, None]
        vel = cr.vec_forward(q)
        back = float(st["dist_min"]) if name == "near4" else rng.integers(1, 9, n)[:, None].astype(np.float64)
        aimed = np.arange(n) % 2 == 0
        pos[aimed] = (point - vel * back)[aimed]
    origins, vels, lives, draws, exp, trav = sr.oracle_shade(
        sc, pos, q, lives, 1000 + np.arange(n), st["max_bounces"], has_bg, max_light=st["max_light"], dist_min=st["dist_min"],
        n_draws=None, **{k: st[k] for k in EXTRA})
    assert draws.shape[1] == max(1, int(exp["counters"][:, sr.C_DRAW].max()))
    for a in (origins, vels, lives, draws, exp):
        a.setflags(write=False)
    _sets[name] = (sc, st, has_bg, origins, vels, lives, draws, exp, trav)
    return _sets[name]


def edge_path_set(name):
    """(records, counts, paths) of path_ref.trace_paths over edge_ray_set(name), with the set's full draw rows."""
    if name not in _paths:
        sc, st, has_bg, origins, vels, lives, draws, exp, trav = edge_ray_set(name)
        rec, counts, paths = pr.trace_paths(sc, st, origins, vels, lives, draws, has_bg)
        rec.setflags(write=False)
        counts.setflags(write=False)
        _paths[name] = (rec, counts, paths)
    return _paths[name]


def rejected(sc, origins, vels, lives):
    """The documented range rule of the explicit-ray calls (Camera.cast_rays), in numpy: true where a ray is NOT accepted --
    |origin| + (max(life, 0) + 2 chunk_size + 2) max(1, |vel|_inf) >= 2^28 on an axis, or |vel| > 2^25, or a value that is
    not finite."""
    vmax = np.abs(vels).max(1)
    reach = (np.maximum(lives, 0) + 2.0 * sc.chunk_size + 2.0) * np.maximum(1.0, vmax)
    bad = (np.abs(origins) + reach[:, None] >= float(1 << 28)).any(1) | (vmax > float(1 << 25))
    return bad | ~np.isfinite(origins).all(1) | ~np.isfinite(vels).all(1) | ~np.isfinite(lives)


def record_resolutions(sc, paths):
    """Per ray, the set of chunk resolutions its path records lie in (a record's cell names its chunk)."""
    out = []
    for path in paths:
        seen = set()
        for step, pos, cell, mat in path:
            c = tuple((np.array(cell, np.int64) - sc.origin) // sc.chunk_size)
            seen.add(int(sc.res[c]))
        out.append(seen)
    return out


def record_materials(paths):
    return {mat for path in paths for step, pos, cell, mat in path}
