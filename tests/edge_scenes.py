"""The small fixed scenes at the edges of the input ranges, shared by the GPU tests that render them against the oracle
(tests/test_gpu_edges.py, tests/test_gpu_parity.py), by the generator that renders them through the real reference
(tests/golden/make_golden_edges.py) and by the tests that read its fixtures (tests/test_oracle_edges_golden.py,
tests/test_gpu_reference_edges.py).  Plain definitions: no pytest marks, nothing of the GPU is imported.

EDGE_CASES sets one input at the edge of its range per scene with the rest kept moderate, so that a failure names its
cause; edge_proof() asserts, from a frame's rays alone, that a scene reached the edge it is named after.  The boundary
scene puts an unrotated camera on chunk corners, faces, the origin and one ulp beside them."""
import hashlib

import numpy as np

import oracle_lib as ol

CNT = {name: i for i, name in enumerate(ol.COUNTERS)}
IDENTITY = (0.0, 0.0, 0.0, 1.0)

# materials: r, g, b, roughness, absorption, ior, energy
MATS4 = np.array([[200, 40, 40, 0.0, 0.5, 0.0, 0.0], [40, 200, 40, 0.5, 1.0, 0.75, 0.0], [40, 40, 200, 0.1, 0.25, 0.25, 0.5],
                  [220, 220, 220, 1.0, 2.0, 1.0, 0.0]])
# weakly absorbing rough materials (0.05: many hits per ray) beside stronger ones that let `bounces` reach its cap
MATS_BOUNCY = np.array([[200, 180, 160, 1.0, 0.05, 1.0, 0.0], [90, 120, 250, 0.5, 0.05, 0.5, 0.0], [60, 200, 90, 0.1, 0.5, 0.75, 0.0],
                        [230, 230, 230, 0.0, 2.0, 1.0, 0.0]])


def mats19():
    """19 materials over the soak's widest property values: roughness up to 2.5, absorption 0.05 and 7."""
    rng = np.random.default_rng(1900)
    m = np.zeros((19, 7))
    m[:, :3] = rng.integers(0, 256, (19, 3))
    m[:, 3] = np.resize([0.0, 0.1, 0.5, 1.0, 2.5], 19)
    m[:, 4] = np.resize([0.05, 7.0, 0.25, 1.0, 7.0, 0.05, 2.0], 19)
    m[:, 5] = np.resize([0.0, 0.25, 0.5, 0.75, 1.0, 0.0], 19)
    m[:, 6] = np.resize([0.0, 0.0, 0.5, 2.0], 19)
    return m


LIMIT = float(1 << 28)   # vrt_render_tile: |pos| + reach < 2^28 on every axis

# Every case sets one input at its edge; what is not named keeps EDGE_DEFAULTS (a 3 x 2 x 3-chunk box of 16-cell chunks at
# resolutions 1..2, fill 0.1, a rotated camera inside the box, a 40 x 30 image of 2 samples, dist_max 200).
#   origin: in chunks.  at: the camera's place in the box, as a fraction of its extent.  st: settings that differ.
#   cameras: "rotated" (a random unit quaternion, fractional position) | "integer" (unrotated, position rounded: every
#   primary ray of the centre row / column stays on voxel boundaries).
# The comment of each case is what the oracle alone gives for it (hits = hit events of the frame, of its first camera).
EDGE_DEFAULTS = dict(cs=16, dims=(3, 2, 3), origin=(-1, -1, -2), fill=0.1, res=(1, 2), mats=MATS4, at=(0.45, 0.55, 0.4),
                     cameras=("rotated",), fov=90.0, pocket=0, limit=0, st={})
EDGE_CASES = {
    # camera beside a chunk corner: 2400 rays, 2148 hits, chunk_get 86
    "cs64": dict(seed=101, cs=64, dims=(2, 3, 2), origin=(-1, -2, -1), at=(0.49, 0.34, 0.49)),
    # rotated: 5219 hits, smallest traversed coordinate 67108672 (> 2^25 = 33554432); integer camera: 5809 hits
    "far_pos": dict(seed=102, cs=64, dims=(2, 2, 3), origin=((1 << 20) - 1,) * 3, cameras=("rotated", "integer")),
    # rotated: 3699 hits, largest traversed coordinate -134217536 (< -2^26 = -67108864); integer camera: 4351 hits
    "far_neg": dict(seed=103, cs=64, dims=(2, 2, 3), origin=(-(1 << 21),) * 3, cameras=("rotated", "integer")),
    # rotated: 3025 hits; integer camera: 3877 hits
    "far_mixed": dict(seed=104, cs=8, dims=(3, 3, 3), origin=(-50000, 1000, 1 << 20), cameras=("rotated", "integer")),
    # camera at +-268433349.5 on every axis (reach 2106): 2592 / 4486 hits, 1421 / 1239 rays that ended by distance
    "limit_28_pos": dict(seed=105, limit=+1, dims=(2, 2, 2), st=dict(dist_min=0)),
    "limit_28_neg": dict(seed=106, limit=-1, dims=(2, 2, 2), st=dict(dist_min=0)),
    # resolutions 1..9 (5, 7 and 9 forced into three chunks): 2060 hits, 575 rays that broke in a chunk of resolution >= 5,
    # 11017 re-snaps
    "res9": dict(seed=107, cs=32, res=(1, 9), at=(0.5, 0.5, 0.35)),
    # 48 x 12 image (proportions 0.625): 108 of 576 pixels with a half-angle of pi / 4 and more; 2103 hits
    "fov179": dict(seed=108, fov=179.0, st=dict(width=48, height=12)),
    # 4559 hits
    "fov20": dict(seed=109, fov=20.0),
    # cap 1.5: 1640 of 2400 rays reach it
    "bounces_half": dict(seed=110, mats=MATS_BOUNCY, fill=0.3, st=dict(max_bounces=0.5, max_light=100.0)),
    # cap 17: 402 of 2400 rays reach it; largest draw count 393, 1566 rays with more than 32 draws
    "bounces16": dict(seed=111, mats=MATS_BOUNCY, fill=0.3, res=(1, 1),
                      st=dict(max_bounces=16.0, max_light=100.0, lod_bounces=0.0, falloff=0.0)),
    # 48 x 36 x 9: 1728 pixels, 1363 of them with fewer than 9 samples; 11689 rays, 2356 with a life below 1 (1043 of exactly 0)
    "lod_full": dict(seed=112, st=dict(width=48, height=36, samples=9, lod_edge=1.0, lod_random=1.0, lod_samples=3.0)),
    # 3123 hits
    "dof10": dict(seed=113, st=dict(dof=10.0, max_bounces=4.0)),
    # life <= detail for all 2400 rays; 424 hits
    "near4": dict(seed=114, st=dict(dist_max=4, dist_min=3)),
    # 3026 hits; the rays that ended in a hit did so on all 19 materials
    "rough25_abs7": dict(seed=115, mats=mats19(), fill=0.2, st=dict(falloff=3.0, max_light=0.1)),
    # 223 hits, 114328 advances
    "fill_sparse": dict(seed=116, fill=0.005),
    # every one of the 2400 rays hits (5070 hits)
    "fill_dense": dict(seed=117, fill=0.9, pocket=3),
    # 72 / 96 / 7 rays (109 / 132 / 7 hits)
    "w1": dict(seed=218, st=dict(width=1, height=36)),
    "h1": dict(seed=119, st=dict(width=48, height=1)),
    "one_pixel": dict(seed=120, st=dict(width=1, height=1, samples=9)),
}
# The EDGE_DEFAULTS scene under a seed of its own, rendered with data.background = None (has_background = 0): the rays that
# end without a hit keep their un-energised colour.  Not in EDGE_CASES: the tests over those render with the background.
NO_BACKGROUND = dict(seed=121)

_scenes = {}


def limit_camera(sign, st):
    """The largest integer-plus-0.5 coordinate that vrt_render_tile's range check accepts for an unrotated camera:
    reach = (|dist_max| + |dist_min| + 2 chunk_size + 2) * (8 |rot|^2 + 1), and |pos| + reach < 2^28 on every axis."""
    reach = (abs(st["dist_max"]) + abs(st["dist_min"]) + 2.0 * st["chunk_size"] + 2.0) * (8 * 1.0 + 1)
    p = LIMIT - reach - 0.5
    assert p == np.floor(p) + 0.5 and p + reach < LIMIT and not (p + 1 + reach < LIMIT)
    return sign * p, reach


def edge_scene(name):
    """(scene, settings, [(camera position, rotation)], lens) of a case of EDGE_CASES (or "no_background");
    deterministic, built once."""
    if name in _scenes:
        return _scenes[name]
    c = dict(EDGE_DEFAULTS)
    c.update(NO_BACKGROUND if name == "no_background" else EDGE_CASES[name])
    rng = np.random.default_rng(c["seed"])
    cs, dims = int(c["cs"]), np.array(c["dims"])
    st = ol.make_settings(**dict(dict(width=40, height=30, samples=2, max_bounces=4.0, chunk_size=cs, dist_max=200, fov=c["fov"]),
                                 **c["st"]))
    origin = np.array(c["origin"], np.int64) * cs
    pos = np.floor(origin + np.array(c["at"]) * dims * cs) + np.array([0.3, 0.6, 0.45])
    if c["limit"]:
        # a two-chunk box round the camera; an unrotated camera looks along +z, so the box starts with the camera's chunk there
        p, _ = limit_camera(c["limit"], st)
        pos = np.array([p, p, p])
        origin = (np.floor(pos / cs).astype(np.int64) - np.array([1, 1, 0])) * cs
    present = (rng.random(tuple(dims)) < 0.85).astype(np.uint8)
    present[tuple(((np.floor(pos) - origin) // cs).astype(np.int64))] = 1
    res = rng.integers(c["res"][0], c["res"][1] + 1, tuple(dims)).astype(np.uint8)
    if c["res"][1] == 9:
        res.reshape(-1)[[4, 7, 10]] = [5, 7, 9]
        present.reshape(-1)[[4, 7, 10]] = 1
    mats = np.asarray(c["mats"], np.float64)
    shape = tuple(dims * cs)
    grid = np.where(rng.random(shape) < c["fill"], rng.integers(1, len(mats) + 1, shape), 0).astype(np.uint8)
    if c["pocket"]:
        lo = (np.floor(pos) - origin).astype(np.int64) - c["pocket"]
        grid[lo[0]:lo[0] + 2 * c["pocket"] + 1, lo[1]:lo[1] + 2 * c["pocket"] + 1, lo[2]:lo[2] + 2 * c["pocket"] + 1] = 0
    sc = ol.Scene(origin, dims, cs, present, res, ol.Scene.camera_grid(grid, origin, dims, cs, present, res), mats)
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    cams = []
    for kind in c["cameras"]:
        if c["limit"] or kind == "integer":
            cams.append((np.round(pos) if kind == "integer" else pos, np.array(IDENTITY)))
        else:
            cams.append((pos, q))
    _scenes[name] = (sc, st, cams, st["fov"] * np.pi / 8)
    return _scenes[name]


def voxel_ids_at(sc, points):
    """Material ids of the scene at world positions [n, 3], as Frame.get_voxel finds them: the chunk's resolution snaps the
    position's floor to a multiple of it (0 outside the box and in missing chunks)."""
    cs = sc.chunk_size
    fp = np.floor(points).astype(np.int64)
    cell = (fp - sc.origin) // cs
    ok = ((cell >= 0) & (cell < sc.dims)).all(1)
    cell = np.where(ok[:, None], cell, 0)
    ok &= sc.present[cell[:, 0], cell[:, 1], cell[:, 2]] != 0
    r = sc.res[cell[:, 0], cell[:, 1], cell[:, 2]].astype(np.int64)[:, None]
    sp = (fp // r) * r - sc.origin
    ok &= ((sp // cs) == cell).all(1)
    sp = np.where(ok[:, None], sp, 0)
    return np.where(ok, sc.grid[sp[:, 0], sp[:, 1], sp[:, 2]], 0), np.where(ok, r[:, 0], 0)


def edge_proof(name, o):
    """Does a frame (first camera) reach the edge the case is named after?  `o`: its "rays" (the oracle's record fields),
    "traversed" and "n_rays".  Returns the figures it asserts on (the comments of EDGE_CASES), from that output and the
    inputs alone."""
    sc, st, cams, lens = edge_scene(name)
    rays = o["rays"]
    cnt = rays["counters"]
    fig = dict(rays=len(rays), hits=int(cnt[:, CNT["hit"]].sum()))
    broke = rays[cnt[:, CNT["broke"]] == 1]
    if name in ("w1", "h1", "one_pixel"):
        assert fig["rays"] == o["n_rays"] > 0
        return fig
    assert fig["hits"] > 0, fig
    if name == "cs64":
        fig["chunk_get"] = int(cnt[:, CNT["chunk_get"]].sum())
        assert fig["chunk_get"] > 0
    elif name == "far_pos":
        fig["trav_min"] = int(o["traversed"].min())
        assert fig["trav_min"] > 1 << 25
    elif name == "far_neg":
        fig["trav_max"] = int(o["traversed"].max())
        assert fig["trav_max"] < -(1 << 26)
    elif name.startswith("limit_28"):
        fig["by_distance"] = int(((cnt[:, CNT["broke"]] == 0) & (rays["step"] >= rays["life"])).sum())
        assert fig["by_distance"] > 0
    elif name == "res9":
        assert set(np.unique(sc.res[sc.present != 0])) >= {5, 7, 9}
        fig["broke_in_res5plus"] = int((voxel_ids_at(sc, broke["pos"])[1] >= 5).sum())
        fig["resnap"] = int(cnt[:, CNT["resnap"]].sum())
        assert fig["broke_in_res5plus"] > 0 and fig["resnap"] > 0
    elif name == "fov179":
        # init.py:41-43 without the jitter: lens_x = dir_x / proportions * lens degrees, the kernel takes sin / cos of half of it
        px = np.unique(np.stack([rays["x"], rays["y"]], 1), axis=0)
        half = np.abs((-1 + px[:, 0] / st["width"] * 2) / st["proportions"] * lens) * (np.pi / 180) / 2
        fig["half_angles_from_pi_4"] = int((half >= np.pi / 4).sum())
        assert fig["half_angles_from_pi_4"] > 0
    elif name in ("bounces_half", "bounces16"):
        fig["at_cap"] = int((rays["bounces"] >= st["max_bounces"] + 1).sum())
        assert fig["at_cap"] > 0
        if name == "bounces16":
            fig["draw_max"] = int(cnt[:, CNT["draw"]].max())
            fig["draw_over_32"] = int((cnt[:, CNT["draw"]] > 32).sum())
            assert fig["draw_over_32"] > 0
    elif name == "lod_full":
        per_pixel = np.unique(rays["x"].astype(np.int64) * st["height"] + rays["y"], return_counts=True)[1]
        fig["pixels"], fig["pixels_below_9"] = len(per_pixel), int((per_pixel < 9).sum())
        fig["life_below_1"], fig["life_0"] = int((rays["life"] < 1).sum()), int((rays["life"] == 0).sum())
        assert per_pixel.max() == 9 and fig["pixels_below_9"] > 0 and fig["life_below_1"] > 0
    elif name == "near4":
        assert (rays["life"] <= 1 * rays["detail"]).all()
    elif name == "rough25_abs7":
        ids = voxel_ids_at(sc, broke["pos"])[0]
        fig["materials_hit"] = len(set(ids[ids > 0].tolist()))
        assert fig["materials_hit"] >= 10
    elif name == "fill_sparse":
        fig["adv"] = int(cnt[:, CNT["adv"]].sum())
        assert fig["adv"] > 100 * fig["hits"]
    elif name == "fill_dense":
        fig["rays_that_hit"] = int((cnt[:, CNT["hit"]] >= 1).sum())
        assert fig["rays_that_hit"] >= 0.98 * len(rays)
    return fig


# ---- the boundary-camera scene (tests/test_gpu_parity.py::test_axis_aligned_rays_from_integer_and_boundary_cameras) ----------
# unrotated camera on chunk corners, faces, the origin and one ulp beside them
BOUNDARY_POSITIONS = [(0.0, 0.0, 0.0), (16.0, 16.0, 16.0), (8.0, 16.0, -16.0), (-0.0, 5.0, -5.0), (-16.0, 0.0, 31.0),
                      (1e-300, -1e-300, 15.999999999999998), (32.0, -32.0, 0.5)]
BOUNDARY_RES_CAPS = (1, 3)      # resolutions <= 1 only (RESMODE 0 kernel) and up to 3


def boundary_scene(res_cap):
    """(scene, settings, rotation, lens) of the seed-12345 world -- 4^3 chunks of 16 round the origin, fill 0.08, resolutions
    1..3 cut to `res_cap` -- with no jitter, dist_min 0 and an even image size: the centre column / row rays of an unrotated
    camera move along the axes planes with coordinates that stay integers."""
    key = ("boundary", res_cap)
    if key not in _scenes:
        rng = np.random.default_rng(12345)
        cs = 16
        dims = np.array([4, 4, 4])
        origin = np.array([-32, -32, -32], np.int64)
        present = (rng.random(tuple(dims)) < 0.85).astype(np.uint8)
        res = rng.integers(1, 4, tuple(dims)).astype(np.uint8)
        grid = np.where(rng.random(tuple(dims * cs)) < 0.08, rng.integers(1, 5, tuple(dims * cs)), 0).astype(np.uint8)
        r_ = np.minimum(res, res_cap).astype(np.uint8)
        sc = ol.Scene(origin, dims, cs, present, r_, ol.Scene.camera_grid(grid, origin, dims, cs, present, r_), MATS4)
        st = ol.make_settings(width=32, height=24, samples=2, max_bounces=4.0, chunk_size=cs, dist_max=96, dist_min=0,
                              dof=0.0, lod_edge=0.0, lod_random=0.0, lod_samples=0.0, fov=90.0)
        _scenes[key] = (sc, st, np.array(IDENTITY), st["fov"] * np.pi / 8)
    return _scenes[key]


# ---- every render pinned to the real reference (tests/golden/edges/) ---------------------------------------------------------
def reference_renders():
    """[(fixture name, scene, settings, camera position, rotation, lens, has_background)]: every camera of every EDGE_CASES
    entry, no_background, and the 7 boundary positions at both resolution caps."""
    out = []
    for name in EDGE_CASES:
        sc, st, cams, lens = edge_scene(name)
        for k, (pos, q) in enumerate(cams):
            out.append((name if k == 0 else "%s_cam%d" % (name, k), sc, st, pos, q, lens, True))
    sc, st, cams, lens = edge_scene("no_background")
    out.append(("no_background", sc, st, cams[0][0], cams[0][1], lens, False))
    for cap in BOUNDARY_RES_CAPS:
        sc, st, q, lens = boundary_scene(cap)
        for k, pos in enumerate(BOUNDARY_POSITIONS):
            out.append(("boundary%d_res%d" % (k, cap), sc, st, np.array(pos), q, lens, True))
    return out


def scene_sha256(sc):
    """SHA-256 over the arrays of a scene that a test rebuilds: origin, dims, present, res, camera grid, materials."""
    h = hashlib.sha256()
    for a, t in ((sc.origin, "<i8"), (sc.dims, "<i8"), (sc.present, "u1"), (sc.res, "u1"), (sc.grid, "u1"), (sc.materials, "<f8")):
        a = np.ascontiguousarray(np.asarray(a).astype(t))
        h.update(("%s%s;" % (t, a.shape)).encode())
        h.update(a.tobytes())
    return h.hexdigest()


def load_reference_render(name):
    """A fixture of tests/golden/edges/ (tests/golden/make_golden_edges.py): its arrays, `settings` decoded, and

        scene, st, has_background   the scene rebuilt from this module and the oracle-style settings of the fixture's JSON
        ref_rays                    the reference's rays as a structured array with the oracle's field names -- every field
                                    for a full fixture; x, y, s, color, alpha, energy, counters and the extra columns for a
                                    compact one
        ref_traversed               int64 [n, 3]

    The scene is not stored: a fixture whose hash is not the rebuilt scene's fails here."""
    import json
    import os
    z = np.load(os.path.join(ol.GOLDEN, "edges", "%s.npz" % name))
    g = {k: z[k] for k in z.files}
    g["settings"] = s = json.loads(bytes(g["settings"]).decode())
    _, sc, st, pos, q, lens, has_bg = [r for r in reference_renders() if r[0] == name][0]
    assert str(g["scene_sha256"]) == scene_sha256(sc), "%s: the fixture was rendered from another scene" % name
    assert {k: s[k] for k in st} == st, (name, s, st)
    assert np.array_equal(g["cam_pos"], pos) and np.array_equal(g["cam_rot"], q) and g["cam_lens"][0] == lens
    assert bool(g["has_background"][0]) == has_bg and list(g["counter_names"]) == ol.COUNTERS
    g["scene"], g["st"], g["has_background"] = sc, st, has_bg
    n = int(g["n_rays"][0])
    cols = {}
    if "rays" in g:
        F = {k: i for i, k in enumerate(g["ray_fields"])}
        R = g["rays"]
        for f in ("x", "y", "s", "alpha", "ntrav"):
            cols[f] = R[:, F[f]].astype(np.int32)
            assert np.array_equal(cols[f], R[:, F[f]])
        cols["color"] = R[:, [F["r"], F["g"], F["b"]]].astype(np.int32)
        cols["counters"] = R[:, [F["c_" + c] for c in ol.COUNTERS]].astype(np.int32)
        assert np.array_equal(cols["color"], R[:, [F["r"], F["g"], F["b"]]])
        for f in ("detail", "energy", "step", "life", "bounces"):
            cols[f] = R[:, F[f]]
        cols["pos"] = R[:, [F["px"], F["py"], F["pz"]]]
        cols["vel"] = R[:, [F["vx"], F["vy"], F["vz"]]]
    else:
        rr = g["ray_rgba"]
        cols.update(x=rr[:, 0], y=rr[:, 1], s=rr[:, 2], color=rr[:, 3:6], alpha=rr[:, 6], energy=g["ray_energy"],
                    counters=g["ray_counters"])
        for i, f in enumerate(g.get("ray_extra_fields", [])):
            cols[str(f)] = g["ray_extra"][:, i]
    dt = np.dtype([(f, a.dtype, a.shape[1:]) for f, a in cols.items()])
    rays = np.zeros(n, dt)
    for f, a in cols.items():
        assert len(a) == n
        rays[f] = a
    g["ref_rays"] = rays
    g["ref_traversed"] = g["traversed_t0"].astype(np.int64)
    assert np.array_equal(g["ref_traversed"], g["traversed_t0"])
    assert np.array_equal(rays["counters"].sum(0), g["counters_total"])
    return g
