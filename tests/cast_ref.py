"""References for explicit rays (Camera.cast_rays -> vrt_cast_rays, cast_kernel).

1. The CPU oracle.  It only traces camera pixels, but a 2 x 2 window's pixel (1, 1) has dir_x = dir_y = 0, and with dof = 0
   the lens quaternion is the identity: that pixel's one ray is origin = cam.pos + vel * dist_min, vel = cam.rot.vec_forward()
   (lib.py:372-376), life = dist_max - dist_min.  One oracle call per ray, each with its own pose and dist_max, so a set of
   rays is a set of (position, quaternion, life) triples; non-unit quaternions vary |vel|.  Materials are the id-materials of
   tests/test_gpu_first_hit.py and max_bounces = 0, so the oracle's end state is the first-hit state.
2. `march`: a short restatement of init.py:66-116 up to the first voxel over an oracle_lib.Scene, for arbitrary velocities.
   tests/test_cast_host.py pins it to the oracle on the CPU; after that it stands in for rays the oracle cannot express."""
import math

import numpy as np

import oracle_lib as ol
from python_raytracer_amd import _native as nat

HIT_DTYPE = np.dtype(nat.HIT_FIELDS)
PIXEL = np.array([[1, 1]], np.int32)


def id_materials(n):
    """n material records whose albedo is (id, 0, 0): a ray that breaks at its first voxel carries the voxel's id as its red."""
    mats = np.zeros((n, 7))
    mats[:, 0] = np.arange(1, n + 1)
    mats[:, 4] = 1.0
    return mats


def id_scene(sc):
    return ol.Scene(sc.origin, sc.dims, sc.chunk_size, sc.present, sc.res, sc.grid,
                    id_materials(max(int(sc.grid.max()), len(sc.materials))))


def ray_settings(chunk_size, dist_min, dist_max):
    return ol.make_settings(width=2, height=2, samples=1, chunk_size=chunk_size, dof=0.0, lod_bounces=0.0, lod_samples=0.0,
                            lod_random=0.0, lod_edge=0.0, max_bounces=0.0, dist_min=dist_min, dist_max=dist_max)


def vec_forward(q):
    """quaternion.vec_forward (lib.py:372-376) for rows (x, y, z, w), in the reference's operation order."""
    x, y, z, w = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    return np.stack([2 * (z * x + w * y), 2 * (y * x - w * z), 1 - 2 * (z * z + y * y)], -1)


def assert_records_equal(got, exp):
    """Bit for bit, field by field (the doubles as their 64-bit patterns: -0.0 is not 0.0 here)."""
    assert got.shape == exp.shape
    assert np.array_equal(got["material"], exp["material"])
    assert np.array_equal(got["cell"], exp["cell"])
    assert np.array_equal(got["step"].view(np.uint64), exp["step"].view(np.uint64))
    assert np.array_equal(got["pos"].view(np.uint64), exp["pos"].view(np.uint64))


def assert_not_vacuous(exp):
    """More than 10 % of the rays hit, more than 10 % miss, at least 3 materials are found."""
    hit = exp["material"] > 0
    assert 0.1 < hit.mean() < 0.9, hit.mean()
    assert len(set(exp["material"][hit].tolist())) >= 3, set(exp["material"][hit].tolist())


def oracle_cast(sc, cam_pos, quats, lives, dist_min=0.0, vacuous_ok=False):
    """One oracle call per ray.  Returns (origins [n, 3], vels [n, 3], lives [n], expected vrt_hit records [n]): the rays as
    the cast takes them -- the velocity from numpy's vec_forward and the life (dist_min + life) - dist_min, both asserted
    bit-identical to the oracle's on every missing ray (a hit Chebyshev-normalises the oracle's velocity and divides its life by
    the chunk's resolution) -- and what it must find."""
    cam_pos = np.asarray(cam_pos, np.float64).reshape(-1, 3)
    quats = np.asarray(quats, np.float64).reshape(-1, 4)
    lives = np.asarray(lives, np.float64).reshape(-1)
    n = len(cam_pos)
    ids = id_scene(sc)
    vels = vec_forward(quats)
    origins = cam_pos + vels * float(dist_min)
    out_lives = (float(dist_min) + lives) - float(dist_min)      # init.py:56 with detail = 1
    exp = np.zeros(n, HIT_DTYPE)
    for k in range(n):
        st = ray_settings(sc.chunk_size, float(dist_min), float(dist_min) + float(lives[k]))
        o = ol.render(ids, st, cam_pos[k], quats[k], st["fov"] * np.pi / 8, PIXEL, libm=ol.LIBM_PORTABLE, has_background=False,
                      want_traversed=False)
        rays = o["rays"]
        assert len(rays) == 1
        r = rays[0]
        hit = int(r["counters"][4]) == 1
        assert int(r["counters"][4]) <= 1
        if not hit:
            assert r["step"] >= r["life"] and r["bounces"] == 0
            assert np.array_equal(r["vel"].view(np.uint64), vels[k].view(np.uint64)), (k, r["vel"], vels[k])
            assert r["life"] == out_lives[k], (k, r["life"], out_lives[k])
        exp["step"][k] = r["step"]
        exp["pos"][k] = r["pos"]
        exp["cell"][k] = np.floor(r["pos"]).astype(np.int32)
        exp["material"][k] = int(r["color"][0]) if hit else 0
    if not vacuous_ok:
        assert_not_vacuous(exp)
    return origins, vels, out_lives, exp


def march(sc, chunk_radius, origin, vel, life):
    """init.py:66-116 up to the first voxel for one ray over an oracle_lib.Scene, in Python floats: the chunk re-snap with
    the reference's inclusive box, present / res, the voxel asked for at (floor(pos) // r) * r -- empty if that lies outside
    the chunk -- and the void step 1 + abs(radius - (min(pos) + radius) % cs) with Python's float %.
    Returns (step, pos, material): material 0 when the life ran out first."""
    cs = sc.chunk_size
    org = [int(v) for v in sc.origin]
    dims = [int(v) for v in sc.dims]
    pos = [float(v) for v in origin]
    vel = [float(v) for v in vel]
    life = float(life)
    step = 0.0
    cmin = cmax = (0.0, 0.0, 0.0)
    chunk = None                                   # (cell index in the scene box) of a present chunk
    while step < life:
        if not all(p >= c for p, c in zip(pos, cmin)) or not all(p <= c for p, c in zip(pos, cmax)):
            cmin = tuple((p // cs) * cs for p in pos)
            cmax = tuple(c + cs for c in cmin)
            cell = tuple((int(c) - o) // cs for c, o in zip(cmin, org))
            chunk = cell if all(0 <= i < d for i, d in zip(cell, dims)) and sc.present[cell] else None
        if chunk is not None:
            res = int(sc.res[chunk])
            f = [math.floor(p) for p in pos]
            q = [(v // res) * res for v in f] if res > 1 else f
            mat = 0
            if all(int(c) <= v < int(c) + cs for v, c in zip(q, cmin)):
                mat = int(sc.grid[q[0] - org[0], q[1] - org[1], q[2] - org[2]])
            if mat:
                return step, pos, mat
            size = res if res else 1               # (Frame.resolution; a zero must not stall the march)
        else:
            size = 1 + abs(chunk_radius - (min(pos) + chunk_radius) % cs)
        step += size
        pos = [p + v * size for p, v in zip(pos, vel)]
    return step, pos, 0


def march_records(sc, chunk_radius, origins, vels, lives):
    """`march` for a set of rays, as vrt_hit records."""
    exp = np.zeros(len(origins), HIT_DTYPE)
    for k, (o, v, l) in enumerate(zip(origins, vels, lives)):
        step, pos, mat = march(sc, chunk_radius, o, v, l)
        exp["step"][k] = step
        exp["pos"][k] = pos
        exp["cell"][k] = [math.floor(p) for p in pos]
        exp["material"][k] = mat
    return exp


# ---- the ray sets of the oracle comparisons: computed once, shared by the CPU and the GPU tests, never changed ----------------
def unit_quats(rng, n):
    q = rng.normal(size=(n, 4))
    return q / np.linalg.norm(q, axis=1)[:, None]


_sets = {}


def ray_set(name):
    """(scene, origins, vels, lives, expected records) of a named oracle comparison.
    default / synth64: the two sets of 1 500 rays checked on the CPU oracle to hit 52 % / 18.5 % of the time, 13 materials each;
    hand / big_table: 500 rays each over test_gpu_first_hit's hand_scene() (resolutions 1, 2 and 3, holes, most origins
    outside the box) and big_table_scene() (4 352 table cells, read from memory);
    default_scaled / default_dmin: the default scene with quaternions of norm 0.5 .. 1.5 (|vel| varies), and with dist_min = 3."""
    if name in _sets:
        return _sets[name]
    dist_min = 0.0
    if name == "default":
        sc = ol.default_scene()
        rng = np.random.default_rng(1)
        pos = rng.uniform([-64, -32, -64], [64, 40, 64], (1500, 3))
        q = unit_quats(rng, 1500)
        lives = rng.uniform(8, 64, 1500)
    elif name == "synth64":
        sc = ol.synth64_scene()
        rng = np.random.default_rng(2)
        pos = rng.uniform(-40, 40, (1500, 3))
        q = unit_quats(rng, 1500)
        lives = rng.uniform(4, 48, 1500)
    elif name in ("default_scaled", "default_dmin"):
        sc = ol.default_scene()
        rng = np.random.default_rng(3 if name == "default_scaled" else 4)
        pos = rng.uniform([-64, -32, -64], [64, 40, 64], (500, 3))
        q = unit_quats(rng, 500)
        if name == "default_scaled":
            q = q * rng.uniform(0.5, 1.5, (500, 1))
        else:
            dist_min = 3.0
        lives = rng.uniform(8, 64, 500)
    elif name == "hand":
        from test_gpu_first_hit import hand_scene
        sc = hand_scene()
        rng = np.random.default_rng(5)
        pos = rng.uniform([-20, -12, -4], [20, 20, 20], (500, 3))
        q = unit_quats(rng, 500)
        lives = rng.uniform(4, 40, 500)
    elif name == "big_table":
        from test_gpu_first_hit import big_table_scene
        sc = big_table_scene()
        rng = np.random.default_rng(6)
        pos = rng.uniform(-60, 60, (500, 3))
        q = unit_quats(rng, 500)
        lives = rng.uniform(4, 48, 500)
    else:
        raise KeyError(name)
    origins, vels, lives, exp = oracle_cast(sc, pos, q, lives, dist_min)
    for a in (origins, vels, lives, exp):
        a.setflags(write=False)
    _sets[name] = (sc, origins, vels, lives, exp)
    return _sets[name]
