"""Reference for the surface pass (Camera.surfaces -> vrt_hit_surfaces, surface_kernel) and the scenes and rays its tests share.

1. `surface`: the rule of include/vrt.h (section "surfaces of hit records") for one hit record and its ray's velocity, in Python
   floats over an oracle_lib.Scene: the current chunk from owner_ref.counting, the three neighbour probes of init.py:92-111
   through shade_ref._chunk / _lookup, the project's normal.  It also says how many neighbour lookups and chunk_gets the
   reflection made, which tests/test_surface_host.py holds to shade_ref.trace's counters.
2. `expect`: vrt_surface records and the statistics words for arrays of records, validation included.
3. `cases()`: the three scenes (gpu_util.sparse_scene, owner_ref.lod_world, the edge scene res9 at chunk size 32) with smooth
   materials whose ior is drawn from {0, 0.25, 0.5, 0.75, 1}, their rays, the first hits and the lives that end shade_ref.trace
   with the step after the hit.  Built once, shared by the CPU and the GPU tests, never changed.
4. `edge_case`, `lattice_case`: the same over the edge scenes of tests/edge_scenes.py -- with the ray sets of tests/edge_rays.py,
   and with whole-number rays that end exactly on chunk faces."""
import math

import numpy as np

import cast_ref as cr
import owner_ref as orf
import shade_ref as sr
from python_raytracer_amd import _native as nat

SURFACE_DTYPE = np.dtype(nat.SURFACE_FIELDS)
LIMIT = float(1 << 28)
IORS = (0.0, 0.25, 0.5, 0.75, 1.0)


def _cmin(sc, cell):
    return tuple(float(int(o) + i * sc.chunk_size) for o, i in zip(sc.origin, cell))


def normalized(vel):
    """lib.py:310-314: the Chebyshev normalize, left alone where the largest component is 0 or 1."""
    v = [float(x) for x in vel]
    ref = max(abs(v[0]), abs(v[1]), abs(v[2]))
    if ref != 0.0 and ref != 1.0:
        v = [x / ref for x in v]
    return v


def reflect(sc, cell, pos, v, ior):
    """init.py:92-111 for a ray at `pos` with the normalised velocity `v` that stands in the present chunk `cell`.
    Returns dict(vel, neighbour, reflect, side, fetched, lookups, fetches)."""
    cs = sc.chunk_size
    out = dict(vel=list(v), neighbour=[0, 0, 0], reflect=0, side=0, fetched=0, lookups=0, fetches=0)
    if ior == 0.0:
        return out
    cmin = _cmin(sc, cell)
    cmax = tuple(c + cs for c in cmin)
    direction = (ior - 0.5) * 2
    for a in range(3):
        p = list(pos)
        up = v[a] < direction
        p[a] = pos[a] + 1 if up else pos[a] - 1
        out["side"] |= int(up) << a
        if all(x >= c for x, c in zip(p, cmin)) and all(x <= c for x, c in zip(p, cmax)):
            nchunk, ncmin = cell, cmin
        else:
            ncmin = tuple((x // cs) * cs for x in p)
            nchunk = sr._chunk(sc, ncmin)
            out["fetched"] |= 1 << a
            out["fetches"] += 1
        nid = 0
        if nchunk is not None:
            nid = sr._lookup(sc, nchunk, ncmin, [math.floor(x) for x in p])
            out["lookups"] += 1
        out["neighbour"][a] = nid
        if not (nid and float(sc.materials[nid - 1][5]) == ior):
            out["reflect"] |= 1 << a
            out["vel"][a] = v[a] - v[a] * ior * 2
    return out


def normal(sc, f, v):
    """The project's normal: (normal, open bits).  The incoming-side neighbour cell of every axis the ray moves on is open if its
    chunk is not listed or Frame.get_voxel finds nothing there; the open axis with the largest |v| (the lowest on a tie) gives
    -sgn(v); none open: (0, 0, 0)."""
    cs = sc.chunk_size
    n, opened, best = [0, 0, 0], 0, 0.0
    for a in range(3):
        if v[a] == 0.0:
            continue
        q = list(f)
        q[a] -= 1 if v[a] > 0 else -1
        ncmin = tuple(float((x // cs) * cs) for x in q)
        chunk = sr._chunk(sc, ncmin)
        if chunk is None or sr._lookup(sc, chunk, ncmin, q) == 0:
            opened |= 1 << a
            if abs(v[a]) > best:
                best, n = abs(v[a]), [0, 0, 0]
                n[a] = -1 if v[a] > 0 else 1
    return n, opened


def surface(sc, pos, cell, material, vel):
    """One record.  Returns dict(status, and for status 0: vel, next, normal, neighbour, resolution, reflect, side, fetched,
    open, lookups, fetches, ambiguous, chunk -- the scene-box cell of the chunk taken as the current one)."""
    material = int(material)
    if material <= 0:
        return dict(status=nat.SURFACE_NONE)
    pos, vel = [float(x) for x in pos], [float(x) for x in vel]
    if (not all(math.isfinite(x) for x in pos + vel) or any(abs(x) >= LIMIT for x in pos) or
            [math.floor(x) for x in pos] != [int(c) for c in cell] or material > len(sc.materials)):
        return dict(status=nat.SURFACE_INVALID)
    got = orf.counting(sc, pos, material)
    if not got:
        return dict(status=nat.SURFACE_ORPHAN)
    v = normalized(vel)
    ior = float(sc.materials[material - 1][5])
    chunk, r, c = got[0]
    out = reflect(sc, chunk, pos, v, ior)
    out["ambiguous"] = False
    for other, _, _ in got[1:]:
        alt = reflect(sc, other, pos, v, ior)
        same_vel = np.array_equal(np.array(alt["vel"]).view(np.uint64), np.array(out["vel"]).view(np.uint64))
        out["ambiguous"] |= not same_vel or alt["reflect"] != out["reflect"] or alt["neighbour"] != out["neighbour"]
    out["status"], out["resolution"], out["chunk"] = 0, r, chunk
    out["next"] = [p + w * float(r) for p, w in zip(pos, out["vel"])]
    out["normal"], out["open"] = normal(sc, [int(x) for x in cell], v)
    return out


def expect(sc, hits, vels):
    """(vrt_surface records, the 16 statistics words, the per-record dicts) for vrt_hit records `hits` (numpy, cast_ref.HIT_DTYPE)
    reached with the velocities `vels` [n, 3]."""
    exp = np.zeros(len(hits), SURFACE_DTYPE)
    stats = np.zeros(nat.NSTATS, np.int64)
    recs = []
    for k in range(len(hits)):
        s = surface(sc, hits["pos"][k], hits["cell"][k], hits["material"][k], vels[k])
        recs.append(s)
        exp["status"][k] = s["status"]
        stats[nat.S_SURFACE_EXAMINED] += int(hits["material"][k]) > 0
        stats[nat.S_SURFACE_ORPHANS] += s["status"] == nat.SURFACE_ORPHAN
        stats[nat.S_SURFACE_INVALID] += s["status"] == nat.SURFACE_INVALID
        if s["status"] != 0:
            continue
        for name in ("vel", "next", "normal", "neighbour", "resolution", "reflect", "side", "fetched", "open"):
            exp[name][k] = s[name]
        stats[nat.S_SURFACE_RESOLVED] += 1
        stats[nat.S_SURFACE_AMBIGUOUS] += s["ambiguous"]
        stats[nat.S_SURFACE_ENCLOSED] += s["normal"] == [0, 0, 0]
    return exp, stats, recs


def assert_records_equal(got, exp):
    """Byte for byte, and field by field first so that a failure names its field."""
    assert got.shape == exp.shape
    for name in SURFACE_DTYPE.names:
        a, b = np.ascontiguousarray(got[name]), np.ascontiguousarray(exp[name])
        if a.dtype == np.float64:
            a, b = a.view(np.uint64), b.view(np.uint64)
        assert np.array_equal(a, b), (name, np.nonzero((a != b).reshape(len(got), -1).any(1))[0][:8])
    assert got.tobytes() == exp.tobytes()


# ---- the shared scenes and rays ---------------------------------------------------------------------------------------------
def smooth_materials(n, seed, rough=False):
    """n materials of absorption 1 and emission 0 with ior drawn from IORS (a random order of them, repeated); roughness 0, or -- rough -- 0.3 for every third."""
    rng = np.random.default_rng(seed)
    m = np.zeros((n, 7))
    m[:, :3] = rng.integers(20, 256, (n, 3))
    m[:, 4] = 1.0
    m[:, 5] = np.resize(rng.permutation(IORS), n)          # (every value occurs once n reaches 5)
    if rough:
        m[::3, 3] = 0.3
    return m


def trace_settings(chunk_size):
    """Settings under which a ray goes on after every hit until its life ends it: no cap on bounces or light, and a life that
    a hit divides by the chunk's resolution alone (lod_bounces 0)."""
    return sr.shade_settings(chunk_size, 1e6, 1e6, lod_bounces=0.0)


CASES = ("sparse", "lod", "res9")
_cases = {}


def case(name, rough=False):
    """dict(scene, settings, origins, vels, lives, hits, vel_in, end_lives, truth) of a scene of CASES.
    origins / vels / lives: the rays; hits: their first-hit records (cast_ref.march); truth: owner_ref.march_true per ray;
    end_lives: for a ray that hits, the life with which shade_ref.trace (and vrt_shade_rays) takes the step after that hit and
    ends -- (step + 0.5) * r, which the hit divides by r: above `step`, so the loop goes on to the reflection, and at most
    step + r, so it ends after one advance; 1.0 for a ray that hits nothing.
    rough: the same scene and rays with every third material rough (the hits are the same: the first hit reads no material)."""
    key = (name, rough)
    if key in _cases:
        return _cases[key]
    if name == "sparse":
        from gpu_util import sparse_scene
        base = sparse_scene(77, 3, fill=0.12)
        cells = np.argwhere(base.grid != 0)[::40] + base.origin
        lo, hi = base.origin.astype(np.float64) - 2, (base.origin + base.dims * base.chunk_size).astype(np.float64) + 2
        origins, vels, lives = orf.casts_at(cells[:12], lo, hi, 400, 5)
    elif name == "lod":
        lw = orf.lod_world()
        base, origins, vels, lives = lw["scene"], lw["origins"], lw["vels"], lw["lives"]
    elif name == "res9":
        import edge_rays as er
        base, st, has_bg, origins, vels, lives = er.edge_ray_set("res9")[:6]
    else:
        raise KeyError(name)
    mats = smooth_materials(len(base.materials), 31 + CASES.index(name), rough)
    if name == "lod":
        # the two one-voxel objects' material: above 0.5 the y neighbour is asked at +1, where the chunk at resolution 3 snaps it
        # back onto the hit voxel and the chunk above finds nothing -- the constructed record is then ambiguous (test_surface_host)
        mats[int(lw["truth"][-1][2]) - 1, 5] = 0.75
    _cases[key] = _finish(base, mats, origins, vels, lives)
    return _cases[key]


def _finish(base, mats, origins, vels, lives):
    """The common tail of case(), edge_case() and lattice_case(): the scene with the smooth materials, the first hits, the
    truth and the lives that end shade_ref.trace one step after each hit."""
    sc = sr.with_materials(base, mats)
    radius = round(sc.chunk_size / 2)
    hits = cr.march_records(sc, radius, origins, vels, lives)
    truth = [orf.march_true(sc, radius, o, v, l) for o, v, l in zip(origins, vels, lives)]
    end_lives = np.ones(len(hits))
    for k, t in enumerate(truth):
        assert (t[0], t[2]) == (hits["step"][k], hits["material"][k])
        if t[2]:
            end_lives[k] = (t[0] + 0.5) * t[4]
    out = dict(scene=sc, settings=trace_settings(sc.chunk_size), origins=np.array(origins, np.float64), vels=np.array(vels, np.float64),
               lives=np.array(lives, np.float64), hits=hits, end_lives=end_lives, truth=truth)
    for a in (out["origins"], out["vels"], out["lives"], hits, end_lives):
        a.setflags(write=False)
    return out


# ---- the edge scenes (tests/edge_scenes.py) --------------------------------------------------------------------------------
_edge_cases, _lattice_cases = {}, {}


def edge_names():
    import edge_rays as er
    return list(er.ALL_CASES)


def edge_case(name):
    """case()'s dict for a set of tests/edge_rays.py: the scene of edge_scenes.edge_scene(name) with smooth materials (seed
    131 + the case's place in edge_rays.ALL_CASES) and the origins, velocities and lives of edge_rays.edge_ray_set(name) --
    chunk sizes 8, 32 and 64, worlds 2^26 to 2^27 cells out, origins beside +-2^28, resolutions up to 9, a dense and a 0.5 %
    grid.  (case("res9") is this for one scene, under its own seed.)"""
    if name not in _edge_cases:
        import edge_rays as er
        base, st, has_bg, origins, vels, lives = er.edge_ray_set(name)[:6]
        mats = smooth_materials(len(base.materials), 131 + er.ALL_CASES.index(name))
        _edge_cases[name] = _finish(base, mats, origins, vels, lives)
    return _edge_cases[name]


LATTICE_CASES = ("fill_dense", "fill_sparse", "cs64", "far_pos", "far_neg", "far_mixed", "limit_28_pos", "limit_28_neg", "res9", "lod_full")
LATTICE_RAYS = 400
LATTICE_SCALES = (0.5, 1.0, 2.0, 3.0)


def lattice_rays(sc, seed, n=LATTICE_RAYS):
    """n rays that end exactly on chunk faces: whole-number origins `cell - d * k` (k in 1..6) in front of filled cells, with a
    direction d of {-1, 0, 1}^3 less 0 scaled by one of LATTICE_SCALES, life 40.  The cells, by quota and in this order (a quota
    no cell fills goes to the next): chunk corners (all three coordinates multiples of the chunk size); cells on the scene box's
    lowest faces (a coordinate equal to the box's origin); cells in the box's last layer or on its highest chunk face (a
    coordinate of the box's end less 1 or less a chunk size); cells with one or two coordinates on a chunk face; any cell.
    In a scene with resolutions that do not divide a chunk face's coordinate the last fifth are upper_face_rays instead."""
    import edge_rays as er
    rng = np.random.default_rng(seed)
    cs = sc.chunk_size
    cells, _ = er.filled_cells(sc)
    origin = np.asarray(sc.origin, np.int64)
    end = origin + np.asarray(sc.dims, np.int64) * cs
    on_face = (cells - origin) % cs == 0
    pools = [np.flatnonzero(on_face.all(1)), np.flatnonzero((cells == origin).any(1)),
             np.flatnonzero(((cells == end - 1) | (cells == end - cs)).any(1)), np.flatnonzero(on_face.any(1)), np.arange(len(cells))]
    quotas = [n * 3 // 20, n // 4, n // 4, n // 4, n - n * 3 // 20 - 3 * (n // 4)]
    pick, carry = [], 0
    for pool, quota in zip(pools, quotas):
        quota += carry
        carry = 0
        if len(pool) == 0:
            carry = quota
            continue
        pick.append(pool[rng.integers(0, len(pool), quota)])
    pick = np.concatenate(pick)
    assert len(pick) == n
    dirs = np.array([d for d in np.ndindex(3, 3, 3) if d != (1, 1, 1)], np.int64) - 1
    d = dirs[rng.integers(0, len(dirs), n)]
    k = rng.integers(1, 7, n)[:, None]
    scale = np.array(LATTICE_SCALES)[rng.integers(0, len(LATTICE_SCALES), n)][:, None]
    origins = (cells[pick] - d * k).astype(np.float64)
    vels = d * scale
    # where a chunk's resolution does not divide its upper face's coordinate (res9 alone among the edge scenes), the last fifth
    # of the set goes to rays whose record only the chunk BELOW the one containing `cell` explains
    faces = upper_face_rays(sc, rng)
    m = min(n // 5, len(faces))
    for i, (o, v) in enumerate(faces[:m]):
        origins[n - m + i], vels[n - m + i] = o, v
    return origins, vels, np.full(n, 40.0)


def upper_face_rays(sc, rng):
    """[(origin, velocity)], shuffled: unit rays along +a from one step (r cells) before the upper face F of a chunk of resolution
    r with F % r != 0, anywhere in the r^3 cell of a filled voxel at (F // r) * r -- after one step the ray stands on F, still in
    its chunk, and reads that voxel, while floor(pos) = F lies in the chunk above (owner_ref.lod_world aims its rays so)."""
    cs = sc.chunk_size
    out = []
    for cell in np.argwhere(sc.present != 0):
        r = int(sc.res[tuple(cell)])
        cmin = np.asarray(sc.origin, np.int64) + cell * cs
        lo = cell * cs
        block = sc.grid[lo[0]:lo[0] + cs, lo[1]:lo[1] + cs, lo[2]:lo[2] + cs]
        voxels = np.argwhere(block != 0) + cmin
        voxels = voxels[(voxels % r == 0).all(1)]
        for a in range(3):
            face = int(cmin[a]) + cs
            if face % r == 0 or face - r < cmin[a]:
                continue
            for q in voxels[voxels[:, a] == (face // r) * r]:
                o = np.minimum(q + rng.integers(0, r, 3), cmin + cs - 1)
                o[a] = face - r
                v = np.zeros(3)
                v[a] = 1.0
                out.append((o.astype(np.float64), v))
    return [out[i] for i in rng.permutation(len(out))]


def lattice_case(name):
    """case()'s dict for the lattice rays of an edge scene of LATTICE_CASES (smooth materials under seed 231 + its place there):
    the hits whose `pos` is a whole multiple of the chunk size on one, two or three axes -- the candidates m = 1..7 of the chunk
    rule, chunk indices -1 at the box's low faces, probes at index = dims past its high ones."""
    if name not in _lattice_cases:
        import edge_scenes as es
        base = es.edge_scene(name)[0]
        at = LATTICE_CASES.index(name)
        origins, vels, lives = lattice_rays(base, 7000 + at)
        _lattice_cases[name] = _finish(base, smooth_materials(len(base.materials), 231 + at), origins, vels, lives)
    return _lattice_cases[name]


def low_mask(sc, pos, cell):
    """Bit a: pos[a] is a whole multiple of the chunk size (the record's `low` of the chunk rule), from a record alone."""
    return sum(int(float(pos[a]) == float(int(cell[a])) and int(cell[a]) % sc.chunk_size == 0) << a for a in range(3))
