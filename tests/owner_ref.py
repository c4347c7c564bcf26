"""References for the owner pass (DeviceWorld.owners -> vrt_hit_owners, owner_kernel).

1. `record_voxel`: a short restatement of "which voxel a hit record means" (include/vrt.h, vrt_hit_owners): the candidate chunks
   of a record in their documented order, which of them count, and the first that does.
2. `march_true`: the reference's loop up to the first voxel (init.py:66-116, restated as tests/cast_ref.py restates it) that
   also returns what a record does not hold: the chunk the ray stood in, its resolution r and the voxel c = (floor(pos) // r) * r
   it read.  tests/test_owner_host.py pins it to cast_ref.march and checks the candidate rule against it on the CPU.
3. `lod_world`: the hand-built world of the LOD tests -- objects, host world with its owner grid, a camera scene with chunks at
   resolutions 1, 2 and 3, axis-aligned integer rays that meet the upper faces of resolution-3 chunks, and one constructed
   record that two chunks explain.  Built once, shared by the CPU and the GPU tests, never changed."""
import math

import numpy as np

import oracle_lib as ol
from cast_ref import id_materials

# which chunk a candidate is: (x, y, z) lowered by one chunk or not -- the containing chunk first (include/vrt.h)
ORDER = [(0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 0), (0, 0, 1), (1, 0, 1), (0, 1, 1), (1, 1, 1)]


def _voxel_in(sc, cell, f):
    """(r, c, byte) of scene-box cell `cell` for floor(pos) = f, or None: not listed, or c outside the chunk."""
    cs = sc.chunk_size
    if not all(0 <= i < d for i, d in zip(cell, sc.dims)) or not sc.present[cell]:
        return None
    r = int(sc.res[cell])
    c = [(v // r) * r for v in f]
    cmin = [int(o) + i * cs for o, i in zip(sc.origin, cell)]
    if not all(m <= v < m + cs for v, m in zip(c, cmin)):
        return None
    return r, tuple(c), int(sc.grid[c[0] - int(sc.origin[0]), c[1] - int(sc.origin[1]), c[2] - int(sc.origin[2])])


def counting(sc, pos, material):
    """The candidates of a record that count, in order: [(cell, r, c)].  Candidates: the chunk containing floor(pos) and, for
    every axis on which pos is a whole multiple of chunk_size, the chunk one below.  One counts if it is listed, its c lies
    inside it and the voxel there is `material`."""
    cs = sc.chunk_size
    f = [math.floor(p) for p in pos]
    low = [float(p) == float(v) and v % cs == 0 for p, v in zip(pos, f)]
    base = [(v - int(o)) // cs for v, o in zip(f, sc.origin)]
    out = []
    for d in ORDER:
        if any(d[a] and not low[a] for a in range(3)):
            continue
        cell = tuple(b - e for b, e in zip(base, d))
        hit = _voxel_in(sc, cell, f)
        if hit is not None and hit[2] == material:
            out.append((cell, hit[0], hit[1]))
    return out


def record_voxel(sc, pos, material):
    """(cell, r, c) of the first candidate that counts, or None (an orphan)."""
    got = counting(sc, pos, material)
    return got[0] if got else None


def march_true(sc, chunk_radius, origin, vel, life):
    """init.py:66-116 up to the first voxel for one ray over an oracle_lib.Scene, in Python floats.
    Returns (step, pos, material, cell, r, c): cell / r / c are None when the life ran out first."""
    cs = sc.chunk_size
    org = [int(v) for v in sc.origin]
    dims = [int(v) for v in sc.dims]
    pos = [float(v) for v in origin]
    vel = [float(v) for v in vel]
    life = float(life)
    step = 0.0
    cmin = cmax = (0.0, 0.0, 0.0)
    chunk = None
    while step < life:
        if not all(p >= c for p, c in zip(pos, cmin)) or not all(p <= c for p, c in zip(pos, cmax)):
            cmin = tuple((p // cs) * cs for p in pos)
            cmax = tuple(c + cs for c in cmin)
            cell = tuple((int(c) - o) // cs for c, o in zip(cmin, org))
            chunk = cell if all(0 <= i < d for i, d in zip(cell, dims)) and sc.present[cell] else None
        if chunk is not None:
            res = int(sc.res[chunk])
            hit = _voxel_in(sc, chunk, [math.floor(p) for p in pos])
            if hit is not None and hit[2]:
                return step, pos, hit[2], chunk, hit[0], hit[1]
            size = res if res else 1
        else:
            size = 1 + abs(chunk_radius - (min(pos) + chunk_radius) % cs)
        step += size
        pos = [p + v * size for p, v in zip(pos, vel)]
    return step, pos, 0, None, None, None


def is_face_case(sc, pos, cell):
    """The ray stood on an upper face of its chunk `cell`: floor(pos) lies in the next chunk on some axis."""
    cs = sc.chunk_size
    return any(p == int(o) + (i + 1) * cs for p, o, i in zip(pos, sc.origin, cell))


# ---- the hand-built LOD world --------------------------------------------------------------------------------------------
CS = 16
AMBIGUOUS_RAY = ((29.0, 21.0, 6.0), (1.0, 0.0, 0.0), 10.0)   # arrives at pos.x == 32.0 in the chunk [16, 32) at resolution 3

_lod = None


def lod_world():
    """dict(objs, world, scene, origins, vels, lives, truth): a world of 12 random boxes (one material each, z >= 32) and two
    one-voxel objects A and B of ONE material at (30, 21, 6) and (32, 21, 6); a camera scene over it with a random resolution
    1..3 per chunk, chunk (1, 1, 0) = [16, 32) x [16, 32) x [0, 16) at 3 and the chunk above it on x at 1; about 500 axis-aligned
    rays from integer points, a third of them aimed at the upper faces of resolution-3 chunks, the LAST one AMBIGUOUS_RAY;
    truth[k] = march_true of ray k."""
    global _lod
    if _lod is not None:
        return _lod
    from python_raytracer_amd import Material
    from python_raytracer_amd.lib import vec3, rgb, material
    from python_raytracer_amd.world import Sprite, Object, build_world
    rng = np.random.default_rng(2024)

    def mat(i):
        return Material(function=material, albedo=rgb(10 + i, 20, 30), roughness=0.1, absorption=1, ior=0, energy=0)

    objs = []
    for k in range(12):
        size = [int(rng.choice([6, 10, 14, 20, 26])) for _ in range(3)]
        if k % 2:
            size[1] = size[2] = size[0]                      # (a quarter turn only applies between equal extents)
        spr = Sprite(size=vec3(*size), frames=1, lod=int(k % 5 == 4))
        m = mat(k)
        n = size[0] * size[1] * size[2]
        vox = {}
        for _ in range(int(0.3 * n)):
            vox[tuple(int(rng.integers(0, s)) for s in size)] = m
        spr.get_frame(0).set_voxels(vox, True)
        half = [s // 2 for s in size]
        pos = [int(rng.integers(h, hi - h)) for h, hi in zip(half, (96, 64, 96))]
        pos[2] = int(rng.integers(32 + half[2], 96 - half[2]))
        ob = Object(pos=vec3(*pos), rot=vec3(*[int(rng.choice([0, 90, 180, 270])) for _ in range(3)]), sprite=spr)
        ob.visible = True
        objs.append(ob)
    shared = mat(40)
    for x in (30, 32):                                       # A, then B: one voxel each, the same material
        spr = Sprite(size=vec3(2, 2, 2), frames=1, lod=0)
        spr.get_frame(0).set_voxels({(0, 0, 0): shared}, True)
        ob = Object(pos=vec3(x + 1, 22, 7), rot=vec3(0, 0, 0), sprite=spr)
        ob.visible = True
        objs.append(ob)
    w = build_world(objs, CS, owners=True)
    assert list(w.origin) == [0, 0, 0] and all(d <= 6 for d in w.dims), (w.origin, w.dims)
    res = rng.integers(1, 4, tuple(w.dims)).astype(np.uint8)
    res[1, 1, 0], res[2, 1, 0] = 3, 1
    grid = ol.Scene.camera_grid(w.grid, w.origin, w.dims, CS, w.present, res)
    sc = ol.Scene(w.origin, w.dims, CS, w.present, res, grid, id_materials(len(w.materials)))
    # rays: integer origins, one axis, +-1, life 40.  A ray whose record two chunks explain is left out: the set is for
    # comparing with the truth, and the one constructed record of that kind comes last
    origins, vels = [], []
    hi = [int(d) * CS for d in w.dims]

    def add(o, v):
        step, pos, m, cell, r, c = march_true(sc, CS // 2, o, v, 40.0)
        if not m or len(counting(sc, pos, m)) == 1:
            origins.append(o)
            vels.append(v)

    while len(origins) < 420:
        o = [int(rng.integers(-4, h + 4)) for h in hi]
        v = [0, 0, 0]
        v[int(rng.integers(0, 3))] = int(rng.choice([-1, 1]))
        add(o, v)
    # ... and towards voxels that a ray of a resolution-3 chunk reads from the chunk's upper face: the last multiple of 3 below
    # a face that is no multiple of 3 itself, from one step (3 cells) before the face
    targets = []
    for cell in np.argwhere((res == 3) & (w.present != 0)):
        cmin = cell * CS
        block = grid[cmin[0]:cmin[0] + CS, cmin[1]:cmin[1] + CS, cmin[2]:cmin[2] + CS]
        for a in range(3):
            face = int(cmin[a]) + CS
            if face % 3:
                for q in np.argwhere(block != 0):
                    if int(q[a] + cmin[a]) == (face // 3) * 3:
                        targets.append((a, face, (q + cmin).tolist()))
    for k in rng.permutation(len(targets))[:170]:
        a, face, c = targets[int(k)]
        o = [int(v + rng.integers(0, 3)) for v in c]         # anywhere in the voxel's cell of 3^3
        o[a] = face - 3
        v = [0, 0, 0]
        v[a] = 1
        add(o, v)
    origins.append(list(AMBIGUOUS_RAY[0]))
    vels.append(list(AMBIGUOUS_RAY[1]))
    origins, vels = np.array(origins, np.float64), np.array(vels, np.float64)
    lives = np.full(len(origins), 40.0)
    lives[-1] = AMBIGUOUS_RAY[2]
    assert not (origins == 0).all(1).any()                   # (a ray that starts at the very origin never re-snaps: init.py:67)
    truth = [march_true(sc, CS // 2, o, v, l) for o, v, l in zip(origins, vels, lives)]
    for a in (origins, vels, lives, w.grid, w.owner, sc.grid, sc.res):
        a.setflags(write=False)
    _lod = dict(objs=objs, world=w, scene=sc, origins=origins, vels=vels, lives=lives, truth=truth)
    return _lod


def host_owner_at(w, c):
    """World.owner at world voxel c."""
    return int(w.owner[c[0] - int(w.origin[0]), c[1] - int(w.origin[1]), c[2] - int(w.origin[2])])


# ---- what the owner pass must report, from the host world ------------------------------------------------------------------
def expect_owners(sc, w, order, hits):
    """vrt_owner records for vrt_hit records `hits` (numpy, cast_ref.HIT_DTYPE) from the restated rule over the camera scene `sc`
    (an oracle_lib.Scene over the host world `w`, built with owners=True from the objects `order`), and the number of records
    that two chunks explain.  A record no candidate explains is an orphan (-2)."""
    from python_raytracer_amd import _native as nat
    from python_raytracer_amd.world import _rotate_index
    exp = np.zeros(len(hits), np.dtype(nat.OWNER_FIELDS))
    exp["object"] = -1
    ambiguous = 0
    for k in np.flatnonzero(hits["material"] > 0):
        got = counting(sc, hits["pos"][k].tolist(), int(hits["material"][k]))
        if not got:
            exp["object"][k] = -2
            continue
        ambiguous += len(got) > 1
        cell, r, c = got[0]
        o = host_owner_at(w, c)
        ob = order[o]
        local = _rotate_index(c[0] - int(ob.mins.x), c[1] - int(ob.mins.y), c[2] - int(ob.mins.z), ob.sprite.size, ob.rot)
        exp[k] = (o, r, c, tuple(int(v) for v in local))
    return exp, ambiguous


def model_material(ob, local, materials):
    """World material id (1 + index in `materials`) of the model voxel `local` of object `ob`, 0 if it holds none."""
    dense, smats = ob.sprite.dense()
    k = int(dense[tuple(int(v) for v in local)])
    return 1 + [id(m) for m in materials].index(id(smats[k - 1])) if k else 0


def shared_voxels(a, b, cs):
    """World voxels [n, 3] at which the objects a and b both have a voxel."""
    from python_raytracer_amd.world import build_world
    wa, wb = build_world([a], cs), build_world([b], cs)
    lo = np.minimum(wa.origin, wb.origin)
    hi = np.maximum(wa.origin + wa.grid.shape, wb.origin + wb.grid.shape)
    both = np.ones(tuple(hi - lo), bool)
    for part in (wa, wb):
        g = np.zeros(tuple(hi - lo), bool)
        o = part.origin - lo
        g[o[0]:o[0] + part.grid.shape[0], o[1]:o[1] + part.grid.shape[1], o[2]:o[2] + part.grid.shape[2]] = part.grid != 0
        both &= g
    return np.argwhere(both) + lo


def casts_at(voxels, box_lo, box_hi, n_random, seed):
    """Rays for a region: one from the centre of each of the 26 neighbours of every voxel of `voxels` into that voxel's centre
    (Chebyshev-unit velocity: it stands there after one step), then n_random rays between random points of the box."""
    rng = np.random.default_rng(seed)
    origins, vels, lives = [], [], []
    for p in np.asarray(voxels):
        for d in np.ndindex(3, 3, 3):
            d = np.array(d) - 1
            if d.any():
                origins.append(p + 0.5 + d)
                vels.append(-d.astype(np.float64))
                lives.append(3.0)
    a = rng.uniform(box_lo, box_hi, (n_random, 3))
    b = rng.uniform(box_lo, box_hi, (n_random, 3))
    d = b - a
    ref = np.abs(d).max(1)
    origins += list(a)
    vels += list(d / ref[:, None])
    lives += list(ref)
    return np.array(origins, np.float64), np.array(vels, np.float64), np.array(lives, np.float64)


_crowd = None


def crowd_world():
    """300 cubes of edge 2 or 4 (a given edge of 3 is rounded up to 4), 70 % full, six materials between them, every quarter
    turn, all inside a box of 40^3 voxels: boxes overlap heavily.  dict(objs, world) -- the host world with its owner grid."""
    global _crowd
    if _crowd is not None:
        return _crowd
    from python_raytracer_amd import Material
    from python_raytracer_amd.lib import vec3, rgb, material
    from python_raytracer_amd.world import Sprite, Object, build_world
    rng = np.random.default_rng(300)
    mats = [Material(function=material, albedo=rgb(10 * i, 20, 30), roughness=0.1, absorption=1, ior=0, energy=0) for i in range(1, 7)]
    objs = []
    for k in range(300):
        e = int(rng.choice([2, 3, 4]))
        spr = Sprite(size=vec3(e, e, e), frames=1, lod=0)
        e = int(spr.size.x)
        vox = {}
        for p in np.ndindex(e, e, e):
            if rng.random() < 0.7:
                vox[p] = mats[int(rng.integers(0, 6))]
        spr.get_frame(0).set_voxels(vox, True)
        ob = Object(pos=vec3(*[int(v) for v in rng.integers(2, 38, 3)]), rot=vec3(*[int(rng.choice([0, 90, 180, 270])) for _ in range(3)]),
                    sprite=spr)
        ob.visible = True
        objs.append(ob)
    w = build_world(objs, CS, owners=True)
    for a in (w.grid, w.owner):
        a.setflags(write=False)
    _crowd = dict(objs=objs, world=w)
    return _crowd
