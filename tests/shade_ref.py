"""References for shaded explicit rays (Camera.shade_rays -> vrt_shade_rays, shade_kernel).

1. The CPU oracle, as tests/cast_ref.py uses it: with dof = 0, pixel (1, 1) of a 2 x 2 window is exactly the ray
   origin = cam.pos + vel * dist_min, vel = cam.rot.vec_forward(), life = dist_max - dist_min.  Here the scene keeps its OWN
   materials and max_bounces is the set's, so the oracle's end state is the whole of Camera.trace.  A non-zero seed_nonce
   gives the ray its own MT19937 stream, seed (1 * 2 + 1) * 1 + 0 + nonce = 3 + nonce; its first draw goes to lod_random
   (init.py:139), the rest are what the loop consumes -- the rows shade_rays is handed.
2. `trace`: a restatement of init.py:66-120, 141 in Python floats over an oracle_lib.Scene, for velocities no quaternion
   yields.  tests/test_shade_host.py pins it to the oracle on the CPU."""
import math

import numpy as np

import cast_ref as cr
import oracle_lib as ol

RAY_DTYPE = ol.RAY_DTYPE
PIXEL = cr.PIXEL
N_DRAWS = 64          # draws per row of the six ordinary sets (the most a ray of them consumes is asserted below it)
C_LOOKUP, C_NBR, C_RESNAP, C_CGET, C_HIT, C_DRAW, C_ADV, C_BROKE = range(8)


def ray_settings(chunk_size, dist_min, dist_max, max_bounces, max_light=1.0, **extra):
    """extra: settings of the oracle's per-ray block that a set changes (falloff, shutter, lod_bounces); the window and the
    ray generation (width, height, samples, dof, lod_samples, lod_random, lod_edge) stay what makes pixel (1, 1) the ray."""
    assert set(extra) <= {"falloff", "shutter", "lod_bounces"}, extra
    return ol.make_settings(**dict(dict(width=2, height=2, samples=1, chunk_size=chunk_size, dof=0.0, lod_samples=0.0,
                                        lod_random=0.0, lod_edge=0.0, max_bounces=float(max_bounces), max_light=float(max_light),
                                        dist_min=dist_min, dist_max=dist_max), **extra))


def shade_settings(chunk_size, max_bounces, max_light=1.0, **kw):
    """The settings dict of a camera that shades a set's rays: what vrt_shade_rays reads of it is the oracle's per-ray block
    (chunk size and radius, shutter, falloff, max_light, max_bounces, lod_bounces); the window is the camera's own business."""
    return ol.make_settings(**dict(dict(width=32, height=24, samples=4, chunk_size=chunk_size, max_bounces=float(max_bounces),
                                        max_light=float(max_light), dist_max=192), **kw))


def packed(rec):
    """r | g << 8 | b << 16 | alpha << 24 of vrt_ray records; 0 for the markers (s < 0)."""
    c = rec["color"].astype(np.uint32)
    out = c[:, 0] | (c[:, 1] << 8) | (c[:, 2] << 16) | (rec["alpha"].astype(np.uint32) << 24)
    return np.where(rec["s"] < 0, np.uint32(0), out).astype(np.uint32)


def assert_records_equal(got, exp):
    """Bit for bit, field by field (the doubles as their 64-bit patterns)."""
    assert got.shape == exp.shape
    for f in ("x", "y", "s", "color", "alpha", "ntrav", "counters"):
        assert np.array_equal(got[f], exp[f]), (f, np.nonzero((got[f] != exp[f]).reshape(len(got), -1).any(1))[0][:8])
    for f in ("detail", "energy", "step", "life", "bounces", "pos", "vel"):
        a, b = np.ascontiguousarray(got[f]).view(np.uint64), np.ascontiguousarray(exp[f]).view(np.uint64)
        assert np.array_equal(a, b), (f, np.nonzero((a != b).reshape(len(got), -1).any(1))[0][:8])


def stats_of(exp):
    """What d_stats[0..10] must hold for these expected records: event sums over the completed rays, then completed,
    rejected and exhausted rays."""
    done = exp["s"] == 0
    return np.concatenate([exp["counters"][done].sum(0).astype(np.int64),
                           [int(done.sum()), int((exp["s"] == -2).sum()), int((exp["s"] == -3).sum())]])


def marker(s):
    rec = np.zeros(1, RAY_DTYPE)
    rec["s"] = s
    return rec[0]


def oracle_shade(sc, cam_pos, quats, lives, nonces, max_bounces, has_background, max_light=1.0, dist_min=0, n_draws=N_DRAWS,
                 **extra):
    """One oracle call per ray.  Returns (origins [n, 3], vels [n, 3], lives [n], draws [n, n_draws], expected vrt_ray records
    [n], the rays' traversed lists): the rays as shade_rays takes them and what it must give.  The oracle's record becomes
    the expected one with x = y = s = 0, detail = 1 and the draw counter less the lod_random draw.
    n_draws: the width of a row; None sizes it from the oracle's own draw counters -- the most draws a ray of the set
    consumes in its loop, at least 1.  Either way no ray may need more than its row holds (asserted).
    extra: what ray_settings takes besides (falloff, shutter, lod_bounces)."""
    cam_pos = np.asarray(cam_pos, np.float64).reshape(-1, 3)
    quats = np.asarray(quats, np.float64).reshape(-1, 4)
    lives = np.asarray(lives, np.float64).reshape(-1)
    n = len(cam_pos)
    vels = cr.vec_forward(quats)
    origins = cam_pos + vels * float(dist_min)
    out_lives = (float(dist_min) + lives) - float(dist_min)      # init.py:56 with detail = 1
    exp = np.zeros(n, RAY_DTYPE)
    trav = []
    for k in range(n):
        st = ray_settings(sc.chunk_size, float(dist_min), float(dist_min) + float(lives[k]), max_bounces, max_light, **extra)
        o = ol.render(sc, st, cam_pos[k], quats[k], st["fov"] * np.pi / 8, PIXEL, libm=ol.LIBM_PORTABLE,
                      has_background=has_background, seed_nonce=int(nonces[k]), want_traversed=True, trav_cap=4096)
        assert len(o["rays"]) == 1
        r = o["rays"][0].copy()
        assert (r["x"], r["y"], r["s"], r["detail"]) == (1, 1, 0, 1.0)
        if int(r["counters"][C_HIT]) == 0:
            assert r["step"] >= r["life"] and r["bounces"] == 0
            assert np.array_equal(r["vel"].view(np.uint64), vels[k].view(np.uint64)), (k, r["vel"], vels[k])
            assert r["life"] == out_lives[k], (k, r["life"], out_lives[k])
        assert 1 <= int(r["counters"][C_DRAW])                   # the lod_random draw, then the loop's
        r["counters"][C_DRAW] -= 1
        r["x"] = r["y"] = r["s"] = 0
        r["detail"] = 1.0
        exp[k] = r
        assert int(r["ntrav"]) == len(o["traversed"])
        trav.append(np.asarray(o["traversed"], np.int64).reshape(-1, 3))
    most = int(exp["counters"][:, C_DRAW].max(initial=0))
    if n_draws is None:
        n_draws = max(1, most)
    assert most <= n_draws, (most, n_draws)                      # no ray runs out of draws
    draws = np.zeros((n, n_draws))
    for k in range(n):
        draws[k] = ol.rng_draws(3 + int(nonces[k]), 1 + n_draws)[1:]
    return origins, vels, out_lives, draws, exp, trav


# ---- the restatement ---------------------------------------------------------------------------------------------------
def _lookup(sc, cell, cmin, f):
    res = int(sc.res[cell])
    cs = sc.chunk_size
    q = [(v // res) * res for v in f] if res > 1 else list(f)
    if not all(int(c) <= v < int(c) + cs for v, c in zip(q, cmin)):
        return 0
    return int(sc.grid[q[0] - int(sc.origin[0]), q[1] - int(sc.origin[1]), q[2] - int(sc.origin[2])])


def _chunk(sc, cmin):
    cs = sc.chunk_size
    cell = tuple((int(c) - int(o)) // cs for c, o in zip(cmin, sc.origin))
    return cell if all(0 <= i < int(d) for i, d in zip(cell, sc.dims)) and sc.present[cell] else None


def _pow(x, y):
    return float(ol.lib().orc_pow(ol.LIBM_PORTABLE, float(x), float(y)))


def _mix_rgb(col, other, b1):
    b2 = 1 - b1
    return [int(round(float(c) * b2 + float(o) * b1)) for c, o in zip(col, other)]


def trace(sc, settings, origin, vel, life, draws, has_background=True, visits=None):
    """init.py:66-120 and tile()'s alpha (init.py:141) for one ray over an oracle_lib.Scene, in Python floats, from the
    state pos = origin, vel = vel, life = life; the k-th lib.rand draw is draws[k].  Returns (vrt_ray record, traversed
    list); the record's s is -3 -- every other field 0 -- when the ray needs more draws than it was given.  visits: a list
    that receives the chunk of EVERY re-snap, repeats included (what a traversed box counts when the chunk lies outside it)."""
    cs = sc.chunk_size
    radius = settings["chunk_radius"]
    pos = [float(v) for v in origin]
    vel = [float(v) for v in vel]
    life = float(life)
    step = bounces = energy = 0.0
    color = [0, 0, 0]
    cnt = [0] * 8
    trav = []
    cmin = cmax = (0.0, 0.0, 0.0)
    chunk = None
    broke = 0
    pow_y = 1 + settings["falloff"]
    while step < life:
        if not all(p >= c for p, c in zip(pos, cmin)) or not all(p <= c for p, c in zip(pos, cmax)):
            cmin = tuple((p // cs) * cs for p in pos)
            cmax = tuple(c + cs for c in cmin)
            chunk = _chunk(sc, cmin)
            key = tuple(int(c) for c in cmin)
            if key not in trav:
                trav.append(key)
            if visits is not None:
                visits.append(key)
            cnt[C_RESNAP] += 1
        broke = 0
        if chunk is not None:
            mat_id = _lookup(sc, chunk, cmin, [math.floor(p) for p in pos])
            cnt[C_LOOKUP] += 1
            if mat_id:
                m = sc.materials[mat_id - 1]
                rough, absorb, ior, emit = float(m[3]), float(m[4]), float(m[5]), float(m[6])
                # lib.material (lib.py:448-460)
                a = absorb / _pow(1 + bounces, pow_y)
                if not a < 1:
                    a = 1
                color = _mix_rgb(color, m[:3], a)
                energy = energy * (1 - a) + emit * a
                life *= 1 - (rough * a)
                if rough != 0.0:
                    if cnt[C_DRAW] + 3 > len(draws):
                        return marker(-3), trav
                    for ax in range(3):
                        vel[ax] += (-1 + float(draws[cnt[C_DRAW] + ax]) * 2) * rough
                    cnt[C_DRAW] += 3
                cnt[C_HIT] += 1
                broke = 1
                bounces += absorb
                life /= float(int(sc.res[chunk])) + absorb * settings["lod_bounces"]
                ref = max(abs(vel[0]), abs(vel[1]), abs(vel[2]))
                if ref != 0.0 and ref != 1.0:
                    vel = [v / ref for v in vel]
                if step >= life or energy >= settings["max_light"] or bounces >= settings["max_bounces"] + 1:
                    break
                if ior != 0.0:
                    direction = (ior - 0.5) * 2
                    solid = []
                    for ax in range(3):
                        npos = list(pos)
                        npos[ax] = pos[ax] + 1 if vel[ax] < direction else pos[ax] - 1
                        if all(p >= c for p, c in zip(npos, cmin)) and all(p <= c for p, c in zip(npos, cmax)):
                            nchunk, ncmin = chunk, cmin
                        else:
                            ncmin = tuple((p // cs) * cs for p in npos)
                            nchunk = _chunk(sc, ncmin)
                            cnt[C_CGET] += 1
                        nid = 0
                        if nchunk is not None:
                            nid = _lookup(sc, nchunk, ncmin, [math.floor(p) for p in npos])
                            cnt[C_NBR] += 1
                        solid.append(bool(nid) and float(sc.materials[nid - 1][5]) == ior)
                    for ax in range(3):
                        if not solid[ax]:
                            vel[ax] -= vel[ax] * ior * 2
        if chunk is not None:
            size = float(int(sc.res[chunk]) if int(sc.res[chunk]) else 1)
        else:
            size = 1 + abs(radius - (min(pos) + radius) % cs)
        step += size
        pos = [p + v * size for p, v in zip(pos, vel)]
        cnt[C_ADV] += 1
        broke = 0
    cnt[C_BROKE] = broke
    if has_background:      # lib.material_background (lib.py:463-476)
        a = 1 / _pow(1 + bounces, pow_y)
        if not a < 1:
            a = 1
        up = vel[1] if vel[1] > 0 else 0
        color = _mix_rgb(color, [127, 127 + up * 64, 127 + up * 128], a)
        energy = energy * (1 - a) + (1 + up) * a
        color = [min(255, int(round(float(c) * energy))) for c in color]
    rec = np.zeros(1, RAY_DTYPE)[0]
    rec["color"] = color
    rec["alpha"] = int(round(min(1, energy + settings["shutter"]) * 255))
    rec["ntrav"] = len(trav)
    rec["counters"] = cnt
    rec["detail"], rec["energy"], rec["step"], rec["life"], rec["bounces"] = 1.0, energy, step, life, bounces
    rec["pos"], rec["vel"] = pos, vel
    return rec, trav


def trace_records(sc, settings, origins, vels, lives, draws, has_background=True):
    """`trace` for a set of rays: (vrt_ray records, the rays' traversed lists)."""
    exp = np.zeros(len(origins), RAY_DTYPE)
    trav = []
    for k in range(len(origins)):
        exp[k], t = trace(sc, settings, origins[k], vels[k], lives[k], draws[k] if draws is not None else (), has_background)
        trav.append(np.asarray(t, np.int64).reshape(-1, 3))
    return exp, trav


def union_in_order(travs):
    """The order-preserving union of per-ray traversed lists in ray order (lib.py:404-409): [m, 3] chunk positions."""
    seen, out = set(), []
    for t in travs:
        for p in t:
            key = tuple(int(v) for v in p)
            if key not in seen:
                seen.add(key)
                out.append(key)
    return np.array(out, np.int64).reshape(-1, 3)


# ---- the ray sets of the oracle comparisons: computed once, shared by the CPU and the GPU tests, never changed ----------------
def varied_materials(n, seed):
    """n materials with roughness, ior and energy varied -- the id-materials of the cast tests end every ray at its first
    voxel --: absorption 0.25 .. 1 so that rays go on after a hit, two in five rough, ior in steps of 0.25, one in four emits."""
    rng = np.random.default_rng(seed)
    m = np.zeros((n, 7))
    m[:, :3] = rng.integers(20, 256, (n, 3))
    m[:, 3] = np.resize([0.0, 0.25, 0.0, 0.5, 0.0], n)
    m[:, 4] = np.resize([0.25, 0.5, 0.25, 1.0], n)
    m[:, 5] = np.resize([0.5, 0.0, 0.25, 0.75, 1.0, 0.5], n)
    m[:, 6] = np.resize([0.0, 0.0, 0.0, 0.4], n)
    return m


def with_materials(sc, mats):
    return ol.Scene(sc.origin, sc.dims, sc.chunk_size, sc.present, sc.res, sc.grid, mats)


SETS = {
    # name: (max_bounces, has_background)
    "default_mb2": (2.0, True),
    "default_mb8": (8.0, True),
    "default_scaled_nobg": (8.0, False),
    "synth64_mb4": (4.0, True),
    "hand": (6.0, True),
    "big_table": (6.0, True),
}
N_RAYS = 600
_sets = {}


def ray_set(name):
    """(scene, settings, has_background, origins, vels, lives, draws, expected records, traversed lists) of a named oracle
    comparison: 600 rays each, nonce 1000 + k.
    default_mb2 / default_mb8 / default_scaled_nobg: the default scene (resolutions 1 and 2, missing chunks), origins uniform in
    [-64, -32, -64] .. [64, 40, 64], unit quaternions from normalised Gaussians (norms 0.5 .. 1.5 for the scaled set, which has
    no background), lives 16 .. 192;  synth64_mb4: origins in +-40, lives 8 .. 96;  hand / big_table: test_gpu_first_hit's
    hand_scene() (resolutions 1, 2, 3) and big_table_scene() (4 352 table cells, read from memory) with varied_materials."""
    if name in _sets:
        return _sets[name]
    max_bounces, has_bg = SETS[name]
    rng = np.random.default_rng(11)
    n = N_RAYS
    if name.startswith("default"):
        sc = ol.default_scene()
        pos = rng.uniform([-64, -32, -64], [64, 40, 64], (n, 3))
        q = cr.unit_quats(rng, n)
        lives = rng.uniform(16, 192, n)
        if name == "default_scaled_nobg":
            q = q * rng.uniform(0.5, 1.5, (n, 1))
    elif name == "synth64_mb4":
        sc = ol.synth64_scene()
        pos = rng.uniform(-40, 40, (n, 3))
        q = cr.unit_quats(rng, n)
        lives = rng.uniform(8, 96, n)
    elif name == "hand":
        from test_gpu_first_hit import hand_scene
        sc = with_materials(hand_scene(), varied_materials(5, 21))
        # origins within 6 cells of the centre of one of the four chunks (8^3 each, holes between them): inside it or just
        # outside.  Uniform over the box of 4 x 3 x 2 chunks only 22 % of the rays hit anything
        centres = np.array([[-12, 4, 4], [12, 4, 12], [-4, 12, 12], [4, -4, 4]], np.float64)
        pos = centres[rng.integers(0, 4, n)] + rng.uniform(-6, 6, (n, 3))
        q = cr.unit_quats(rng, n)
        lives = rng.uniform(8, 64, n)
    elif name == "big_table":
        from test_gpu_first_hit import big_table_scene
        sc = with_materials(big_table_scene(), varied_materials(5, 22))
        pos = rng.uniform(-50, 50, (n, 3))
        q = cr.unit_quats(rng, n)
        lives = rng.uniform(48, 160, n)
    else:
        raise KeyError(name)
    st = shade_settings(sc.chunk_size, max_bounces)
    nonces = 1000 + np.arange(n)
    origins, vels, lives, draws, exp, trav = oracle_shade(sc, pos, q, lives, nonces, max_bounces, has_bg)
    for a in (origins, vels, lives, draws, exp):
        a.setflags(write=False)
    _sets[name] = (sc, st, has_bg, origins, vels, lives, draws, exp, trav)
    return _sets[name]
