"""Shaded explicit rays (Camera.shade_rays -> vrt_shade_rays, shade_kernel): colour and end state along any origin and
velocity, bit for bit against the CPU oracle where the oracle can express the ray (tests/shade_ref.py: one 2 x 2 frame per
ray, its own MT19937 stream per ray) and against the Python restatement of Camera.trace's loop -- pinned to the oracle in
tests/test_shade_host.py, which also asserts that no ray set is vacuous -- where it cannot.  Doubles are compared as bit
patterns."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import cast_ref as cr
import oracle_lib as ol
import shade_ref as sr
from gpu_util import camera_for, launches_of, settings_store
from python_raytracer_amd import _native as nat
from python_raytracer_amd import data

gpu = pytest.mark.gpu

IDENTITY = (0.0, 0.0, 0.0, 1.0)
_cams = {}
# the instance a call runs, by the highest resolution of the scene's chunks and by whether it keeps records: what the launch
# census must show for a shade_rays call
SHADE_INSTANCE = {(1, True): 'shade_kernel<8,0,true>', (2, True): 'shade_kernel<8,1,true>', (3, True): 'shade_kernel<4,2,true>',
                  (1, False): 'shade_kernel<8,0,false>', (2, False): 'shade_kernel<8,1,false>', (3, False): 'shade_kernel<4,2,false>'}
RES_MAX = {"default_mb2": 2, "default_mb8": 2, "default_scaled_nobg": 2, "synth64_mb4": 1, "hand": 3, "big_table": 1}


@contextlib.contextmanager
def background(on):
    """data.background as the set wants it (the camera asks for it at every call)."""
    saved = data.background
    if not on:
        data.background = None
    try:
        yield
    finally:
        data.background = saved


def cam_for(sc, st, key):
    """A camera over `sc` with its own materials and the settings dict `st` (its pose plays no part in shade_rays)."""
    if key not in _cams:
        _cams[key] = camera_for(sc, settings_store(st), (0.0, 0.0, 0.0), IDENTITY, st["fov"] * np.pi / 8,
                                grid=getattr(sc, "grid_lod0", None))
    return _cams[key]


def cam_of(name):
    sc, st = sr.ray_set(name)[:2]
    return cam_for(sc, st, name)


def rgba_of(res):
    return res.rgba.cpu().numpy().view(np.uint32)


def check_result(res, exp):
    sr.assert_records_equal(res.numpy(), exp)
    assert np.array_equal(rgba_of(res), sr.packed(exp))
    assert np.array_equal(res.stats[:11], sr.stats_of(exp)), (res.stats, sr.stats_of(exp))
    assert (res.stats[12:] == 0).all(), res.stats
    assert np.array_equal(res.rejected_mask().cpu().numpy(), exp["s"] == -2)
    assert np.array_equal(res.exhausted_mask().cpu().numpy(), exp["s"] == -3)


def default_cam(max_bounces=8.0, **kw):
    sc = ol.default_scene()
    st = sr.shade_settings(sc.chunk_size, max_bounces, **kw)
    return cam_for(sc, st, ("default", max_bounces, tuple(sorted(kw.items())))), sc, st


# ---- 1. oracle parity ------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", ["default_mb2", "default_mb8", "default_scaled_nobg", "synth64_mb4", "hand", "big_table"])
def test_against_the_oracle(name):
    """The default scene (resolutions 1 and 2, missing chunks) at max_bounces 2 and 8 and, with quaternions of norm 0.5 .. 1.5
    (|vel| varies), without a background; synth64 (an identity table: entries computed, not read); the hand scene (resolutions
    1, 2 and 3: the generic instance) and 4 352 table cells (read from memory): records, colours and statistics, then the
    same colours without records."""
    sc, st, has_bg, origins, vels, lives, draws, exp, trav = sr.ray_set(name)
    cam = cam_of(name)
    with background(has_bg):
        res, ran = launches_of(lambda: cam.shade_rays(origins, vels, lives, draws=draws))
        assert ran == {SHADE_INSTANCE[RES_MAX[name], True]}, (name, ran)   # the instance the set is there for, and no other
        check_result(res, exp)
        assert int(res.stats[11]) == 0
        lean, ran = launches_of(lambda: cam.shade_rays(origins, vels, lives, draws=draws, want_records=False))
        assert ran == {SHADE_INSTANCE[RES_MAX[name], False]}, (name, ran)
        assert lean.records is None and np.array_equal(rgba_of(lean), sr.packed(exp))
        assert np.array_equal(lean.stats[:11], sr.stats_of(exp))
        with pytest.raises(ValueError, match="records"):
            lean.exhausted_mask()
    c = cam._c_scene(cam._ensure_scene())
    assert int(c.max_resolution) == RES_MAX[name]
    if name == "big_table":
        assert int(np.prod(sc.dims)) == 4352 > 4096 and not (int(c.flags) & nat.SCENE_TABLE_IS_IDENTITY)
    if name == "synth64_mb4":
        assert int(c.flags) & nat.SCENE_TABLE_IS_IDENTITY


# ---- 2. arbitrary velocities against the restatement -----------------------------------------------------------------
@gpu
def test_arbitrary_velocities_against_the_restatement():
    cam, sc, st = default_cam(8.0)
    rng = np.random.default_rng(31)
    o, v, l = [], [], []

    def add(origin, vel, life):
        o.append(np.asarray(origin, np.float64)), v.append(np.asarray(vel, np.float64)), l.append(float(life))

    for axis in range(3):                                   # axis-parallel, from integer origins and chunk corners
        for sign in (1.0, -1.0):
            for start in rng.integers(-40, 40, (4, 3)):
                vel = [0.0, 0.0, 0.0]
                vel[axis] = sign
                add(start.astype(float), vel, 96.0)
                add((start // 16 * 16).astype(float), vel, 96.0)
    for k in range(80):                                     # Chebyshev-normalised, some with zero and -0.0 components
        d = rng.normal(size=3)
        d = d / np.abs(d).max()
        if k % 4 == 0:
            d[rng.integers(3)] = 0.0
        if k % 4 == 1:
            d[rng.integers(3)] = -0.0
        add(rng.uniform([-50, -20, -50], [50, 30, 50]), d, rng.uniform(16, 128))
    for k in range(40):                                     # any length
        add(rng.uniform([-50, -20, -50], [50, 30, 50]), rng.normal(size=3) * rng.choice([0.05, 0.5, 2.0]), rng.uniform(16, 128))
    add([3.5, 20.25, -7.0], [3.5, -0.75, 0.5], 64.0)        # |vel|_inf = 3.5
    add([-20.0, 10.0, 5.5], [0.25, -0.5, 1.75], 64.0)       # vel.z > 1
    add([0.0, 0.0, 0.0], [0.5, -1.0, 0.25], 64.0)           # from the origin exactly
    for life in (0.0, -1.0, -0.0):                          # no loop at all: with a background the colour is the sky's
        add(rng.uniform(-30, 30, 3), [0.5, 1.0, -0.25], life)
        add(rng.uniform(-30, 30, 3), [0.5, -1.0, -0.25], life)
    while len(o) < 200:
        d = rng.normal(size=3)
        add(rng.uniform([-50, -20, -50], [50, 30, 50]), d / np.abs(d).max(), 0.5 if len(o) % 2 else 160.0)
    o, v, l = np.array(o), np.array(v), np.array(l)
    assert len(o) == 200 and (np.abs(v).max(1) == 3.5).any() and (v[:, 2] > 1).any()
    draws = np.stack([ol.rng_draws(7000 + k, sr.N_DRAWS) for k in range(200)])
    exp, _ = sr.trace_records(sc, st, o, v, l, draws, True)
    assert (exp["s"] == 0).all() and (exp["counters"][:, sr.C_HIT] >= 2).mean() > 0.15
    res = cam.shade_rays(o, v, l, draws=draws, max_life=160.0)
    check_result(res, exp)
    never = l <= 0
    assert never.sum() == 6 and (exp["step"][never] == 0).all() and (exp["counters"][never][:, :5] == 0).all()
    up = np.maximum(v[never][:, 1], 0)                      # lib.material_background on the start state
    sky = np.stack([np.full(6, 127.0), 127 + up * 64, 127 + up * 128], 1)
    assert np.array_equal(exp["color"][never], np.minimum(255, np.rint(np.rint(sky) * (1 + up)[:, None])).astype(np.int32))
    assert len(set(map(tuple, exp["color"][never].tolist()))) == 2


# ---- 3. sizes and order ----------------------------------------------------------------------------------------------
@gpu
def test_sizes_and_order():
    import torch
    o8, v8, l8, d8, e8 = sr.ray_set("default_mb8")[3:8]
    cam = cam_of("default_mb8")
    # 1 199 rays: default_mb8's 600 and its first 599 again, in another order
    idx = np.concatenate([np.arange(600), np.arange(599)[::-1]])
    origins, vels, lives, draws, exp = o8[idx], v8[idx], l8[idx], d8[idx], e8[idx]
    for n in (1, 63, 64, 65, 1199):
        check_result(cam.shade_rays(origins[:n], vels[:n], lives[:n], draws=draws[:n]), exp[:n])
    perm = np.random.default_rng(12).permutation(1199)
    check_result(cam.shade_rays(origins[perm], vels[perm], lives[perm], draws=draws[perm]), exp[perm])
    # ready records, torch tensors, mixed inputs
    rec = np.zeros((1199, 8))
    rec[:, 0:3], rec[:, 3:6], rec[:, 6], rec[:, 7] = origins, vels, lives, 123.0
    drec = torch.from_numpy(rec).cuda()
    check_result(cam.shade_rays(drec, draws=torch.from_numpy(draws).cuda()), exp)
    check_result(cam.shade_rays(torch.from_numpy(origins[:70]), torch.from_numpy(vels[:70]).cuda(), lives[:70],
                                draws=draws[:70].astype(np.float64)), exp[:70])
    # n = 0 through the ABI: the statistics are zeroed and nothing else happens
    stats = torch.full((nat.NSTATS,), 7, dtype=torch.int64, device="cuda")
    ws = torch.zeros(8192, dtype=torch.uint8, device="cuda")
    st, csc = cam._c_settings(0), cam._c_scene(cam._ensure_scene())
    assert nat.lib().vrt_shade_rays(C.byref(csc), C.byref(st), None, 0, 64.0, None, 0, ws.data_ptr(), ws.numel(), None, None,
                                    stats.data_ptr(), None, None) == 0
    torch.cuda.synchronize()
    assert (stats.cpu().numpy() == 0).all()
    # the host-side checks
    o5, v5, l5, d5 = origins[:5], vels[:5], lives[:5], draws[:5]
    for bad in (lambda: cam.shade_rays(origins[:0], vels[:0]), lambda: cam.shade_rays(o5, vels[:4]),
                lambda: cam.shade_rays(o5[:, :2], v5), lambda: cam.shade_rays(o5, v5, lives[:4]),
                lambda: cam.shade_rays(o5, v5, l5, seeds=np.arange(5), draws=d5), lambda: cam.shade_rays(o5, v5, l5, draws=draws[:4]),
                lambda: cam.shade_rays(o5, v5, l5, draws=d5[:, 0]), lambda: cam.shade_rays(o5, v5, l5, draws=d5, n_draws=32),
                lambda: cam.shade_rays(o5, v5, l5, seeds=np.arange(4)), lambda: cam.shade_rays(o5, v5, l5, seeds=np.arange(5), n_draws=1),
                lambda: cam.shade_rays(o5, v5, l5, seeds=np.arange(5) * 0.5), lambda: cam.shade_rays(o5, v5, l5, seeds=-np.arange(5)),
                lambda: cam.shade_rays(o5, v5, l5, max_life=0.0), lambda: cam.shade_rays(drec.float()),
                lambda: cam.shade_rays(drec.cpu()), lambda: cam.shade_rays(drec[:, :7]),
                lambda: cam.shade_rays(o5, v5, l5, want_traversed=([1, 0, 0], [4, 4, 4]))):
        with pytest.raises(ValueError):
            bad()
    # an image from H * W rays in row-major order
    res = cam.shade_rays(origins[:24], vels[:24], lives[:24], draws=draws[:24])
    img = res.image(4, 6).cpu().numpy()
    assert img.shape == (4, 6, 4) and img.dtype == np.uint8
    assert np.array_equal(img.reshape(24, 4), np.concatenate([exp["color"][:24], exp["alpha"][:24, None]], 1).astype(np.uint8))
    with pytest.raises(ValueError):
        res.image(5, 5)


# ---- 4. the same rays as the camera ----------------------------------------------------------------------------------
@gpu
def test_same_rays_as_the_camera():
    """A frame at 32 x 24 x 4 with dof != 0 on the raised default camera: the cached per-slot ray table (lens quaternion,
    life) and draw table read back, the plan's seed index; vel and origin formed in numpy in the reference's operation order
    (lib.py:353-358, 372-376; init.py:54); draws[k] is the slot's row from index 1 + 2 on (the lod_random draw and the two
    lens draws came first).  Every used slot then equals the frame's sample."""
    from test_gpu_first_hit import case1
    cam, st, h, exp = case1(False)
    assert st["dof"] != 0
    r = cam.render(0, want_ray_rgba=True, want_rays=True)
    dp = cam._pixels_tensor(0, None)
    slots = len(exp)
    tab = dp.ray_table.cpu().numpy().view(np.float64).reshape(-1, 8)[:slots]
    used = tab[:, 4] >= 0
    assert 0 < (~used).sum() < used.sum()
    rows = dp.draw_table.cpu().numpy().view(np.float64).reshape(dp.n_distinct, -1)
    raw = dp.plan.cpu().numpy()
    off = 64 + ((4 * slots + 255) // 256) * 256
    seedidx = raw[off:off + 4 * slots].view(np.uint32)
    assert (seedidx[used] < dp.n_distinct).all() and rows.shape[1] in (32, 64)
    ox, oy, oz, ow = (tab[used, i] for i in range(4))
    x, y, z, w = (float(v) for v in (cam.rot.x, cam.rot.y, cam.rot.z, cam.rot.w))
    q = np.stack([w * ox + z * oy - y * oz + x * ow, z * ox + w * oy + x * oz + y * ow, y * ox - x * oy + w * oz + z * ow,
                  x * ox - y * oy - z * oz + w * ow], -1)
    vel = cr.vec_forward(q)
    pos = np.array([float(cam.pos.x), float(cam.pos.y), float(cam.pos.z)])
    origins = pos + vel * float(st["dist_min"])
    draws = np.ascontiguousarray(rows[seedidx[used]][:, 3:])
    res = cam.shade_rays(origins, vel, tab[used, 4], draws=draws, max_life=float(st["dist_max"]))
    got, frame = res.numpy(), r.rays[used]
    assert (got["s"] == 0).all() and (frame["s"] >= 0).all() and len(got) == used.sum()
    for f in ("color", "alpha"):
        assert np.array_equal(got[f], frame[f]), f
    for f in ("energy", "step", "life", "bounces", "pos", "vel"):
        assert np.array_equal(np.ascontiguousarray(got[f]).view(np.uint64), np.ascontiguousarray(frame[f]).view(np.uint64)), f
    shift = np.zeros(8, np.int32)
    shift[sr.C_DRAW] = 3
    assert np.array_equal(got["counters"] + shift, frame["counters"])
    assert np.array_equal(rgba_of(res), r.ray_rgba.cpu().numpy().view(np.uint32)[used])
    assert (got["counters"][:, sr.C_HIT] >= 2).mean() > 0.1      # (42 % of this frame's rays hit twice; none meets a rough material)


# ---- 5. draws --------------------------------------------------------------------------------------------------------
@gpu
def test_draws():
    sc, st, has_bg, origins, vels, lives, draws, exp, trav = sr.ray_set("default_mb8")
    cam = cam_of("default_mb8")
    # seeds: random.seed(seed), then random.random() repeatedly -- made on the device
    seeds = 5000 + 3 * np.arange(600)
    rows = np.stack([ol.rng_draws(int(s), 32) for s in seeds])
    a = cam.shade_rays(origins, vels, lives, seeds=seeds)
    b = cam.shade_rays(origins, vels, lives, draws=rows)
    assert (b.numpy()["s"] == 0).all() and b.numpy()["counters"][:, sr.C_DRAW].max() >= 12
    sr.assert_records_equal(a.numpy(), b.numpy())
    assert np.array_equal(rgba_of(a), rgba_of(b)) and np.array_equal(a.stats, b.stats)
    import torch
    c = cam.shade_rays(origins, vels, lives, seeds=torch.from_numpy(seeds).cuda(), n_draws=40)
    sr.assert_records_equal(c.numpy(), b.numpy())
    # two draws a row: a ray is not completed at its first rough hit
    out = exp["counters"][:, sr.C_DRAW] > 2
    assert 0.2 < out.mean() < 0.8
    want = exp.copy()
    want[out] = sr.marker(-3)
    res = cam.shade_rays(origins, vels, lives, draws=draws[:, :2], n_draws=2)
    check_result(res, want)
    assert int(res.stats[10]) == int(out.sum()) and int(res.stats[8]) == int((~out).sum())
    assert (rgba_of(res)[out] == 0).all()
    # ... and the marked ones repeated with longer rows give the rest
    again = np.nonzero(res.exhausted_mask().cpu().numpy())[0]
    check_result(cam.shade_rays(origins[again], vels[again], lives[again], draws=draws[again]), exp[again])
    # no draws at all over materials without roughness: every ray is completed
    smooth = sr.with_materials(sc, np.where(np.arange(7) == 3, 0.0, sc.materials))
    smooth.grid_lod0 = sc.grid_lod0
    cam0 = cam_for(smooth, st, "default_smooth")
    e0, _ = sr.trace_records(smooth, st, origins[:300], vels[:300], lives[:300], None, True)
    assert (e0["s"] == 0).all() and (e0["counters"][:, sr.C_DRAW] == 0).all() and (e0["counters"][:, sr.C_HIT] >= 2).mean() > 0.2
    check_result(cam0.shade_rays(origins[:300], vels[:300], lives[:300]), e0)
    # ... and over the scene's own a rough hit runs out at once
    none = cam.shade_rays(origins, vels, lives)
    assert np.array_equal(none.exhausted_mask().cpu().numpy(), exp["counters"][:, sr.C_DRAW] > 0)


# ---- 6. rejection ----------------------------------------------------------------------------------------------------
@gpu
def test_bad_rays_are_rejected_and_reported():
    sc, st, has_bg, origins, vels, lives, draws, exp, trav = sr.ray_set("default_mb2")
    cam = cam_of("default_mb2")
    keep = np.nonzero(lives <= 64.0)[0][:100]                # (the table's max_life is 64)
    assert len(keep) == 100
    origins, vels, lives, draws, exp = origins[keep], vels[keep], lives[keep], draws[keep], exp[keep]
    big = float(1 << 28)
    nan, inf = float("nan"), float("inf")
    bad = [([nan, 0, 0], [1, 0, 0], 10),                 # origin not finite
           ([0, 0, 0], [0, inf, 0], 10),                 # velocity not finite
           ([1, 2, 3], [1, 0, 0], 64.5),                 # life > max_life
           ([0, big, 0], [0, 0, 1], 10),                 # origin at 2^28
           ([1, 2, 3], [0, 0, -float(1 << 26)], 1),      # |vel| = 2^26
           ([big - 90, 0, 0], [-1, 0.5, 0], 64),         # reach: 2^28 - 90 + (64 + 2 * 16 + 2) * 1 = 2^28 + 8
           ([1, 2, 3], [1, 0, 0], nan),                  # life not finite
           ([1, 2, 3], [0.5, -nan, 0], 10)]              # a NaN that fmax would drop
    at = [0, 1, 63, 64, 70, 90, 100, 107]                # where the bad ones sit in the 108
    o8, v8, l8, d8, e8 = np.zeros((108, 3)), np.zeros((108, 3)), np.zeros(108), np.zeros((108, sr.N_DRAWS)), np.zeros(108, sr.RAY_DTYPE)
    good = np.setdiff1d(np.arange(108), at)
    o8[good], v8[good], l8[good], d8[good], e8[good] = origins, vels, lives, draws, exp
    for i, (bo, bv, bl) in zip(at, bad):
        o8[i], v8[i], l8[i] = bo, bv, bl
        e8[i] = sr.marker(-2)
    res = cam.shade_rays(o8, v8, l8, draws=d8, max_life=64.0)
    check_result(res, e8)
    assert int(res.stats[9]) == 8 and int(res.stats[8]) == 100 and (rgba_of(res)[at] == 0).all()
    assert np.array_equal(np.nonzero(res.rejected_mask().cpu().numpy())[0], at)
    lean = cam.shade_rays(o8, v8, l8, draws=d8, max_life=64.0, want_records=False)
    assert np.array_equal(rgba_of(lean), sr.packed(e8)) and int(lean.stats[9]) == 8
    # just inside the range rule: accepted, and marched like any other ray (2^28 - 100 + 98 < 2^28)
    o2, v2, l2 = np.array([[big - 100, 0, 0], [0, -(big - 100), 0.5]]), np.array([[-1, 0.5, 0], [0, 1, 0]]), np.array([64.0, 64.0])
    e2, _ = sr.trace_records(sc, st, o2, v2, l2, d8[:2], True)
    check_result(cam.shade_rays(o2, v2, l2, draws=d8[:2], max_life=64.0), e2)


# ---- 7. traversed ----------------------------------------------------------------------------------------------------
@gpu
def test_traversed():
    sc, st, has_bg, origins, vels, lives, draws, exp, trav = sr.ray_set("default_mb2")
    cam = cam_of("default_mb2")
    cs = sc.chunk_size
    want = sr.union_in_order(trav)
    lo, hi = want.min(0), want.max(0)
    box = ([int(v) for v in lo], [int(v) for v in (hi - lo) // cs + 1])
    assert len(want) > 600 and np.prod(box[1]) < (1 << 20)
    res = cam.shade_rays(origins, vels, lives, draws=draws, want_traversed=box)
    check_result(res, exp)
    assert np.array_equal(np.array(res.traversed(cs), np.int64).reshape(-1, 3), want)
    assert np.array_equal(res.numpy()["ntrav"], [len(t) for t in trav]) and int(res.stats[11]) == 0
    keys = res.traversed_keys.cpu().numpy()
    first = {tuple(p): k for k, t in reversed(list(enumerate(trav))) for p in t.tolist()}     # chunk -> its first ray
    cell = (want - lo) // cs
    idx = (cell[:, 0] * box[1][1] + cell[:, 1]) * box[1][2] + cell[:, 2]
    assert np.array_equal(keys[idx] >> 12, [first[tuple(p)] for p in want.tolist()]) and (keys != -1).sum() == len(want)
    # the same without records
    lean = cam.shade_rays(origins, vels, lives, draws=draws, want_traversed=box, want_records=False)
    assert np.array_equal(lean.traversed_keys.cpu().numpy(), keys)
    # a box of one cell counts the rest
    visits = []
    for k in range(600):
        sr.trace(sc, st, origins[k], vels[k], lives[k], draws[k], True, visits=visits)
    assert len(visits) == int(exp["counters"][:, sr.C_RESNAP].sum())
    one = tuple(int(v) for v in want[0])
    inside = sum(1 for p in visits if p == one)
    assert 0 < inside < len(visits)
    res1 = cam.shade_rays(origins, vels, lives, draws=draws, want_traversed=(list(one), [1, 1, 1]))
    check_result(res1, exp)
    assert int(res1.stats[11]) == len(visits) - inside and res1.traversed(cs) == [tuple(float(v) for v in one)]
    # without a box the records are identical
    sr.assert_records_equal(cam.shade_rays(origins, vels, lives, draws=draws).numpy(), res.numpy())
    # the camera's own box (around cam.pos, sized for dist_max) holds what falls inside it, in the same order
    own = cam.shade_rays(origins, vels, lives, draws=draws, want_traversed=True)
    o, d = np.array(own.trav_origin), np.array(own.trav_dims)
    inbox = ((want >= o) & (want < o + d * cs)).all(1)
    assert 0 < inbox.sum() and np.array_equal(np.array(own.traversed(cs), np.int64).reshape(-1, 3), want[inbox])


# ---- 8. hand-out independence ----------------------------------------------------------------------------------------
@gpu
def test_every_copy_of_a_ray_is_identical():
    """default_mb2 tiled to 80 400 rays under a permutation (more than a workgroup's share, many hand-outs per wave, lanes
    refilled in the middle of passes): every copy of a ray gives the oracle's record."""
    import torch
    sc, st, has_bg, origins, vels, lives, draws, exp, trav = sr.ray_set("default_mb2")
    cam = cam_of("default_mb2")
    idx = np.random.default_rng(8).permutation(600 * 134) % 600
    rec = np.zeros((len(idx), 8))
    rec[:, 0:3], rec[:, 3:6], rec[:, 6] = origins[idx], vels[idx], lives[idx]
    res = cam.shade_rays(torch.from_numpy(rec).cuda(), draws=torch.from_numpy(draws[idx]).cuda())
    want = exp[idx]
    sr.assert_records_equal(res.numpy(), want)
    assert np.array_equal(rgba_of(res), sr.packed(want)) and np.array_equal(res.stats[:11], sr.stats_of(want))
    lean = cam.shade_rays(torch.from_numpy(rec).cuda(), draws=torch.from_numpy(draws[idx]).cuda(), want_records=False)
    assert np.array_equal(rgba_of(lean), sr.packed(want))


# ---- 9. graph capture ------------------------------------------------------------------------------------------------
@gpu
def test_shade_is_graph_capturable():
    import torch
    sc, st, has_bg, origins, vels, lives, draws, exp, trav = sr.ray_set("default_mb2")
    cam = cam_of("default_mb2")
    rec = np.zeros((len(exp), 8))
    rec[:, 0:3], rec[:, 3:6], rec[:, 6] = origins, vels, lives
    drec, ddraws = torch.from_numpy(rec).cuda(), torch.from_numpy(draws).cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        cam.shade_rays(drec, draws=ddraws)       # (warm-up on the capturing side: the scene, the allocator, the pow table)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        res = cam.shade_rays(drec, draws=ddraws)
    for _ in range(2):
        res.records.zero_()
        res.rgba.view(torch.uint8).zero_()
        res._stats_dev.fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        sr.assert_records_equal(res.numpy(), exp)
        assert np.array_equal(rgba_of(res), sr.packed(exp))
        assert np.array_equal(res._stats_dev.cpu().numpy()[:11], sr.stats_of(exp))


# ---- 10. 255 materials -----------------------------------------------------------------------------------------------
@gpu
def test_255_materials():
    """The scene of tests/test_gpu_lds_room.py whose 255 material records take 16 320 bytes of the workgroup's LDS: 300 rays
    against the oracle."""
    from test_gpu_lds_room import room_scene
    sc, st_room, pos, q, lens = room_scene("mats255")
    assert len(sc.materials) == 255
    rng = np.random.default_rng(10)
    n = 300
    lo, hi = np.asarray(sc.origin, np.float64), np.asarray(sc.origin + sc.dims * sc.chunk_size, np.float64)
    origins, vels, lives, draws, exp, trav = sr.oracle_shade(sc, rng.uniform(lo, hi, (n, 3)), cr.unit_quats(rng, n),
                                                             rng.uniform(16, 92, n), 2000 + np.arange(n), 4.0, True)
    c = exp["counters"]
    hit = exp["color"][c[:, sr.C_HIT] >= 1]
    assert (c[:, sr.C_HIT] >= 1).mean() >= 0.3 and (c[:, sr.C_HIT] >= 2).mean() >= 0.1 and len(set(map(tuple, hit.tolist()))) > 100
    st = sr.shade_settings(sc.chunk_size, 4.0)
    cam = cam_for(sc, st, "mats255")
    check_result(cam.shade_rays(origins, vels, lives, draws=draws), exp)
    assert cam._c_scene(cam._ensure_scene()).n_materials == 255
