"""Where a ray's life ends (init.py:66, `ray.step < ray.life`).  march_step and hit_body decide the loop condition of the
NEXT iteration right after their advance (python_raytracer_amd/csrc/vrt_kernels.hip: LANE_ENDED from the step that uses up
the life, not from a march execution of its own); march_step keeps the test at its top for rays that are born dead.  The
decision must be the reference's to the bit: `<`, not `<=`; the life a hit has just shrunk; plain ENDED, never `broke`.

Frames: gpu_util.sparse_scene (6 x 6 x 6 chunks of 8 voxels), the camera in the middle of a present resolution-1 chunk, 64 x 48
pixels or a pixel list, 1-2 samples, bit-exact against the oracle through gpu_util.check_frame_march under "pool"
(march_pool_kernel, forced as tests/test_gpu_pool_passes.py forces it) and "lanes" (march_kernel, VRT_POOL=0): per-sample
colours, fp32 means, stats[:8] (`broke` among them), the traversed list, and check_frame_march's legs without the settled
bitmap, with the bitmap window and without the cached ray table.  No wave gave up (stats[13] == 0); the pool kernel ran where
it was asked for (stats[12] > 0).  Explicit rays: first_hit, cast_rays, shade_rays and path_rays over the same scenes against
their reference helpers (tests/test_gpu_first_hit.py, cast_ref.py, shade_ref.py, path_ref.py).

Every case first asserts from the oracle's output alone that the class of ray it is there for is among its inputs -- rays with
step == life, with step > life, with life == 0 at birth, `broke` rays, rays that the HIT body's own advance ended -- so inputs
that stop producing a class fail instead of passing empty.  The tests without the gpu mark assert the same on the CPU."""
import itertools

import numpy as np
import pytest

import cast_ref as cr
import oracle_lib as ol
import path_ref as pr
import shade_ref as sr
from gpu_util import camera_for, check_frame_march, settings_store, sparse_scene

gpu = pytest.mark.gpu

CS = 8
W, H = 64, 48
IDENTITY = np.array([0.0, 0.0, 0.0, 1.0])
# seed, highest resolution, camera: the middle of a chunk that is present at resolution 1 (asserted in scene())
SCENES = {"res1": (1, 1, (-4.0, -4.0, -4.0)), "res2": (1, 2, (-4.0, -4.0, -4.0)), "res3": (2, 3, (-4.0, -4.0, 4.0))}
NO_LOD = dict(dof=0.0, lod_bounces=0.0, lod_samples=0.0, lod_random=0.0, lod_edge=0.0)     # life == dist_max for every ray
# dist_max: the end falls on each of the eight speculative positions, on the step after a full step, and behind a chunk border
DIST = (1, 2, 3, 4, 5, 6, 7, 8, 9, 12)
# rays of the 3 072 with step == life per frame, from the CPU oracle (NO_LOD, one sample, the full window), by DIST
EXACT = {"res1": (3072, 3072, 2902, 2902, 2902, 2902, 2733, 2733, 2702, 2502),
         "res2": (3072, 3072, 3072, 2939, 2939, 2885, 2885, 2736, 2709, 2344),
         "res3": (3072, 3072, 3072, 3072, 3072, 3025, 2997, 2660, 2353, 1402)}
WINDOW = ol.pixel_lists(W, H, 1)[0]
CORNERS = np.array([[0, 0], [0, H - 1], [W - 1, 0], [W - 1, H - 1]], np.int32)
C_RESNAP, C_HIT, C_DRAW, C_BROKE = sr.C_RESNAP, sr.C_HIT, sr.C_DRAW, sr.C_BROKE

_scenes, _frames, _starts, _exits, _sets = {}, {}, {}, {}, {}


def scene(key):
    if key not in _scenes:
        seed, res_max, pos = SCENES[key]
        sc = sparse_scene(seed, res_max, CS)
        cell = tuple((np.floor(np.array(pos) / CS).astype(np.int64) * CS - sc.origin) // CS)
        assert sc.present[cell] == 1 and sc.res[cell] == 1 and int(sc.res[sc.present != 0].max()) == res_max
        _scenes[key] = (sc, np.array(pos))
    return _scenes[key]


def mixed_pixels():
    """The four corner pixels among 60 others of the window, in a fixed shuffled order."""
    inner = WINDOW[(WINDOW[:, 0] > 0) & (WINDOW[:, 0] < W - 1)]
    rng = np.random.default_rng(7)
    px = np.concatenate([CORNERS, inner[rng.permutation(len(inner))[:60]]])
    return np.ascontiguousarray(px[rng.permutation(len(px))], dtype=np.int32)


PIXELS = {"window": WINDOW, "origin": CORNERS[:1], "corners": CORNERS, "mixed": mixed_pixels()}


def frame(key, pixels="window", samples=1, **settings):
    """(scene, settings, camera position, lens, pixel list, the oracle's frame): computed once per case, shared, never changed."""
    at = (key, pixels, samples, tuple(sorted(settings.items())))
    if at not in _frames:
        sc, pos = scene(key)
        st = ol.make_settings(width=W, height=H, samples=samples, chunk_size=CS, **dict({"max_bounces": 4.0}, **settings))
        lens = st["fov"] * np.pi / 8
        o = ol.render(sc, st, pos, IDENTITY, lens, PIXELS[pixels], libm=ol.LIBM_PORTABLE)
        assert len(o["rays"]) > 0
        o["rays"].setflags(write=False)
        _frames[at] = (sc, st, pos, lens, PIXELS[pixels], o)
    return _frames[at]


def classes(o):
    """How many of a frame's rays end in each way, from the oracle's records alone."""
    r = o["rays"]
    return dict(exact=int((r["step"] == r["life"]).sum()), over=int((r["step"] > r["life"]).sum()),
                born_dead=int(((r["life"] == 0) & (r["step"] == 0) & (r["counters"][:, sr.C_ADV] == 0)).sum()),
                broke=int(r["counters"][:, C_BROKE].sum()), hit=int((r["counters"][:, C_HIT] > 0).sum()),
                resnaps=int(r["counters"][:, C_RESNAP].max()), rays=len(r))


def march(monkeypatch, which, fr):
    """The frame through the frame kernel `which` names, against the oracle; returns the statistics."""
    sc, st, pos, lens, px, o = fr
    monkeypatch.setenv("VRT_POOL", "1" if which == "pool" else "0")
    monkeypatch.setenv("VRT_POOL_MIN_RAYS", "0")
    monkeypatch.setenv("VRT_WADDR", "0")
    cam = camera_for(sc, settings_store(st), pos, IDENTITY, lens)
    r = check_frame_march(cam, o, CS, which, pixels=np.ascontiguousarray(px))
    stats = [int(v) for v in r.stats]
    assert stats[8] == len(o["rays"]), (stats[8], len(o["rays"]))
    assert stats[13] == 0, stats                      # no wave gave up
    assert (stats[12] > 0) == (which == "pool"), stats
    assert stats[C_BROKE] == classes(o)["broke"]      # (part of stats[:8]; said once more because an early ENDED must not count)
    return stats


# ---- the classes, from the oracle alone ---------------------------------------------------------------------------------------
def exact_frame(key, dist_max):
    fr = frame(key, dist_max=dist_max, **NO_LOD)
    c = classes(fr[5])
    assert c["rays"] == W * H and c["exact"] == EXACT[key][DIST.index(dist_max)] > 1000, (key, dist_max, c)
    assert c["resnaps"] >= (1, 1, 1, 1, 1, 2, 2, 3, 3, 4)[DIST.index(dist_max)], c      # (from 7 on more than one re-snap per ray)
    return fr


def overshoot_frame(key):
    """The reference's default LOD settings, two samples, dist_max 40: fractional lives, void skips past the world's edge
    (24 cells from the origin), chunks that step by 2 and 3, hits that shrink the life."""
    fr = frame(key, samples=2, dist_max=40)
    sc, st, pos, lens, px, o = fr
    c, r = classes(o), o["rays"]
    loop = r["counters"][:, C_BROKE] == 0                                           # left through the loop condition
    assert c["exact"] == 0 and (r["step"][loop] > r["life"][loop]).all() and loop.sum() > 1000 and c["broke"] > 100, c
    assert c["resnaps"] >= 3, c
    assert (np.abs(r["pos"]).max(1) > 24 + CS).sum() > 100                          # rays that went on through the void
    assert (r["life"] != np.floor(r["life"])).mean() > 0.5                          # most lives are fractional
    assert len(hit_body_exits(key)) >= 1                                            # (see below)
    return fr


def born_dead_frame(pixels):
    """lod_edge = 1.  A pixel's detail is 1 - |dir_x dir_y| with dir = -1 + 2 x / width (init.py:128-130), which is -1 at
    x = 0 and 1 - 2 / width at the last column: of the four corner pixels only (0, 0) has detail 0 exactly and a ray of life
    0; the other three have details of 0.03 .. 0.07 and rays that live for one to three steps.  So "origin" -- pixel (0, 0)
    alone -- is the launch whose every ray is born dead, "corners" the four corner pixels, "mixed" those among 60 others."""
    fr = frame("res2", pixels=pixels, samples=3, dist_max=40, lod_edge=1.0)
    r = fr[5]["rays"]
    c = classes(fr[5])
    at_origin = (r["x"] == 0) & (r["y"] == 0)
    assert c["born_dead"] == int(at_origin.sum()) == 1 and (r["detail"][at_origin] == 0).all() and (r["life"][at_origin] == 0).all(), c
    corner = np.isin(r["x"], (0, W - 1)) & np.isin(r["y"], (0, H - 1))
    assert (r["life"][corner & ~at_origin] > 0).all() and (r["life"][corner] < 4).all()
    if pixels == "origin":
        assert c["rays"] == 1, c                      # every ray of the launch
    elif pixels == "corners":
        assert c["rays"] == int(corner.sum()) == 4, c
    else:
        assert c["rays"] - int(corner.sum()) >= 60 and c["hit"] > 0 and c["over"] > 0, c
    return fr


def start_states(key):
    """origin, velocity and life of every ray of overshoot_frame(key) before its first iteration, from the oracle alone: the
    same frame over a world without chunks -- no ray hits anything, so every record still holds the velocity and the life the
    ray was born with -- and with dist_max = 0, where no ray takes a step and every record holds the origin."""
    if key not in _starts:
        sc, st, pos, lens, px, o = frame(key, samples=2, dist_max=40)
        void = ol.Scene(sc.origin, sc.dims, CS, np.zeros_like(sc.present), sc.res, np.zeros_like(sc.grid), sc.materials)
        a = ol.render(void, st, pos, IDENTITY, lens, px, libm=ol.LIBM_PORTABLE, want_traversed=False)["rays"]
        b = ol.render(sc, dict(st, dist_max=0), pos, IDENTITY, lens, px, libm=ol.LIBM_PORTABLE, want_traversed=False)["rays"]
        r = o["rays"]
        for f in ("x", "y", "s", "detail"):
            assert np.array_equal(a[f], r[f]) and np.array_equal(b[f], r[f]), f
        assert (a["counters"][:, C_HIT] == 0).all() and (b["step"] == 0).all() and np.array_equal(a["vel"], b["vel"])
        nohit = r["counters"][:, C_HIT] == 0         # (what the real frame's records can confirm)
        assert np.array_equal(a["vel"][nohit], r["vel"][nohit]) and np.array_equal(a["life"][nohit], r["life"][nohit])
        _starts[key] = (b["pos"].copy(), a["vel"].copy(), a["life"].copy())
    return _starts[key]


def hit_body_exits(key):
    """Indices of the rays of overshoot_frame(key) that leave the loop straight after the HIT body's advance: the life their
    last hit left them was past the pre-advance test (`step >= life`: the reference's break) and is used up by that one
    advance.  path_ref.trace_path -- the loop restated in Python -- runs every ray that ends with bounces > 0 and not `broke`
    from its start state with the draws of its seed; its record must be the oracle's to the bit (which pins the restatement on
    exactly these rays), and the ray took this exit iff its last step is its last hit's step plus that chunk's step size."""
    if key not in _exits:
        sc, st, pos, lens, px, o = frame(key, samples=2, dist_max=40)
        origins, vels, lives = start_states(key)
        r = o["rays"]
        first = 1 + 2 * (st["dof"] != 0)             # lod_random's draw and the two lens draws come before the loop's
        cand = np.flatnonzero((r["bounces"] > 0) & (r["counters"][:, C_BROKE] == 0))
        assert len(cand) >= 100, len(cand)
        out = []
        for k in cand:
            n = int(r["counters"][k, C_DRAW]) - first
            assert n >= 0 and n % 3 == 0
            seed = (1 + int(r["x"][k])) * (1 + int(r["y"][k])) * (1 + int(r["s"][k]))
            draws = ol.rng_draws(seed, first + n)[first:]
            rec, path = pr.trace_path(sc, st, origins[k], vels[k], lives[k], draws, True)
            for f in ("step", "life", "bounces", "energy", "pos", "vel"):
                assert np.array_equal(np.ascontiguousarray(rec[f]).view(np.uint64), np.ascontiguousarray(r[f][k]).view(np.uint64)), (k, f)
            assert np.array_equal(rec["color"], r["color"][k]) and len(path) == int(r["counters"][k, C_HIT]) >= 1
            step, _, cell, _ = path[-1]
            size = float(int(sc.res[tuple((np.array(cell, np.int64) - sc.origin) // CS)]))
            if float(rec["step"]) == step + size:
                assert not float(rec["step"]) < float(rec["life"])
                out.append(int(k))
        _exits[key] = out
    return _exits[key]


# ---- the explicit rays ----------------------------------------------------------------------------------------------------------
def ray_set(key):
    """About 200 explicit rays over scene(key) with its own materials and lod_bounces = 0 (a smooth material then leaves the
    life of a ray in a resolution-1 chunk as it is): axis-parallel rays from integer and half-integer positions with integer
    lives (step == life unless they hit), rays that start 1 .. 6 cells in front of a filled voxel of a resolution-1 chunk and
    live one step longer than it takes to reach it, Chebyshev-normalised directions with fractional lives, and lives <= 0.
    Returns (scene, settings, origins, velocities, lives, draws, shade_ref's records, path_ref's counts and paths, cast_ref's
    records): computed once, shared, never changed."""
    if key in _sets:
        return _sets[key]
    sc, pos = scene(key)
    st = sr.shade_settings(CS, 4.0, lod_bounces=0.0)
    rng = np.random.default_rng(5)
    o, v, l = [], [], []

    def add(origin, vel, life):
        o.append(np.asarray(origin, np.float64)), v.append(np.asarray(vel, np.float64)), l.append(float(life))

    for axis, sign in itertools.product(range(3), (1.0, -1.0)):
        vel = [0.0, 0.0, 0.0]
        vel[axis] = sign
        for life in (1, 2, 3, 5, 8, 9, 12, 30):
            add(pos + (0.5 if life % 2 else 0.0), vel, life)
    idx = np.argwhere(sc.grid > 0)
    idx = idx[sc.res[tuple((idx // CS).T)] == 1]
    for cell in idx[rng.choice(len(idx), 60, replace=False)] + sc.origin:
        axis, sign, k = int(rng.integers(3)), float(rng.choice([1.0, -1.0])), int(rng.integers(1, 7))
        vel = [0.0, 0.0, 0.0]
        vel[axis] = sign
        add(cell + 0.5 - np.array(vel) * k, vel, k + 1)
    for k in range(80):
        d = rng.normal(size=3)
        add(pos + rng.uniform(-6, 6, 3), d / np.abs(d).max(), rng.uniform(0.5, 40))
    for life in (0.0, -1.0, -0.0):
        add(pos + rng.uniform(-3, 3, 3), [0.5, 1.0, -0.25], life)
        add(pos + rng.uniform(-3, 3, 3), [1.0, -0.5, -0.25], life)
    o, v, l = np.array(o), np.array(v), np.array(l)
    draws = np.stack([ol.rng_draws(9000 + k, sr.N_DRAWS) for k in range(len(o))])
    exp, _ = sr.trace_records(sc, st, o, v, l, draws, True)
    rec, counts, paths = pr.trace_paths(sc, st, o, v, l, draws, True)
    assert (exp["s"] == 0).all() and (counts >= 0).all()
    sr.assert_records_equal(rec, exp)
    hits = cr.march_records(sc, st["chunk_radius"], o, v, l)
    assert np.array_equal(hits["material"] > 0, counts > 0)
    # the classes: exact endings with and without a hit, overshoots, rays that never loop, `broke` rays, and rays that the
    # HIT body's own advance ends (the last step is the last hit's plus that chunk's step size) -- on step == life among them
    nohit = counts == 0
    after_hit = np.zeros(len(o), bool)
    for k, path in enumerate(paths):
        if path and exp["counters"][k, C_BROKE] == 0:
            size = float(int(sc.res[tuple((np.array(path[-1][2], np.int64) - sc.origin) // CS)]))
            after_hit[k] = float(exp["step"][k]) == path[-1][0] + size
    figures = dict(exact_nohit=int((nohit & (exp["step"] == exp["life"]) & (l > 0)).sum()),
                   over=int(((exp["step"] > exp["life"]) & (exp["counters"][:, C_BROKE] == 0)).sum()),
                   never=int(((l <= 0) & (exp["step"] == 0)).sum()), broke=int(exp["counters"][:, C_BROKE].sum()),
                   after_hit=int(after_hit.sum()), after_hit_exact=int((after_hit & (exp["step"] == exp["life"])).sum()))
    assert figures["exact_nohit"] >= 10 and figures["over"] >= 30 and figures["never"] == 6 and figures["broke"] >= 5, figures
    assert figures["after_hit"] >= 3 and figures["after_hit_exact"] >= 1, figures
    for a in (o, v, l, draws, exp, counts, hits):
        a.setflags(write=False)
    _sets[key] = (sc, st, o, v, l, draws, exp, counts, paths, hits, figures)
    return _sets[key]


def first_hit_case(key):
    """The exact-ending frame of dist_max 12 as a first-hit pass (id materials, max_bounces 0): (settings, lens, the expected
    records); rays that find nothing with step == life == 12, and rays that find a voxel, are both there."""
    from test_gpu_first_hit import oracle_hits
    sc, pos = scene(key)
    st = ol.make_settings(width=W, height=H, samples=1, chunk_size=CS, dist_max=12, **NO_LOD)
    lens = st["fov"] * np.pi / 8
    exp = oracle_hits(sc, st, pos, IDENTITY, lens, WINDOW, vacuous_ok=True)
    none = exp["material"] == 0
    assert (exp["step"][none] == 12.0).sum() >= 100 and (exp["material"] > 0).sum() >= 10, (none.sum(), (exp["material"] > 0).sum())
    return st, lens, exp


# ---- on the CPU: the inputs hold their classes ------------------------------------------------------------------------------
@pytest.mark.parametrize("key", sorted(SCENES))
def test_inputs_hold_their_classes(key):
    for dist_max in DIST:
        exact_frame(key, dist_max)
    overshoot_frame(key)
    first_hit_case(key)
    print(key, "rays ended by the HIT body's advance, of the default-LOD frame:", len(hit_body_exits(key)), ray_set(key)[10])


def test_corner_pixels_are_born_dead():
    for pixels in ("origin", "corners", "mixed"):
        born_dead_frame(pixels)


# ---- on the GPU -------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("which", ["pool", "lanes"])
@pytest.mark.parametrize("dist_max", DIST)
@pytest.mark.parametrize("key", sorted(SCENES))
def test_step_lands_on_the_life(monkeypatch, key, dist_max, which):
    """life == dist_max, integer step sizes: EXACT rays of the frame reach step == life and must end there -- not one
    position later (`<=`), and as plain ended rays."""
    march(monkeypatch, which, exact_frame(key, dist_max))


@gpu
@pytest.mark.parametrize("which", ["pool", "lanes"])
@pytest.mark.parametrize("key", sorted(SCENES))
def test_overshoot(monkeypatch, key, which):
    """Default LOD settings: no ray ends on its life exactly, every one steps past it -- by a void skip, a step of 2 or 3,
    or the advance behind a hit that has just shrunk the life (hit_body_exits: at least one ray of the frame does)."""
    stats = march(monkeypatch, which, overshoot_frame(key))
    assert stats[C_HIT] > 0 and stats[C_BROKE] > 0


@gpu
@pytest.mark.parametrize("which", ["pool", "lanes"])
@pytest.mark.parametrize("pixels", ["origin", "corners", "mixed"])
def test_born_dead(monkeypatch, pixels, which):
    """lod_edge = 1: pixel (0, 0) has detail 0, its ray life 0 -- ended by the test at the top of march_step, which no
    take_ray site replaces.  That pixel alone: every ray of the launch; the four corners; the corners among 60 other pixels."""
    stats = march(monkeypatch, which, born_dead_frame(pixels))
    if pixels == "origin":
        assert stats[:5] == [0, 0, 0, 0, 0] and stats[sr.C_ADV] == 0, stats


@gpu
@pytest.mark.parametrize("key", sorted(SCENES))
def test_first_hit(key):
    """A ray that finds nothing reports the position its life ended at: first_hit_kernel leaves its loop on LANE_ENDED."""
    from test_gpu_first_hit import assert_records_equal, check_against_oracle
    st, lens, want = first_hit_case(key)
    sc, pos = scene(key)
    cam, h, exp = check_against_oracle(sc, st, pos, IDENTITY, lens, vacuous_ok=True)
    assert np.array_equal(h.pixels, WINDOW)
    assert_records_equal(exp, want)


@gpu
@pytest.mark.parametrize("key", sorted(SCENES))
def test_cast_rays(key):
    from test_gpu_shade import cam_for
    sc, st, o, v, l, draws, exp, counts, paths, hits, figures = ray_set(key)
    res = cam_for(sc, st, ("life_end", key)).cast_rays(o, v, l, max_life=64.0)
    cr.assert_records_equal(res.numpy(), hits)
    assert int(res.stats[8]) == len(o) and int(res.stats[4]) == int((hits["material"] > 0).sum()) and not res.rejected_mask().any()


@gpu
@pytest.mark.parametrize("key", sorted(SCENES))
def test_shade_rays(key):
    from test_gpu_shade import cam_for, check_result, rgba_of
    sc, st, o, v, l, draws, exp, counts, paths, hits, figures = ray_set(key)
    cam = cam_for(sc, st, ("life_end", key))
    res = cam.shade_rays(o, v, l, draws=draws, max_life=64.0)
    check_result(res, exp)
    assert int(res.stats[C_BROKE]) == figures["broke"]
    lean = cam.shade_rays(o, v, l, draws=draws, max_life=64.0, want_records=False)
    assert np.array_equal(rgba_of(lean), sr.packed(exp)) and np.array_equal(lean.stats[:11], res.stats[:11])


@gpu
@pytest.mark.parametrize("key", sorted(SCENES))
def test_path_rays(key):
    from test_gpu_paths import check_paths
    from test_gpu_shade import cam_for
    sc, st, o, v, l, draws, exp, counts, paths, hits, figures = ray_set(key)
    res = cam_for(sc, st, ("life_end", key)).path_rays(o, v, l, draws=draws, max_hits=8, max_life=64.0)
    check_paths(res, exp, counts, paths, 8)
