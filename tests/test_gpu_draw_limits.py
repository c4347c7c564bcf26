"""Frames whose rays outrun the draw tables: counted, retried, raised.

A ray's random draws come from a stack of tables (include/vrt.h, vrt_workspace_bytes): the frame's table of `fast_draws` =
32 or 64 draws per seed; a first re-trace tier of private 113-draw rows for at most 1/64 of a march launch's ray slots, held
between 2^18 and 2^22 (the whole launch if it is smaller); a second tier of 1024-draw rows for at most 4096 rays of a launch.
A ray that finds no room is counted in d_stats[10]; Camera.render / render_views then retry once with 64 draws per seed and
raise if rays are still left over.  The other GPU modules only ever assert stats[10] == 0.  Here every regime is reached
with a tiny scene (CASES) and pinned to the CPU oracle: the counts at each list's capacity, the retry, the VrtError, the
state a frame that raised leaves behind, launches cut to 4096 rays (where no list can overflow), batches of views, and
re-seeded frames under the nonces render() really draws (63 bits, two-word MT19937 keys).

The limits are read from the header's text (header_limits), never asked of the library.  The reference of every value is the
CPU oracle in its portable-libm mode, computed once per case and shared (oracle_frame); each case is first shown, from the
oracle's per-ray draw counters alone and on the CPU, to lie where its name says (test_cases_lie_at_their_limits).  With
static seeds a ray's stream depends on its pixel and sample only -- and under a nonce on the window slot of the pixel --, so
the oracle's frame also gives the expected values of every sub-list of its pixels (expected_for)."""
import os
import re

import numpy as np
import pytest

import oracle_lib as ol
from gpu_util import camera_for, check_frame_march, run_children, settings_store, sparse_scene

gpu = pytest.mark.gpu

DRAW = ol.COUNTERS.index("draw")
IDENTITY = np.array([0.0, 0.0, 0.0, 1.0])
S_RAYS, S_RETRACED, S_EXHAUSTED = 8, 9, 10


def header_limits():
    """The draw limits as include/vrt.h's comment on vrt_workspace_bytes states them."""
    with open(os.path.join(ol.ROOT, "include", "vrt.h")) as f:
        text = re.sub(r"\s*\n\s*\*\s*", " ", f.read())           # (comment lines joined)
    fast = re.search(r"kept per distinct seed in the frame's table, (\d+) or (\d+);", text)
    slow = re.search(r"re-traced with a private (\d+)-draw row", text)
    full = re.search(r"with a (\d+)-draw row from a full-state MT19937", text)
    caps = re.search(r"first re-trace list holds 1/(\d+) of the launch's ray slots, held between 2\^(\d+) and 2\^(\d+) \(the whole launch "
                     r"if it has fewer than 2\^(\d+)\), and the second (\d+) rays", text)
    assert fast and slow and full and caps, "include/vrt.h no longer states the draw limits in these words"
    assert caps.group(2) == caps.group(4)
    return dict(fast=(int(fast.group(1)), int(fast.group(2))), slow=int(slow.group(1)), full=int(full.group(1)),
                share=int(caps.group(1)), list_min=1 << int(caps.group(2)), list_max=1 << int(caps.group(3)), full_cap=int(caps.group(5)))


LIM = header_limits()
D32, D64 = LIM["fast"]
D113, D1024, CAP2, CAP1 = LIM["slow"], LIM["full"], LIM["full_cap"], LIM["list_min"]


def first_list_cap(launch):
    """Rays of a march launch of `launch` ray slots that the first re-trace list holds (the header's rule)."""
    return min(launch, min(max(launch // LIM["share"], LIM["list_min"]), LIM["list_max"]))


# ------------------------------------------------------------------------------------------------- the scene family
# One dense box for all cases: 3 x 2 x 3 chunks of 16 cells, all present at resolution 1, 9 cells in 10 filled, a 5^3 pocket
# round an unrotated camera; three rough materials (roughness 1 / 0.5 / 1) that share one absorption `a`: the lower it is,
# the more rough hits -- three draws each -- a ray takes before its life (dist_max) runs out.  max_light 100, lod_bounces 0
# and falloff 0 keep the rays from ending early.  The comment of a case is what the oracle alone gives for it
# (rays; rays with more than 32 / 64 / 113 / 1024 draws; the largest draw count).
CASES = {
    # 13824; 13824 / 13822 / 13816 / 0; 546
    "tier3": dict(width=96, height=72, samples=2, a=0.02, max_bounces=16.0, dist_max=400),
    # 2400; 2400 / 2400 / 2400 / 324; 1182
    "over1024": dict(width=40, height=30, samples=2, a=0.02, max_bounces=16.0, dist_max=1200),
    # 327680; 293529 / 107867 / 0 / 0; 66
    "list32": dict(width=512, height=320, samples=2, a=0.35, max_bounces=6.0, dist_max=200),
    # 327680; 327534 / 317922 / 0 / 0; 108.  The cap of `bounces` (max_bounces + 1 = 7, a per hit) is what keeps every ray within
    # 113 draws: a = 0.19 already lets 55 426 rays past them, and at a = 0.2 with list32's dist_max only 220 513 rays pass 64
    # draws -- fewer than the list holds -- so this case lengthens the rays' lives instead of lowering a further
    "list64": dict(width=512, height=320, samples=2, a=0.2, max_bounces=6.0, dist_max=400),
    # the three views: 3072 each; 3072 / 3072, 3072, 3071 / 3072, 3072, 3070 / 0; 549
    "views": dict(width=64, height=48, samples=1, a=0.02, max_bounces=16.0, dist_max=400),
}
LARGE = ("list32", "list64")
CS, DIMS, ORIGIN = 16, np.array([3, 2, 3]), np.array([-1, -1, -2]) * 16
POS = np.floor(ORIGIN + np.array([0.45, 0.55, 0.4]) * DIMS * CS) + np.array([0.3, 0.6, 0.45])
# the second and third view of the batches: the camera moved inside its pocket, and turned
VIEW_POSES = [(POS, IDENTITY), (POS + np.array([0.4, -0.3, 0.25]), IDENTITY),
              (POS, np.array([0.0, 0.38268343236508978, 0.0, 0.92387953251128674]))]

_scenes, _oracle = {}, {}


def limit_scene(name):
    """(scene, settings, lens) of a case; deterministic, built once."""
    if name not in _scenes:
        c = CASES[name]
        rng = np.random.default_rng(2024)
        st = ol.make_settings(width=c["width"], height=c["height"], samples=c["samples"], chunk_size=CS, max_bounces=c["max_bounces"],
                              dist_max=c["dist_max"], max_light=100.0, lod_bounces=0.0, falloff=0.0)
        a = c["a"]
        mats = np.array([[200, 180, 160, 1.0, a, 1.0, 0.0], [90, 120, 250, 0.5, a, 0.5, 0.0], [60, 200, 90, 1.0, a, 0.75, 0.0]])
        shape = tuple(DIMS * CS)
        grid = np.where(rng.random(shape) < 0.9, rng.integers(1, 4, shape), 0).astype(np.uint8)
        lo = (np.floor(POS) - ORIGIN).astype(np.int64) - 2
        grid[lo[0]:lo[0] + 5, lo[1]:lo[1] + 5, lo[2]:lo[2] + 5] = 0
        ones = np.ones(tuple(DIMS), np.uint8)
        _scenes[name] = (ol.Scene(ORIGIN, DIMS, CS, ones, ones, grid, mats), st, st["fov"] * np.pi / 8)
    return _scenes[name]


def frame_pixels(name):
    """The whole window in settings.pixels[0]'s order (one thread)."""
    c = CASES[name]
    return ol.pixel_lists(c["width"], c["height"], 1)[0]


def oracle_frame(name, view=0, seed_nonce=0, pixels=None):
    """The oracle's frame of a case (of one of VIEW_POSES; under a nonce; of a pixel list other than the whole window --
    then with the traversed list): computed once, shared by every test and leg, never modified."""
    key = (name, view, seed_nonce, None if pixels is None else pixels.tobytes())
    if key not in _oracle:
        sc, st, lens = limit_scene(name)
        pos, rot = VIEW_POSES[view]
        kw = dict(threads=8, want_traversed=False) if pixels is None else {}
        _oracle[key] = ol.render(sc, st, pos, rot, lens, frame_pixels(name) if pixels is None else pixels, libm=ol.LIBM_PORTABLE,
                                 seed_nonce=seed_nonce, **kw)
    return _oracle[key]


def figures(o):
    """Rays of an oracle frame, those that need more draws than each table holds, and the largest draw count."""
    d = o["rays"]["counters"][:, DRAW]
    return dict(rays=len(d), n32=int((d > D32).sum()), n64=int((d > D64).sum()), n113=int((d > D113).sum()),
                n1024=int((d > D1024).sum()), draw_max=int(d.max()))


def packed(rays):
    return (rays["color"][:, 0].astype(np.uint32) | (rays["color"][:, 1].astype(np.uint32) << 8) |
            (rays["color"][:, 2].astype(np.uint32) << 16) | (rays["alpha"].astype(np.uint32) << 24))


def expected_for(name, o, pixels):
    """What a frame of `pixels` (distinct pixels of the window) must give, from the oracle's frame `o` of the whole window:
    the oracle's rays of those pixels, their slot in the list's per-sample output, the pixels' fp32 means, the event
    counters summed over those rays."""
    c = CASES[name]
    H = c["height"]
    rays = o["rays"]
    where = np.full(c["width"] * H, -1, np.int64)
    where[pixels[:, 0].astype(np.int64) * H + pixels[:, 1]] = np.arange(len(pixels))
    at = where[rays["x"].astype(np.int64) * H + rays["y"]]
    sel = rays[at >= 0]
    full = frame_pixels(name)
    row = np.full(c["width"] * H, -1, np.int64)
    row[full[:, 0].astype(np.int64) * H + full[:, 1]] = np.arange(len(full))
    return dict(rays=sel, slot=at[at >= 0] * c["samples"] + sel["s"], draws=sel["counters"][:, DRAW],
                mean=o["pix_mean"][row[pixels[:, 0].astype(np.int64) * H + pixels[:, 1]]].astype(np.float32),
                counters=sel["counters"].astype(np.int64).sum(0))


def per_pixel_over(name, o, limit):
    """For every pixel of the window, in frame_pixels' order: how many of its rays need more than `limit` draws."""
    c = CASES[name]
    rays = o["rays"]
    n = np.zeros(c["width"] * c["height"], np.int64)
    np.add.at(n, rays["x"].astype(np.int64) * c["height"] + rays["y"], rays["counters"][:, DRAW] > limit)
    full = frame_pixels(name)
    return n[full[:, 0].astype(np.int64) * c["height"] + full[:, 1]]


def capacity_lists(name, o):
    """Pixel lists at the second list's capacity, chosen from the oracle's counts: the pixels of the window in order, each
    taken while the rays that need more than 113 draws stay within 4096, until they are exactly 4096; and that list plus
    the next pixel that has such rays.  Returns (fitting list, list one pixel over, rays that pixel adds beyond 113)."""
    over = per_pixel_over(name, o, D113)
    full = frame_pixels(name)
    take, total = [], 0
    for i, k in enumerate(over):
        if total + k <= CAP2:
            take.append(i)
            total += int(k)
        if total == CAP2:
            break
    assert total == CAP2, total
    taken = set(take)
    extra = next(i for i, k in enumerate(over) if k > 0 and i not in taken)
    return full[take], full[take + [extra]], int(over[extra])


def case_proof(name):
    """Does the oracle's frame lie where the case is named after?  From the draw counters alone; returns the figures."""
    o = oracle_frame(name)
    fig = figures(o)
    assert fig["rays"] == o["n_rays"] == len(frame_pixels(name)) * CASES[name]["samples"]
    assert (o["rays"]["counters"].astype(np.int64).sum(0) == o["counters"]).all()
    if name == "tier3":
        assert fig["n113"] > CAP2 and fig["n1024"] == 0, fig
        assert fig["rays"] < CAP1                          # the first list holds the whole launch
        fit, over, added = capacity_lists(name, o)
        assert len(over) == len(fit) + 1 and added >= 1
    elif name == "over1024":
        assert 1 <= fig["n1024"] <= fig["rays"] // 2 and fig["n113"] <= CAP2, fig
    elif name == "list32":
        assert fig["n32"] > CAP1 >= fig["n64"] and fig["n113"] == 0, fig
        assert first_list_cap(fig["rays"]) == CAP1
    elif name == "list64":
        assert fig["n64"] > CAP1 and fig["n113"] == 0, fig
        assert first_list_cap(fig["rays"]) == CAP1
    elif name == "views":
        for v in range(len(VIEW_POSES)):
            f = figures(oracle_frame(name, v))
            assert f["n113"] <= CAP2 and f["n1024"] == 0 and f["n113"] > CAP2 // 2, (v, f)   # one fits, any two do not
    return fig


# ------------------------------------------------------------------------------------------------- 1. on the CPU
def test_header_states_the_limits():
    assert (D32, D64, D113, D1024, CAP2, CAP1) == (32, 64, 113, 1024, 4096, 1 << 18), LIM
    assert first_list_cap(13824) == 13824 and first_list_cap(327680) == 1 << 18 and first_list_cap(1 << 28) == 1 << 22


def test_error_text_states_the_header_rule():
    """The VrtError of Camera.render and render_views names every limit the header does."""
    from python_raytracer_amd import camera
    for what in ("frame", "batch"):
        text = camera._EXHAUSTED_RULE % what
        for word in ("more than %d random draws" % D1024, "more than %d rays" % CAP2, "more than %d draws" % D113, "1/%d of the launch" % LIM["share"],
                     "2**18", "2**22", "the whole launch if it is smaller", "%d-draw table" % D64, "of the %s" % what):
            assert word in text, (word, text)


@pytest.mark.parametrize("case", list(CASES))
def test_cases_lie_at_their_limits(case):
    """Every case against its condition (case_proof), from the oracle's output alone: a case that drifts off its limit
    fails here, without a GPU."""
    case_proof(case)


# ------------------------------------------------------------------------------------------------- GPU helpers
@pytest.fixture(params=["pool", "lanes"])
def frame_march(request, monkeypatch):
    """Both frame kernels, as the `frame_march` fixtures of the other GPU modules choose them (without their look-ahead legs)."""
    monkeypatch.setenv("VRT_POOL", "1" if request.param == "pool" else "0")
    monkeypatch.setenv("VRT_POOL_MIN_RAYS", "0")
    monkeypatch.setenv("VRT_WADDR", "0")
    return request.param


def camera(name, view=0):
    sc, st, lens = limit_scene(name)
    return camera_for(sc, settings_store(st), VIEW_POSES[view][0], VIEW_POSES[view][1], lens)


def device_stats(r):
    return [int(v) for v in r._stats_dev.cpu().numpy()]


def assert_ran(stats, which):
    """The frame kernel the leg names ran (march_pool_kernel's workgroups count themselves in stats[12])."""
    groups = stats[12] & 0xffffffff
    assert (groups > 0) == (which == "pool"), (which, groups)


def assert_exact(r, stats, exp, which=None):
    """A frame that completed: per-sample colours, fp32 means, event counters; every ray traced, none left over."""
    got = r.ray_rgba.cpu().numpy().view(np.uint32)
    assert np.array_equal(got[exp["slot"]], packed(exp["rays"]))
    assert np.array_equal(r.rgba_f32.cpu().numpy(), exp["mean"])
    assert stats[:8] == [int(v) for v in exp["counters"]], (stats[:8], exp["counters"])
    assert stats[S_RAYS] == len(exp["rays"]) and stats[S_EXHAUSTED] == 0, stats
    if which is not None:
        assert_ran(stats, which)


def whole(name, o=None):
    return expected_for(name, oracle_frame(name) if o is None else o, frame_pixels(name))


# ------------------------------------------------------------------------------------------------- 2. tier3
@gpu
@pytest.mark.parametrize("fast", [32, 64])
def test_tier3_accounting(frame_march, fast):
    """13 819 rays of one launch need more than 113 draws and the second list holds 4096: exactly the others are counted in
    stats[10], every ray is either traced or counted, every ray within 113 draws has the oracle's colour, and at least 4096 of
    the others have it too (which 4096 is the schedule's choice).  stats[9]: the rays that were re-traced to their end --
    the oracle's count of rays beyond `fast` draws less those left over."""
    exp = whole("tier3")
    fig = figures(oracle_frame("tier3"))
    cam = camera("tier3")
    cam.fast_draws = fast
    r = cam.render(0, want_ray_rgba=True, check=False)
    assert np.array_equal(r.pixels, frame_pixels("tier3"))
    stats = device_stats(r)
    print("tier3", frame_march, fast, fig, stats[8:11])
    assert_ran(stats, frame_march)
    assert stats[S_EXHAUSTED] == fig["n113"] - CAP2, (stats, fig)
    assert stats[S_RAYS] + stats[S_EXHAUSTED] == fig["rays"], (stats, fig)
    n_fast = fig["n32"] if fast == 32 else fig["n64"]
    assert stats[S_RETRACED] == n_fast - stats[S_EXHAUSTED], (stats, fig)
    same = r.ray_rgba.cpu().numpy().view(np.uint32)[exp["slot"]] == packed(exp["rays"])
    within = exp["draws"] <= D113
    assert same[within].all(), np.flatnonzero(~same & within)[:5]
    assert int(same[~within].sum()) >= CAP2, int(same[~within].sum())
    assert cam.fast_draws == fast                # (an unchecked frame changes nothing)


@gpu
def test_tier3_retries_then_raises_and_leaves_a_clean_state(frame_march):
    """With the check on the frame is rendered again with 64 draws per seed (cam.fast_draws says so afterwards) and then
    raises, naming the count.  The next frame of the same Camera, a pixel list that fits, is exact: counters and lists
    of the frame that raised are clean again."""
    from python_raytracer_amd import _native as nat
    o = oracle_frame("tier3")
    fig = figures(o)
    cam = camera("tier3")
    assert cam.fast_draws == 32
    with pytest.raises(nat.VrtError) as err:
        cam.render(0, want_ray_rgba=True)
    assert cam.fast_draws == 64
    left = fig["n113"] - CAP2
    assert str(err.value).startswith("%d rays could not be completed" % left), str(err.value)
    assert int(cam.last_stats[S_EXHAUSTED]) == left
    fit, _, _ = capacity_lists("tier3", o)
    exp = expected_for("tier3", o, fit)
    r = cam.render(0, pixels=fit, want_ray_rgba=True)
    assert_exact(r, [int(v) for v in r.stats], exp, frame_march)
    assert int(r.stats[S_RETRACED]) == int((exp["draws"] > D64).sum())


@gpu
@pytest.mark.parametrize("fast", [32, 64])
def test_tier3_capacity_edge(frame_march, fast):
    """A pixel list whose rays include exactly 4096 that need more than 113 draws completes, bit-exact, with stats[9] the
    oracle's count of its rays beyond `fast` draws; one more pixel with such rays leaves exactly its rays over."""
    o = oracle_frame("tier3")
    fit, over, added = capacity_lists("tier3", o)
    exp = expected_for("tier3", o, fit)
    assert int((exp["draws"] > D113).sum()) == CAP2
    cam = camera("tier3")
    cam.fast_draws = fast
    r = cam.render(0, pixels=fit, want_ray_rgba=True, check=False)
    stats = device_stats(r)
    print("tier3 fit", frame_march, fast, len(exp["rays"]), stats[8:11])
    assert_exact(r, stats, exp, frame_march)
    assert stats[S_RETRACED] == int((exp["draws"] > fast).sum()), stats
    exp1 = expected_for("tier3", o, over)
    r1 = cam.render(0, pixels=over, want_ray_rgba=True, check=False)
    stats1 = device_stats(r1)
    print("tier3 over", frame_march, fast, len(exp1["rays"]), stats1[8:11])
    assert stats1[S_EXHAUSTED] == added and stats1[S_RAYS] == len(exp1["rays"]) - added, (stats1, added)
    assert stats1[S_RETRACED] == int((exp1["draws"] > fast).sum()) - added, stats1
    same = r1.ray_rgba.cpu().numpy().view(np.uint32)[exp1["slot"]] == packed(exp1["rays"])
    assert same[exp1["draws"] <= D113].all() and int(same[exp1["draws"] > D113].sum()) >= CAP2


def _small_launch_child(which):
    """Run in a child process with VRT_BATCH_LOG2=12 (read once per process): the tier3 frame as four launches of at most
    4096 ray slots, the last of them short."""
    exp = whole("tier3")
    cam = camera("tier3")
    r = cam.render(0, want_ray_rgba=True)
    stats = [int(v) for v in r.stats]
    assert_exact(r, stats, exp, which)
    assert cam.fast_draws == 64                  # (the frame completed, and re-traced more than 1 ray in 50)
    print("SMALL", " ".join(str(v) for v in stats[8:11]))


@gpu
def test_tier3_in_launches_of_4096_rays_completes(frame_march):
    """Launches of 4096 ray slots can never overflow a list: the same frame completes bit-exact, all of its 13 819 second-tier
    rays re-traced over four launches -- which also holds the counters' clear between launches."""
    fig = figures(oracle_frame("tier3"))
    assert fig["rays"] > 3 * CAP2 and fig["rays"] % CAP2 != 0
    words = run_children("import test_gpu_draw_limits as t; t._small_launch_child(%r)" % frame_march, [{"VRT_BATCH_LOG2": "12"}], "SMALL")[0]
    assert [int(w) for w in words[1:]] == [fig["rays"], fig["n32"], 0], (words, fig)


# ------------------------------------------------------------------------------------------------- 3. over1024
@gpu
def test_over1024(frame_march):
    """Rays that outrun the last table, 1024 draws: counted one by one, the others exact; with the check on the frame raises
    (after its retry at 64 draws)."""
    from python_raytracer_amd import _native as nat
    exp = whole("over1024")
    fig = figures(oracle_frame("over1024"))
    cam = camera("over1024")
    for fast in (32, 64):
        cam.fast_draws = fast
        r = cam.render(0, want_ray_rgba=True, check=False)
        stats = device_stats(r)
        print("over1024", frame_march, fast, fig, stats[8:11])
        assert_ran(stats, frame_march)
        assert stats[S_EXHAUSTED] == fig["n1024"] and stats[S_RAYS] == fig["rays"] - fig["n1024"], (stats, fig)
        assert stats[S_RETRACED] == (fig["n32"] if fast == 32 else fig["n64"]) - fig["n1024"], (stats, fig)
        same = r.ray_rgba.cpu().numpy().view(np.uint32)[exp["slot"]] == packed(exp["rays"])
        assert same[exp["draws"] <= D1024].all()
    cam.fast_draws = 32
    with pytest.raises(nat.VrtError) as err:
        cam.render(0)
    assert cam.fast_draws == 64 and str(err.value).startswith("%d rays could not be completed" % fig["n1024"]), str(err.value)


# ------------------------------------------------------------------------------------------------- 4. list32, list64
@gpu
def test_list32_accounting(frame_march):
    """More than 2^18 rays of one launch outrun 32 draws: the first list holds 2^18, the others are counted."""
    fig = figures(oracle_frame("list32"))
    exp = whole("list32")
    cam = camera("list32")
    r = cam.render(0, want_ray_rgba=True, check=False)
    stats = device_stats(r)
    print("list32", frame_march, 32, fig, stats[8:11])
    assert_ran(stats, frame_march)
    assert stats[S_EXHAUSTED] == fig["n32"] - CAP1, (stats, fig)
    assert stats[S_RAYS] + stats[S_EXHAUSTED] == fig["rays"], (stats, fig)
    assert stats[S_RETRACED] == CAP1, stats
    same = r.ray_rgba.cpu().numpy().view(np.uint32)[exp["slot"]] == packed(exp["rays"])
    assert same[exp["draws"] <= D32].all() and int(same[exp["draws"] > D32].sum()) >= CAP1


@gpu
def test_list32_silent_retry(frame_march):
    """The same frame with the check on: rendered again with 64 draws per seed, which its first list holds, and returned
    -- exact, nothing raised."""
    fig = figures(oracle_frame("list32"))
    cam = camera("list32")
    r = cam.render(0, want_ray_rgba=True)
    stats = [int(v) for v in r.stats]
    print("list32 retry", frame_march, 64, fig, stats[8:11])
    assert cam.fast_draws == 64
    assert_exact(r, stats, whole("list32"), frame_march)
    assert stats[S_RETRACED] == fig["n64"], (stats, fig)


@gpu
def test_list64_raises(frame_march):
    """More than 2^18 rays outrun 64 draws as well: the retry does not help, and the frame raises with the count."""
    from python_raytracer_amd import _native as nat
    fig = figures(oracle_frame("list64"))
    cam = camera("list64")
    with pytest.raises(nat.VrtError) as err:
        cam.render(0)
    stats = [int(v) for v in cam.last_stats]
    print("list64", frame_march, 64, fig, stats[8:11])
    assert cam.fast_draws == 64
    assert stats[S_EXHAUSTED] == fig["n64"] - CAP1 and stats[S_RAYS] + stats[S_EXHAUSTED] == fig["rays"], (stats, fig)
    assert stats[S_RETRACED] == CAP1, stats
    assert str(err.value).startswith("%d rays could not be completed" % stats[S_EXHAUSTED]), str(err.value)


# ------------------------------------------------------------------------------------------------- 5. views
def view_expected(v):
    return expected_for("views", oracle_frame("views", v), frame_pixels("views"))


def assert_view_exact(r, exp):
    assert np.array_equal(r.ray_rgba.cpu().numpy().view(np.uint32)[exp["slot"]], packed(exp["rays"]))
    assert np.array_equal(r.rgba_f32.cpu().numpy(), exp["mean"])


@gpu
def test_views_one_pose_completes(frame_march):
    """One view's 3072 second-tier rays fit: render_views of one pose equals render() and the oracle."""
    exp = view_expected(0)
    cam = camera("views")
    single = cam.render(0, want_ray_rgba=True)
    assert_exact(single, [int(v) for v in single.stats], exp, frame_march)
    cam.fast_draws = 32
    got = cam.render_views(VIEW_POSES[:1], want_ray_rgba=True)
    assert len(got) == 1
    assert_view_exact(got[0], exp)
    stats = [int(v) for v in got[0].stats]
    print("views 1", frame_march, stats[8:11])
    assert stats[:12] == [int(v) for v in single.stats[:12]] and stats[S_EXHAUSTED] == 0
    assert stats[S_RETRACED] == int((exp["draws"] > D32).sum()) and cam.fast_draws == 64   # (many re-traced at 32: 64 from now on)
    assert np.array_equal(got[0].image_u8.cpu().numpy(), single.image_u8.cpu().numpy())


@gpu
def test_views_two_poses_in_one_launch_overflow(frame_march):
    """Two views in one launch hold 6144 second-tier rays: 4096 find room, the batch retries with 64 draws and raises."""
    from python_raytracer_amd import _native as nat
    figs = [figures(oracle_frame("views", v)) for v in (0, 1)]
    total, n113 = sum(f["rays"] for f in figs), sum(f["n113"] for f in figs)
    cam = camera("views")
    for fast in (32, 64):
        cam.fast_draws = fast
        got = cam.render_views(VIEW_POSES[:2], want_ray_rgba=True, check=False)
        stats = device_stats(got[0])
        print("views 2", frame_march, fast, figs, stats[8:11])
        assert stats[S_EXHAUSTED] == n113 - CAP2 and stats[S_RAYS] + stats[S_EXHAUSTED] == total, (stats, figs)
        assert stats[S_RETRACED] == sum(f["n32" if fast == 32 else "n64"] for f in figs) - stats[S_EXHAUSTED], (stats, figs)
        done = 0
        for v in (0, 1):
            exp = view_expected(v)
            same = got[v].ray_rgba.cpu().numpy().view(np.uint32)[exp["slot"]] == packed(exp["rays"])
            assert same[exp["draws"] <= D113].all()
            done += int(same[exp["draws"] > D113].sum())
        assert done >= CAP2, done
    cam.fast_draws = 32
    with pytest.raises(nat.VrtError) as err:
        cam.render_views(VIEW_POSES[:2])
    assert cam.fast_draws == 64 and str(err.value).startswith("%d rays of the batch could not be completed" % (n113 - CAP2)), str(err.value)


def _views_child():
    """Run in a child process with VRT_BATCH_LOG2=12: a launch of a batch is then one view of 3072 slots."""
    cam = camera("views")
    got = cam.render_views(VIEW_POSES, want_ray_rgba=True)
    for v, r in enumerate(got):
        assert_view_exact(r, view_expected(v))
    print("VIEWS", " ".join(str(int(v)) for v in got[0].stats[8:11]))


@gpu
def test_views_one_view_per_launch_completes(frame_march):
    """The same poses, and a third, one view per launch: each launch's lists hold its view, and the batch completes, every
    view the oracle's single frame."""
    figs = [figures(oracle_frame("views", v)) for v in range(len(VIEW_POSES))]
    words = run_children("import test_gpu_draw_limits as t; t._views_child()", [{"VRT_BATCH_LOG2": "12"}], "VIEWS")[0]
    assert [int(w) for w in words[1:]] == [sum(f["rays"] for f in figs), sum(f["n32"] for f in figs), 0], (words, figs)


# ------------------------------------------------------------------------------------------------- 6. nonces
# what render() draws for a non-static frame: getrandbits(63) | 1 -- keys of two 32-bit words for init_by_array.  The
# largest such values; a fixed "random" one; and one under which the slot seeds of a frame -- slot + nonce -- straddle 2^32,
# so that one-word and two-word keys are seeded side by side.
NONCES = {"top": ((1 << 63) - 25) | 1, "random": 0x5bd1e9955bd1e995 >> 1 | 1, "straddle": ((1 << 32) - 1000) | 1}


def test_nonces_are_what_render_draws():
    for name, n in NONCES.items():
        assert n & 1 and n < 1 << 63, name
    assert NONCES["top"] >> 32 and NONCES["random"] >> 32
    # tier3's window has 13 824 slots: the first thousand of them are seeded with one-word keys, the others with two
    assert NONCES["straddle"] < 1 << 32 < NONCES["straddle"] + 2048 * 2


def nonstatic(st):
    return dict(st, static=False)


@gpu
@pytest.mark.parametrize("nonce", list(NONCES))
def test_retrace_tiers_under_a_nonce(frame_march, nonce):
    """The first 2048 pixels of tier3's window -- 4096 ray slots, so that both lists hold whatever the nonce's draws ask for
    -- in a re-seeded frame: rng_slots_kernel seeds the frame's rows and both re-trace tiers seed theirs under the nonce.
    All three tables are used (asserted from the oracle's draw counts); the frame equals the oracle's under the same nonce,
    through check_frame_march and its legs."""
    n = NONCES[nonce]
    sc, st, lens = limit_scene("tier3")
    px = np.ascontiguousarray(frame_pixels("tier3")[:2048])
    o = oracle_frame("tier3", seed_nonce=n, pixels=px)
    fig = figures(o)
    assert fig["rays"] <= CAP2 and fig["n32"] >= fig["n113"] > 0 and fig["n1024"] == 0, fig
    if nonce == "straddle":
        seeds = (o["rays"]["y"].astype(np.int64) * st["width"] + o["rays"]["x"]) * st["samples"] + o["rays"]["s"] + n
        assert (seeds < 1 << 32).any() and (seeds >= 1 << 32).any()
    cam = camera_for(sc, settings_store(nonstatic(st)), POS, IDENTITY, lens)
    r = check_frame_march(cam, o, CS, frame_march, pixels=px, seed_nonce=n)
    assert int(r.stats[S_RAYS]) == fig["rays"] and int(r.stats[S_EXHAUSTED]) == 0 and int(r.stats[S_RETRACED]) == fig["n32"], (r.stats, fig)


SPARSE = {"res2": (1, 2, 139, (1.5, 2.25, -3.5)), "res3": (2, 3, 136, (-2.5, 1.25, 3.5))}   # (tests/test_gpu_pool_passes.py's worlds)


@gpu
@pytest.mark.parametrize("nonce", list(NONCES))
@pytest.mark.parametrize("world", list(SPARSE))
def test_per_pixel_ray_table_under_a_nonce(frame_march, world, nonce):
    """A sparse world at resolutions <= 2 and at 3 on the settings that give one ray record per pixel (dof, lod_random and
    lod_samples 0): raygen_tile_kernel's table and the march that reads a ray's first draws from the draw table, in a
    re-seeded frame, against the oracle under the same nonce."""
    n = NONCES[nonce]
    seed, res_max, dist_max, pos = SPARSE[world]
    key = ("sparse", world, n)
    sc = sparse_scene(seed, res_max, 8)
    st = ol.make_settings(width=64, height=48, samples=2, chunk_size=8, dist_max=dist_max, max_bounces=4.0, static=False,
                          dof=0.0, lod_random=0.0, lod_samples=0.0)
    lens = st["fov"] * np.pi / 8
    if key not in _oracle:
        _oracle[key] = ol.render(sc, st, np.array(pos), IDENTITY, lens, ol.pixel_lists(64, 48, 1)[0], libm=ol.LIBM_PORTABLE, seed_nonce=n)
    o = _oracle[key]
    assert len(o["rays"]) > 4096 and int(o["counters"][ol.COUNTERS.index("hit")]) > 0
    if nonce == "straddle":
        assert 64 * 48 * 2 > 1000                 # slots either side of 2^32
    cam = camera_for(sc, settings_store(st), np.array(pos), IDENTITY, lens)
    r = check_frame_march(cam, o, 8, frame_march, seed_nonce=n)
    assert int(r.stats[S_RAYS]) == len(o["rays"]) and int(r.stats[S_EXHAUSTED]) == 0
