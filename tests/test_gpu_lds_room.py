"""GPU tests where LDS room decides what a frame-march launch keeps beside the march: 255 materials, chunk tables of 4096
cells and one row more, and scenes placed between the byte thresholds at which the ray pool gives up the settled bitmap,
then the world-axis tables, then itself.  "Never changes a result" (include/vrt.h, VRT_S_POOL_GROUPS) is the contract:
every case is bit-exact against the CPU oracle in its portable-libm mode under the four frame_march legs, proves from the
oracle's output alone that it reached its edge, and checks what the launch says it chose (vrt_diag_last_plan) against the
case's name and against arithmetic on the reported bytes.

The byte thresholds rest on each kernel's static LDS, which only the compiler knows.  From the compiler's resource report
of the shipped source (-Rpass-analysis=kernel-resource-usage, the command of tests/test_kernel_resources.py; `LDS Size
[bytes/block]`): every march_kernel / march_pool_kernel instance without the look-ahead has 8032 bytes, every look-ahead
instance (W) 4976.  tests/test_kernel_resources.py::test_static_lds_of_the_frame_kernels pins both on the CPU.  With
160 KiB / VRT_WAVES_PER_SIMD = 40960 bytes per workgroup and 27648 + 16 bytes of pools, the pool fits while
    align16(64 materials + 4 table cells in LDS + 4 bitmap words) [+ world tables] <= 40960 - 27664 - static:
    5264 bytes without the look-ahead, 8320 with it."""
import hashlib
import os

import numpy as np
import pytest

import oracle_lib as ol
from gpu_util import (BUDGET_LDS, POOL_LDS, STATIC_LDS, active, camera_for, check_frame_march, march_dyn_lds, run_children,
                      settings_store)
from edge_scenes import CNT, voxel_ids_at
from test_gpu_edges import RAY_FIELDS

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True, params=["pool", "lanes", "pool-ahead", "lanes-ahead"])
def frame_march(request, monkeypatch):
    """As in tests/test_gpu_edges.py: both frame kernels asked for, each with and without the look-ahead across chunk
    borders (VRT_WADDR=1: the world-axis tables in LDS); tests marked `one_march` run once."""
    if request.node.get_closest_marker("one_march") and request.param != "pool":
        pytest.skip("runs once")
    monkeypatch.setenv("VRT_POOL", "1" if request.param.startswith("pool") else "0")
    monkeypatch.setenv("VRT_POOL_MIN_RAYS", "0")
    monkeypatch.setenv("VRT_WADDR", "1" if request.param.endswith("-ahead") else "0")
    return request.param


CS = 8
SMALL_ROT = tuple(np.array([0.1, -0.2, 0.05, 0.97]) / np.linalg.norm([0.1, -0.2, 0.05, 0.97]))   # velocity bound 1.4459
Y90 = (0.0, float(np.sin(np.pi / 4)), 0.0, float(np.cos(np.pi / 4)))                               # velocity bound 1: looks along x
MATS4 = np.array([[200, 40, 40, 0.0, 0.5, 0.0, 0.0], [40, 200, 40, 0.5, 1.0, 0.75, 0.0], [40, 40, 200, 0.1, 0.25, 0.25, 0.5],
                  [220, 220, 220, 1.0, 2.0, 1.0, 0.0]])


def mats_n(n, seed=2550):
    """n materials of moderate properties: random albedo, roughness 0..1, absorption 0.25..2, ior 0..1, some that emit."""
    rng = np.random.default_rng(seed)
    m = np.zeros((n, 7))
    m[:, :3] = rng.integers(0, 256, (n, 3))
    m[:, 3] = np.resize([0.0, 0.1, 0.5, 1.0], n)
    m[:, 4] = np.resize([0.25, 1.0, 0.5, 2.0, 1.0], n)
    m[:, 5] = np.resize([0.0, 0.25, 0.5, 0.75, 1.0, 0.0], n)
    m[:, 6] = np.resize([0.0, 0.0, 0.5], n)
    return m


# What a launch keeps, per frame_march leg: (kernel, settled bitmap, world tables).  The four patterns the cases take:
def _legs(pool, pool_ahead):
    return {"pool": pool, "lanes": ("lanes", "box", False), "pool-ahead": pool_ahead, "lanes-ahead": ("lanes", "box", True)}


NO_POOL = _legs(("lanes", "box", False), ("lanes", "box", True))                    # the pool cannot fit; march_kernel keeps its bitmap
POOL_NO_BITMAP = _legs(("pool", "none", False), ("pool", "none", True))             # the pool fits once the bitmap is given up
NOTHING = {leg: ("lanes", "none", leg.endswith("-ahead")) for leg in NO_POOL}        # no pool, no bitmap, no window

# Every case: one resource at its limit, the rest moderate.  40 x 30 x 2 samples, max_bounces 4, chunk size 8; a camera
# rotated by SMALL_ROT with dist_max 92 has a traversed box of 39^3 = 59319 cells: 1854 bitmap words, 7416 bytes (a box of
# 32 cells and more a side could have the 4 KiB window instead); Y90 with dist_max 64 one of 21^3 = 9261: 290 words, 1160 bytes.
#   A = 64 materials + 4 table cells in LDS.  wt = 4 * (world cells + 64) summed over the axes.
# The comments give the bytes each placement rests on, then what the oracle alone gives for the case.
ROOM_CASES = {
    # A = 16320 + 256 = 16576 > 5264 by 11312: no pool.  march_kernel: 8032 + 16576 + 7416 + 2048 + 64 = 34136 <= 40960: bitmap.
    # oracle: 2400 rays, 3272 hits; the 904 rays that ended in a hit did so on 117 distinct ids, 469 of them on ids >= 128, 26 on id 255
    "mats255": dict(seed=3, dims=(4, 4, 4), mats=255, fill=0.08, expect=NO_POOL),
    # 4096 cells: the table's 16384 bytes are in LDS.  A = 256 + 16384 = 16640 > 5264: no pool either (the issue of this
    # module expected one: 8032 + 16640 + 27664 = 52336 bytes allow three workgroups).  march_kernel: 34200 <= 40960: bitmap.
    # oracle: 2400 rays, 2297 hits; 61 of the 591 traversed chunks in row 15 of the 16-long axis, 202 rays ended in a hit there
    "table4096": dict(seed=2, dims=(16, 16, 16), mats=4, fill=0.04, present=0.85, at=(0.93, 0.5, 0.45), expect=NO_POOL),
    # the same world one row larger: 4352 cells, read from memory.  A = 256: with the bitmap 7672 > 5264 by 2408, without
    # 256 <= 5264; look-ahead (wt 2336): 10008 > 8320 by 1688, without the bitmap 2592 <= 8320.
    # oracle: 2400 rays, 2324 hits; 44 of the 586 traversed chunks in row 16 of the 17-long axis, 21 rays ended in a hit there
    "table4352": dict(seed=2, dims=(17, 16, 16), mats=4, fill=0.04, present=0.85, at=(0.93 * 16 / 17, 0.5, 0.45), expect=POOL_NO_BITMAP),
    # A = 16320 + 16384 = 32704: march_kernel's room for a bitmap or a window is 40960 - 2048 - 8032 - 32704 - 64 = -1888
    # (look-ahead, wt 2304: 40960 - 2048 - 4976 - 32704 - 2304 - 64 = -1136); its dynamic LDS is 32720 / 35024 bytes.
    # oracle: 2400 rays, 3151 hits; 1343 rays ended in a hit, on 224 distinct ids, 797 of them on ids >= 128, 2 on id 255
    "mats255_table4096": dict(seed=4, dims=(16, 16, 16), mats=255, fill=0.04, present=0.85, at=(0.93, 0.5, 0.45), expect=NOTHING),
    # 40 materials, 18 cells: A = 2632.  With the bitmap 10048 > 5264 by 4784; without 2632 <= 5264 by 2632.  Look-ahead
    # (wt 1024): 11072 > 8320 by 2752; without the bitmap 3656 <= 8320 by 4664.
    # oracle: 2400 rays, 2469 hits
    "pool_no_bitmap": dict(seed=5, dims=(3, 2, 3), mats=40, fill=0.1, expect=POOL_NO_BITMAP),
    # 12 materials, a tube of 200 x 2 x 1 chunks (dense layout): A = 768 + 1600 = 2368, bitmap 1160, wt 4 * (1600 + 16 + 8
    # + 192) = 7264.  Look-ahead: 2368 + 1168 + 7264 = 10800 > 8320 by 2480; without the bitmap 9632 > 8320 by 1312; without
    # the tables (the kernel of 8032 bytes again) 3528 <= 5264 by 1736: the pool keeps the bitmap and gives the tables up.
    # oracle: 2400 rays, 3032 hits
    "pool_no_tables": dict(seed=6, dims=(200, 2, 1), mats=12, fill=0.1, rot=Y90, dist_max=64, at=(0.5, 0.5, 0.5),
                           expect=_legs(("pool", "box", False), ("pool", "box", False))),
    # 150 materials, 18 cells: A = 9672 > 5264 by 4408 with nothing else in LDS; look-ahead (wt 1024): 10696 > 8320 by 2376
    # without the bitmap (110 materials would still fit there: 4976 + 7112 + 1024 + 27664 = 40776): everything is given up;
    # march_kernel keeps the bitmap (8032 + 9672 + 7416 + 2112 = 27232 <= 40960).
    # oracle: 2400 rays, 2803 hits
    "no_pool": dict(seed=7, dims=(3, 2, 3), mats=150, fill=0.1, expect=NO_POOL),
}
ROOM_DEFAULTS = dict(present=0.85, res=(1, 2), rot=SMALL_ROT, dist_max=92, at=(0.45, 0.55, 0.4), st={})

_scenes, _oracle = {}, {}


def build_scene(c):
    """(scene, settings, camera position, rotation, lens) of a case dict; deterministic."""
    c = dict(ROOM_DEFAULTS, **c)
    rng = np.random.default_rng(c["seed"])
    dims = np.array(c["dims"])
    st = ol.make_settings(**dict(dict(width=40, height=30, samples=2, max_bounces=4.0, chunk_size=CS, dist_max=c["dist_max"]), **c["st"]))
    origin = -(dims // 2) * CS
    pos = np.floor(origin + np.array(c["at"]) * dims * CS) + np.array([0.3, 0.6, 0.45])
    # (drawn for 17 rows, whatever the world's: `table4352` is `table4096` with one row more)
    full = dims.copy()
    if tuple(dims[1:]) == (16, 16):
        full[0] = 17
    present = (rng.random(tuple(full)) < c["present"]).astype(np.uint8)[:dims[0]]
    res = rng.integers(c["res"][0], c["res"][1] + 1, tuple(full)).astype(np.uint8)[:dims[0]]
    present[tuple(((np.floor(pos) - origin) // CS).astype(np.int64))] = 1
    mats = (MATS4 if c["mats"] == 4 else mats_n(c["mats"])) if isinstance(c["mats"], int) else np.asarray(c["mats"], np.float64)
    shape = tuple(full * CS)
    ids = rng.integers(1, len(mats) + 1, shape)
    grid = np.where(rng.random(shape) < c["fill"], ids, 0).astype(np.uint8)[:dims[0] * CS]
    assert len(np.unique(grid)) == len(mats) + 1                       # every id is placed
    sc = ol.Scene(origin, dims, CS, present, res, ol.Scene.camera_grid(grid, origin, dims, CS, present, res), mats)
    return sc, st, pos, np.array(c["rot"]), st["fov"] * np.pi / 8


def room_scene(name):
    if name not in _scenes:
        _scenes[name] = build_scene(ROOM_CASES[name])
    return _scenes[name]


def room_oracle(name, pixels):
    """The oracle's frame of a case: computed once, shared by the frame_march legs and the one_march tests, never modified."""
    if name not in _oracle:
        sc, st, pos, q, lens = room_scene(name)
        _oracle[name] = ol.render(sc, st, pos, q, lens, pixels, libm=ol.LIBM_PORTABLE)
    return _oracle[name]


def room_proof(name, o):
    """Does the oracle's frame reach the edge the case is named after?  The figures of the comments of ROOM_CASES."""
    sc = room_scene(name)[0]
    rays = o["rays"]
    cnt = rays["counters"]
    fig = dict(rays=len(rays), hits=int(cnt[:, CNT["hit"]].sum()))
    assert fig["hits"] > 0
    broke = rays[cnt[:, CNT["broke"]] == 1]
    if len(sc.materials) == 255:
        ids = voxel_ids_at(sc, broke["pos"])[0]
        assert (ids > 0).all()
        fig.update(ended_in_hit=len(ids), distinct=len(set(ids.tolist())), from_128=int((ids >= 128).sum()), on_255=int((ids == 255).sum()))
        assert fig["distinct"] >= 100 and fig["from_128"] > 0 and fig["on_255"] > 0, fig
    if name.startswith("table"):
        last = int(sc.dims[0]) - 1
        row = lambda p: (np.floor(np.asarray(p, np.float64)[:, 0]).astype(np.int64) - int(sc.origin[0])) // CS
        fig["trav_last_row"] = int((row(o["traversed"]) == last).sum())
        fig["ended_in_hit_last_row"] = int((row(broke["pos"]) == last).sum())
        assert sc.present[last].any() and fig["trav_last_row"] > 0 and fig["ended_in_hit_last_row"] > 0, fig
        assert int(np.prod(sc.dims)) == (4096 if name == "table4096" else 4352)
        # no identity table: chunks are missing and resolutions differ
        assert (sc.present == 0).any() and set(np.unique(sc.res[sc.present != 0])) == {1, 2}
    return fig


def trav_words(r):
    return (int(np.prod(r.trav_dims)) + 31) // 32


def check_plan(name, leg, cam, r, plan):
    """What the launch of record-less frame `r` reported (vrt_diag_last_plan) against the case's name, and against
    arithmetic on the reported bytes -- the layout of march_lds restated (gpu_util.march_dyn_lds), not the library's word."""
    sc = room_scene(name)[0]
    kernel, bitmap, tables = ROOM_CASES[name]["expect"][leg]
    words = trav_words(r)
    assert int(np.prod(r.trav_dims)) <= 65536                          # (a box that may have a bitmap of its own)
    cells = int(np.prod(sc.dims))
    ct = cells if cells <= 4096 else 0
    wt_cells = [int(d) * CS for d in sc.dims]
    assert plan["n_materials"] == len(sc.materials) and plan["ct_cells"] == ct
    # 1. what the case is named after; the pool and the tables cross-checked against the kernels' own counts
    assert plan["pool"] == (kernel == "pool"), plan
    assert (int(r.stats[12]) & 0xffffffff > 0) == (kernel == "pool")
    assert plan["wt_on"] == int(tables), plan
    assert (int(r.stats[14]) > 0) == tables
    assert plan["trav_words"] == (words if bitmap == "box" else 0) and plan["bm_window"] == -1, plan
    # 2. the bytes: the dynamic LDS is the documented layout, the static LDS the compiler's
    W = bool(plan["wt_on"])
    assert plan["static_bytes"] == STATIC_LDS[W]
    assert plan["dyn_bytes"] == march_dyn_lds(len(sc.materials), ct, plan["trav_words"], wt_cells if W else None, bool(plan["pool"]))
    if plan["pool"]:
        assert plan["static_bytes"] + plan["dyn_bytes"] <= BUDGET_LDS
    # 3. the configurations the planner asked the runtime about: in the order bitmap, then tables, then the pool; each
    # rejected one exceeds the budget, the accepted one does not, and none that would have fitted was passed over
    if leg.startswith("pool"):
        ahead = leg.endswith("-ahead")
        # (the planner starts from what march_kernel would keep: a bitmap only where its 2 KiB of margin allow one)
        given = STATIC_LDS[ahead] + march_dyn_lds(len(sc.materials), ct, words, wt_cells if ahead else None, False) + 2048 + 64 <= BUDGET_LDS
        richer = [(w, b) for w in ([True, False] if ahead else [False]) for b in ((words, 0) if given else (0,))]
        want = []
        for w, b in richer:
            total = STATIC_LDS[w] + march_dyn_lds(len(sc.materials), ct, b, wt_cells if w else None, True)
            want.append((w, b, total))
            if total <= BUDGET_LDS:
                break
        assert len(plan["probes"]) == len(want), (plan, want)
        for p, (w, b, total) in zip(plan["probes"], want):
            assert (p["wt_on"], p["trav_words"], p["static_bytes"] + p["dyn_bytes"]) == (int(w), b, total), (p, w, b, total)
            assert abs(total - BUDGET_LDS) >= 1024, (name, total)       # (no case sits on a threshold)
            assert (p["groups_per_cu"] >= 4) == (total <= BUDGET_LDS), p
        fitted = want[-1][2] <= BUDGET_LDS
        assert fitted == bool(plan["pool"])
        if fitted:
            assert (plan["wt_on"], plan["trav_words"], plan["static_bytes"] + plan["dyn_bytes"]) == (int(want[-1][0]), want[-1][1], want[-1][2])
    else:
        assert plan["probes"] == []
    if not plan["pool"]:
        # march_kernel keeps the bitmap while 2 KiB and 64 bytes of margin remain (fill_params), and only then
        with_bitmap = STATIC_LDS[W] + march_dyn_lds(len(sc.materials), ct, words, wt_cells if W else None, False)
        assert abs(with_bitmap + 2048 + 64 - BUDGET_LDS) >= 1024
        assert (plan["trav_words"] != 0) == (with_bitmap + 2048 + 64 <= BUDGET_LDS), (plan, with_bitmap)
        if name == "mats255_table4096":     # ... nor is there room for the 4 KiB window its box could have
            assert min(r.trav_dims) >= 32
            assert plan["static_bytes"] + plan["dyn_bytes"] + 4096 + 2048 + 64 - BUDGET_LDS >= 1024
            assert plan["dyn_bytes"] == (35024 if W else 32720)


# ------------------------------------------------------------------------------------------------- 1. the frames
@pytest.mark.parametrize("case", list(ROOM_CASES))
def test_lds_room_scene_bit_exact(case, frame_march):
    """Every field of every ray record, the fp32 means, the traversed list and the counters against the oracle; the
    record-less frame and what its launch chose (check_plan); its three re-renders (check_frame_march, told which kernel
    the case runs under this leg); and the proof from the oracle's frame alone that the case reached its edge."""
    from python_raytracer_amd import _native as nat
    sc, st, pos, q, lens = room_scene(case)
    cam = camera_for(sc, settings_store(st), pos, q, lens)
    r = cam.render(0, want_rays=True)
    o = room_oracle(case, r.pixels)
    got, exp = active(r), o["rays"]
    assert len(got) == len(exp) == int(r.stats[8]) == o["n_rays"]
    for f in RAY_FIELDS:
        assert np.array_equal(got[f], exp[f]), (f, np.flatnonzero((got[f] != exp[f]).reshape(len(got), -1).any(1))[:5])
    assert np.array_equal(r.rgba_f32.cpu().numpy(), o["pix_mean"].astype(np.float32))
    assert np.array_equal(np.array(r.traversed(CS), np.int64).reshape(-1, 3), o["traversed"])
    assert (r.stats[:8] == o["counters"]).all(), (r.stats[:8], o["counters"])
    before = nat.last_plan()["launches"]
    r1 = cam.render(0, want_ray_rgba=True)
    plan = nat.last_plan()
    assert plan["launches"] > before                                  # (the frame's march; its re-traces are not recorded)
    print(case, frame_march, plan)
    check_plan(case, frame_march, cam, r1, plan)
    kernel = ROOM_CASES[case]["expect"][frame_march][0]
    check_frame_march(cam, o, CS, frame_march, lookahead=ROOM_CASES[case]["expect"][frame_march][2], expect_pool=(kernel == "pool"))
    print(case, room_proof(case, o))


# ------------------------------------------------------------------------------------------------- 2. the other kernels
@pytest.mark.one_march
@pytest.mark.parametrize("case", ["mats255_table4096", "table4352"])
def test_first_hit_at_the_limits(case):
    """Camera.first_hit (first_hit_kernel shares the prologue: chunk table in LDS or from memory) against the oracle's
    first-hit entry, as tests/test_gpu_first_hit.py does; with 255 materials `material` goes up to 255 and is negative
    for unused slots only."""
    from test_gpu_first_hit import check_against_oracle
    sc, st, pos, q, lens = room_scene(case)
    cam, h, exp = check_against_oracle(sc, st, pos, q, lens)
    got = h.numpy()
    assert np.array_equal(got["material"] < 0, exp["material"] == -1) and (got["material"] >= -1).all()
    if case.startswith("mats255"):
        assert int(got["material"].max()) == 255 and int((got["material"] >= 128).sum()) > 100
        assert len(set(got["material"][got["material"] > 0].tolist())) >= 100


@pytest.mark.one_march
def test_render_views_255_materials_table4096():
    """Camera.render_views (march_views_kernel: materials and chunk table beside its view records) of three poses: every
    view equals Camera.render at that pose, view 0 equals the oracle."""
    from test_gpu_views import assert_view_equals_single, set_pose, singles
    sc, st, pos, q, lens = room_scene("mats255_table4096")
    poses = [(tuple(pos), tuple(q)), (tuple(pos + np.array([-9.0, 3.0, 5.5])), (0.0, 0.0, 0.0, 1.0)), (tuple(pos + np.array([2.0, -11.0, -7.25])), Y90)]
    cam = camera_for(sc, settings_store(st), pos, q, lens)
    ref = singles(cam, poses)
    got = cam.render_views(poses, want_ray_rgba=True)
    assert len(got) == 3
    for b, s in zip(got, ref):
        assert int(s.stats[4]) > 0
        assert_view_equals_single(b, s, CS)
    o = room_oracle("mats255_table4096", got[0].pixels)
    assert np.array_equal(got[0].rgba_f32.cpu().numpy(), o["pix_mean"].astype(np.float32))
    slot, want = packed_colours(o, got[0])
    assert np.array_equal(got[0].ray_rgba.cpu().numpy().view(np.uint32)[slot], want)
    assert np.array_equal(np.array(got[0].traversed(CS), np.int64).reshape(-1, 3), o["traversed"])


@pytest.mark.one_march
def test_trace_many_255_materials():
    """Camera.trace_many (vrt_trace_rays) on every ray of the `mats255` frame, each fed its own draw stream: the records equal
    the oracle's rays (tile() consumed the lod_random draw: the rows start at the second draw, the draw counters are one
    lower), as in tests/test_gpu_edges.py::test_trace_many_equals_the_tiles_own_rays."""
    sc, st, pos, q, lens = room_scene("mats255")
    cam = camera_for(sc, settings_store(st), pos, q, lens)
    exp = room_oracle("mats255", cam.render(0, check=False).pixels)["rays"]
    n = len(exp)
    assert n % 256 != 0 and n > 1024
    W, H = st["width"], st["height"]
    dx = [-1 + (int(x) / W) * 2 for x in exp["x"]]
    dy = [-1 + (int(y) / H) * 2 for y in exp["y"]]
    nd = int(exp["counters"][:, CNT["draw"]].max()) + 1
    draws = np.stack([ol.rng_draws((1 + int(x)) * (1 + int(y)) * (1 + int(s)), nd + 1)[1:] for x, y, s in zip(exp["x"], exp["y"], exp["s"])])
    cam.trace_many(dx, dy, [float(d) for d in exp["detail"]], draws=draws)
    rec = cam.last_trace_records
    assert len(rec) == n
    for f in ("color", "energy", "step", "life", "bounces", "pos", "vel"):
        assert np.array_equal(rec[f], exp[f]), (f, np.flatnonzero((rec[f] != exp[f]).reshape(n, -1).any(1))[:5])
    want = exp["counters"].copy()
    want[:, CNT["draw"]] -= 1
    assert np.array_equal(rec["counters"], want)


# ------------------------------------------------------------------------------------------------- 3. the pow memo
# 255 rough materials whose absorptions are 255 distinct values in [0.05, 2]; a bounce budget of 8; lod_bounces 0, so that a
# hit does not shorten the ray.  A ray's `bounces` is the sum of the absorptions it met, and 1 + bounces the base of the next
# hit's pow: the memo (256 slots, 4 probes, insert-only, one per device and falloff) is shown more bases than it has slots.
# oracle: scene A 2400 rays, 7237 hits, 652 distinct non-zero final `bounces`; scene B 2672 hits, 415
POW_FALLOFF = 0.4375      # (no other test renders with it: the device's table for it starts empty)
POW_SCENES = {"A": dict(seed=11, dims=(4, 4, 4), mats=255, fill=0.3, st=dict(max_bounces=8.0, lod_bounces=0.0, falloff=POW_FALLOFF)),
              "B": dict(seed=12, dims=(4, 4, 4), mats=255, fill=0.2, at=(0.55, 0.4, 0.5), st=dict(max_bounces=8.0, lod_bounces=0.0, falloff=POW_FALLOFF))}


def pow_mats():
    m = mats_n(255, seed=2551)
    m[:, 3] = 1.0
    m[:, 4] = np.linspace(0.05, 2.0, 255)
    assert len(set(m[:, 4].tolist())) == 255
    return m


def pow_scene(which):
    if ("pow", which) not in _scenes:
        _scenes[("pow", which)] = build_scene(dict(POW_SCENES[which], mats=pow_mats()))
    return _scenes[("pow", which)]


def pow_oracle(which, pixels):
    if ("pow", which) not in _oracle:
        sc, st, pos, q, lens = pow_scene(which)
        o = ol.render(sc, st, pos, q, lens, pixels, libm=ol.LIBM_PORTABLE)
        bases = np.unique(o["rays"]["bounces"])
        o["distinct_bases"] = int((bases != 0).sum())
        assert o["distinct_bases"] > 256, o["distinct_bases"]
        _oracle[("pow", which)] = o
    return _oracle[("pow", which)]


def packed_colours(o, r):
    """(slots, colours): the oracle's per-sample colours as Camera.render packs them, and the slot p * max_samples + s of each."""
    rays = o["rays"]
    where = {(int(x), int(y)): i for i, (x, y) in enumerate(r.pixels)}
    slot = np.array([where[(int(x), int(y))] for x, y in zip(rays["x"], rays["y"])], np.int64) * r.max_samples + rays["s"]
    return slot, (rays["color"][:, 0].astype(np.uint32) | (rays["color"][:, 1].astype(np.uint32) << 8) |
                  (rays["color"][:, 2].astype(np.uint32) << 16) | (rays["alpha"].astype(np.uint32) << 24))


def pow_frame(which):
    """Render a pow scene (record-less: the frame kernel the leg names, if it fits) and hold it against the oracle; returns
    the digest of its packed colours."""
    sc, st, pos, q, lens = pow_scene(which)
    cam = camera_for(sc, settings_store(st), pos, q, lens)
    r = cam.render(0, want_ray_rgba=True)
    o = pow_oracle(which, r.pixels)
    slot, want = packed_colours(o, r)
    got = r.ray_rgba.cpu().numpy().view(np.uint32)[slot]
    assert np.array_equal(got, want), which
    assert np.array_equal(r.rgba_f32.cpu().numpy(), o["pix_mean"].astype(np.float32)), which
    assert (r.stats[:8] == o["counters"]).all(), (which, r.stats[:8], o["counters"])
    assert np.array_equal(np.array(r.traversed(CS), np.int64).reshape(-1, 3), o["traversed"]), which
    return hashlib.sha256(got.tobytes()).hexdigest()


def test_pow_memo_beyond_its_capacity(frame_march):
    """More distinct pow bases than the memo has slots, on a table that starts empty: the first frame fills it and overflows
    it, the second finds it full, a different scene with the same falloff meets the first scene's entries.  All bit-exact."""
    import python_raytracer_amd as pra
    try:
        first = pow_frame("A")
        assert pow_frame("A") == first
        pow_frame("B")
        assert pow_frame("A") == first
    finally:
        pra.release_caches()


def _pow_child():
    print("POWMEMO", pow_frame("A"), pow_frame("B"))


@pytest.mark.one_march
def test_pow_memo_per_frame_gives_the_same_colours():
    """The same two scenes in a fresh process with VRT_POW_MEMO=frame (read once per process: every frame memoises into its
    own workspace): the packed per-sample colours are those of this process, which uses the per-device table."""
    import python_raytracer_amd as pra
    assert os.environ.get("VRT_POW_MEMO", "") == ""
    try:
        here = [pow_frame("A"), pow_frame("B")]
    finally:
        pra.release_caches()
    lines = run_children("import test_gpu_lds_room as t; t._pow_child()", [{"VRT_POW_MEMO": "frame"}], "POWMEMO")
    assert lines[0][1:] == here
