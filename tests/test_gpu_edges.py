"""GPU tests at the edges of the input ranges, and of the set-up kernels on their own.

tests/test_gpu_parity.py::test_random_scenes_bit_exact draws moderate inputs; the hand-run soaks (tests/soak) draw much
wider ones.  This module pins the wide ends as small fixed scenes, one edge per scene with the rest kept moderate, so that
a failure names its cause: chunk size 64, worlds 2^26 and 2^27 cells from the origin, the largest coordinates the range
check of vrt_render_tile accepts, Frame resolutions up to 9, 179 and 20 degree lenses, the extreme settings, one-pixel-wide
images; batches of explicit rays (vrt_trace_rays); vrt_select_chunks on random worlds; and the kernels that build the
world-axis offset tables, the occupancy words, the tile plan and the voxel blocks, each against numpy.
The reference of every GPU value is the CPU oracle in its portable-libm mode or plain numpy.  Every scene is checked on
the CPU first to reach the edge it is named after: each case asserts that from the oracle's output alone (EDGE_CASES,
in tests/edge_scenes.py, which holds the scene definitions)."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as ol
from edge_scenes import CNT, EDGE_CASES, IDENTITY, LIMIT, MATS4, edge_proof, edge_scene, limit_camera
from gpu_util import active, camera_for, check_frame_march, check_tile_plan, settings_store

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True, params=["pool", "lanes", "pool-ahead", "lanes-ahead"])
def frame_march(request, monkeypatch):
    """As in tests/test_gpu_parity.py: every test runs with both frame kernels (march_pool_kernel, march_kernel), each with
    the march step that stops its look-ahead at chunk borders and the one that looks across them (VRT_WADDR=1); tests
    marked `one_march` (they do not render frames) run once."""
    if request.node.get_closest_marker("one_march") and request.param != "pool":
        pytest.skip("runs once")
    monkeypatch.setenv("VRT_POOL", "1" if request.param.startswith("pool") else "0")
    monkeypatch.setenv("VRT_POOL_MIN_RAYS", "0")
    monkeypatch.setenv("VRT_WADDR", "1" if request.param.endswith("-ahead") else "0")
    return request.param


RAY_FIELDS = ("x", "y", "s", "color", "alpha", "counters", "ntrav", "detail", "energy", "step", "life", "bounces", "pos", "vel")

_oracle = {}


def edge_oracle(name, k, pixels):
    """The oracle's frame of camera k of a case: computed once, shared by the frame_march legs, never modified."""
    if (name, k) not in _oracle:
        sc, st, cams, lens = edge_scene(name)
        _oracle[(name, k)] = ol.render(sc, st, cams[k][0], cams[k][1], lens, pixels, libm=ol.LIBM_PORTABLE)
    return _oracle[(name, k)]


# ------------------------------------------------------------------------------------------------- 1. edge scenes
@pytest.mark.parametrize("case", list(EDGE_CASES))
def test_edge_scene_bit_exact(case, frame_march):
    """One input at the edge of its range per scene (EDGE_CASES), every field of every ray bit-exact against the oracle;
    then the frame march the fixture names (check_frame_march) and the proof, from the oracle's frame alone, that the
    scene reached its edge.  The far cases render a second time from an unrotated camera at an integer position.  The
    two limit_28 cases also assert that the camera one chunk farther out is refused by vrt_render_tile's range check."""
    from python_raytracer_amd import _native as nat
    from python_raytracer_amd.lib import vec3
    sc, st, cams, lens = edge_scene(case)
    cs = st["chunk_size"]
    for k, (pos, q) in enumerate(cams):
        cam = camera_for(sc, settings_store(st), pos, q, lens)
        r = cam.render(0, want_rays=True)
        o = edge_oracle(case, k, r.pixels)
        got, exp = active(r), o["rays"]
        assert len(got) == len(exp) == int(r.stats[8]) == o["n_rays"]
        for f in RAY_FIELDS:
            assert np.array_equal(got[f], exp[f]), (k, f, np.flatnonzero((got[f] != exp[f]).reshape(len(got), -1).any(1))[:5])
        assert np.array_equal(r.rgba_f32.cpu().numpy(), o["pix_mean"].astype(np.float32))
        assert np.array_equal(np.array(r.traversed(cs), np.int64).reshape(-1, 3), o["traversed"])
        assert (r.stats[:8] == o["counters"]).all(), (r.stats[:8], o["counters"])
        check_frame_march(cam, o, cs, frame_march)
        if k:
            assert int(exp["counters"][:, CNT["hit"]].sum()) > 0
    edge_proof(case, edge_oracle(case, 0, None))
    if case.startswith("limit_28"):
        sign = 1 if case.endswith("pos") else -1
        p, reach = limit_camera(sign, st)
        assert float(cam.pos.x) == p and abs(p) + reach == LIMIT - 0.5
        cam.pos = vec3(p + sign * cs, p, p)        # refused by fill_params, before anything of the frame is launched
        with pytest.raises(nat.VrtError) as err:
            cam.render(0)
        assert "vrt_render_tile" in str(err.value) and nat.lib().vrt_status_string(-1).decode() in str(err.value)
        cam.pos = vec3(p, p, p)                    # ... and the boundary itself still renders
        assert np.array_equal(cam.render(0).rgba_f32.cpu().numpy(), o["pix_mean"].astype(np.float32))


# ------------------------------------------------------------------------------------------------- 2. explicit rays
@pytest.mark.one_march
@pytest.mark.parametrize("case", ["cs64", "far_pos", "bounces16"])
def test_trace_many_equals_the_tiles_own_rays(case):
    """Camera.trace_many (vrt_trace_rays, raygen_explicit_kernel) on every ray of a frame at once -- a batch of several
    256-thread blocks whose size is no multiple of 256 -- each ray fed its own draw stream: the records equal the ORACLE's
    rays of the frame.  tile() consumed the lod_random draw before trace(), so the rows start at the second draw and the
    draw counters are one lower.  With the rows cut to the median draw count the rays that need more are counted in
    VRT_S_RNG_EXHAUSTED and the call raises.  (Camera.last_trace_records is only set by a call that returns, so there is
    nothing to compare after the raise.  The oracle has no entry that takes explicit draws, so the rule of include/vrt.h
    for rows shorter than the first hit's draws -- they read as 0.5 -- has no reference here and is not asserted.)"""
    from python_raytracer_amd import _native as nat
    sc, st, cams, lens = edge_scene(case)
    pos, q = cams[0]
    cam = camera_for(sc, settings_store(st), pos, q, lens)
    r = cam.render(0, want_rays=True)
    exp = edge_oracle(case, 0, r.pixels)["rays"]
    n = len(exp)
    assert n == len(active(r)) and n % 256 != 0 and n > 1024
    W, H = st["width"], st["height"]
    dx = [-1 + (int(x) / W) * 2 for x in exp["x"]]
    dy = [-1 + (int(y) / H) * 2 for y in exp["y"]]
    used = exp["counters"][:, CNT["draw"]].astype(np.int64)
    nd = int(used.max()) + 1
    draws = np.stack([ol.rng_draws((1 + int(x)) * (1 + int(y)) * (1 + int(s)), nd + 1)[1:]
                      for x, y, s in zip(exp["x"], exp["y"], exp["s"])])
    cam.trace_many(dx, dy, [float(d) for d in exp["detail"]], draws=draws)
    rec = cam.last_trace_records
    assert len(rec) == n
    for f in ("color", "energy", "step", "life", "bounces", "pos", "vel"):
        assert np.array_equal(rec[f], exp[f]), (f, np.flatnonzero((rec[f] != exp[f]).reshape(n, -1).any(1))[:5])
    want = exp["counters"].copy()
    want[:, CNT["draw"]] -= 1
    assert np.array_equal(rec["counters"], want)
    # (trace_many raises on VRT_S_RNG_EXHAUSTED != 0: having returned, it was 0)
    nd_short = int(np.median(used))
    assert nd_short >= 3 and (used - 1 > nd_short).any()
    with pytest.raises(nat.VrtError, match="more random draws than were supplied"):
        cam.trace_many(dx, dy, [float(d) for d in exp["detail"]], draws=draws[:, :nd_short])


# ------------------------------------------------------------------------------------------------- 3. chunk selection
def select_world(seed):
    """The draws of tests/soak/soak_select.py (chunk size 64 added); every fifth seed 2^20 chunks away from the origin."""
    rng = np.random.default_rng(seed)
    cs = int(rng.choice([8, 16, 32, 64]))
    dims = rng.integers(1, 7, 3)
    origin = (rng.integers(-4, 3, 3) * cs).astype(np.int64)
    if seed % 5 == 0:
        origin += np.array([1, -1, 1], np.int64) * (cs << 20)
    present = (rng.random(tuple(dims)) < 0.7).astype(np.uint8)
    pos = origin + rng.uniform(-0.5, 1.5, 3) * dims * cs
    dist_max = float(rng.choice([16, 48, 192, 1000]))
    lod = int(rng.choice([0, 1, 2, 5]))
    culling = bool(rng.integers(0, 2))
    ntr = int(rng.integers(0, 40))
    trav = (origin + rng.integers(-1, dims.max() + 1, (ntr, 3)) * cs).astype(np.float64)
    return cs, dims, origin, present, pos, dist_max, lod, culling, trav


SELECT_SEEDS = range(1, 61)


def select_coverage(seeds=SELECT_SEEDS):
    """What the oracle's selections of the seeds cover (conditions on the inputs, checked on the CPU)."""
    cov = dict(kept={False: 0, True: 0}, dropped={False: 0, True: 0}, lod0=0, lod_max=0, outside=0, far=0)
    for seed in seeds:
        cs, dims, origin, present, pos, dist_max, lod, culling, trav = select_world(seed)
        p0, r0 = ol.select_chunks(origin, dims, cs, present, pos, dist_max, lod, culling, trav)
        cov["kept"][culling] += int(p0.sum())
        cov["dropped"][culling] += int((p0 == 0).sum())
        cov["lod0"] += int((r0[p0 > 0] == 1).sum())
        cov["lod_max"] += int((r0[p0 > 0] == lod + 1).sum()) if lod else 0
        cell = (trav - origin) // cs
        cov["outside"] += int(((cell < 0) | (cell >= dims)).any(1).sum()) if len(trav) else 0
        cov["far"] += int(np.abs(origin).max() >= 8 << 20)
    return cov


@pytest.mark.one_march
def test_select_chunks_random_worlds():
    """Camera.chunk_update (vrt_select_chunks, select_chunks_kernel) over 60 random worlds, cameras and traversed lists
    against the oracle: chunk sizes 8..64, dims 1..6, dist_max 16..1000, chunk_lod 0..5, culling on and off, worlds 2^20
    chunks out.  Over the 60 seeds the oracle keeps 948 chunks and drops 449 with culling off, keeps 59 and drops 1602
    with it on; 488 kept chunks are at LOD 0 and 430 at a non-zero chunk_lod; 1056 traversed positions lie outside their
    world; 12 worlds are the far ones."""
    from python_raytracer_amd import Camera, PackedScene
    from python_raytracer_amd.lib import vec3, quaternion
    cov = select_coverage()
    assert all(cov["kept"][c] > 0 and cov["dropped"][c] > 0 for c in (False, True)), cov
    assert cov["lod0"] > 0 and cov["lod_max"] > 0 and cov["outside"] > 0 and cov["far"] > 0, cov
    for seed in SELECT_SEEDS:
        cs, dims, origin, present, pos, dist_max, lod, culling, trav = select_world(seed)
        p0, r0 = ol.select_chunks(origin, dims, cs, present, pos, dist_max, lod, culling, trav)
        sst = settings_store(ol.make_settings(width=8, height=8, chunk_size=cs, dist_max=dist_max, chunk_lod=lod))
        sst.culling = culling
        cam = Camera(settings=sst)
        grid = np.zeros(tuple(dims * cs), np.uint8)
        for c in np.argwhere(present):
            grid[tuple(c * cs)] = 1
        world = PackedScene.from_dense(origin, dims, cs, present, np.ones_like(present), grid, np.array([[1, 2, 3, 0, 1, 1, 0.0]]))
        cam.set_world_scene(world)
        cam.pos, cam.rot = vec3(*[float(v) for v in pos]), quaternion(*IDENTITY)
        table = cam.chunk_update([tuple(int(v) for v in t) for t in trav]).cpu().numpy().view(np.uint32).reshape(tuple(dims))
        assert np.array_equal((table != 0).astype(np.uint8), p0), seed
        assert np.array_equal((table >> 24).astype(np.uint8)[table != 0], r0[p0 > 0]), seed
        assert np.array_equal(table[table != 0] & 0xffffff, world.chunk_table.reshape(tuple(dims))[table != 0] & 0xffffff), seed


@pytest.mark.one_march
def test_select_chunks_from_device_keys_of_a_larger_traversed_box():
    """The previous frame's RenderResult as `traversed` (its device-side keys are read in place) on a chunk-size-8 world of
    3 x 2 x 3 chunks, much smaller than the traversed box round the camera (17 cells a side and more): culling keeps exactly
    the world chunks the oracle's frame traversed, at the oracle's LODs, for three frames in a row -- the first selection,
    with nothing traversed yet, keeps nothing, and its frame still records the chunk positions its rays cross."""
    from python_raytracer_amd import Camera, PackedScene
    from python_raytracer_amd.lib import vec3, quaternion
    rng = np.random.default_rng(301)
    cs, dims, origin = 8, np.array([3, 2, 3]), np.array([-8, -8, -16], np.int64)
    world_present = np.ones(tuple(dims), np.uint8)
    world_present[0, 1, 2] = 0
    grid = np.where(rng.random(tuple(dims * cs)) < 0.1, rng.integers(1, 5, tuple(dims * cs)), 0).astype(np.uint8)
    grid[:8, 8:, 16:] = 0
    st = ol.make_settings(width=32, height=24, samples=2, max_bounces=4.0, chunk_size=cs, dist_max=48, chunk_lod=2)
    sst = settings_store(st)
    sst.culling = True
    cam = Camera(settings=sst)
    cam.set_world_scene(PackedScene.from_dense(origin, dims, cs, world_present, np.ones_like(world_present), grid, MATS4))
    pos, q = np.array([3.3, -2.4, -13.5]), np.array([0.1, -0.2, 0.05, 0.97])
    cam.pos, cam.rot = vec3(*pos), quaternion(*q)
    prev, trav = None, np.zeros((0, 3))
    kept = []
    for frame in range(3):
        table = cam.chunk_update(prev).cpu().numpy().view(np.uint32).reshape(tuple(dims))
        pres, res = ol.select_chunks(origin, dims, cs, world_present, pos, 48, 2, True, trav)
        assert np.array_equal((table != 0).astype(np.uint8), pres) and np.array_equal((table >> 24).astype(np.uint8), res), frame
        kept.append(int(pres.sum()))
        r = cam.render(0)
        assert all(d > max(dims) for d in r.trav_dims)
        osc = ol.Scene(origin, dims, cs, pres, np.maximum(res, 1), ol.Scene.camera_grid(grid, origin, dims, cs, pres, np.maximum(res, 1)), MATS4)
        o = ol.render(osc, st, pos, q, cam.lens, r.pixels, libm=ol.LIBM_PORTABLE)
        assert np.array_equal(r.rgba_f32.cpu().numpy(), o["pix_mean"].astype(np.float32)), frame
        assert np.array_equal(np.array(r.traversed(cs), np.int64).reshape(-1, 3), o["traversed"]), frame
        prev, trav = r, o["traversed"].astype(np.float64)
    assert kept[0] == 0 and 0 < kept[1] < int(world_present.sum()) and kept[2] > 0, kept


# ------------------------------------------------------------------------------------------------- 4. set-up kernels
def voxel_offset_table(cs):
    """Byte offset of every cell (lx, ly, lz) of a chunk block in the bricked order of include/vrt.h -- 8^3 bricks
    [bx][by][bz], 4^3 micro-bricks [mx][my][mz], voxels [x][y][z] -- restated with numpy, [cs, cs, cs]."""
    nb = cs // 8
    lin = np.arange(cs ** 3, dtype=np.int64).reshape(nb, 2, 4, nb, 2, 4, nb, 2, 4)        # x = (bx, mx, vx), y, z
    order = lin.transpose(0, 3, 6, 1, 4, 7, 2, 5, 8).reshape(-1)                           # cell stored at each byte
    off = np.empty(cs ** 3, np.int64)
    off[order] = np.arange(cs ** 3)
    return off.reshape(cs, cs, cs)


def world_tables_reference(dims, cs, cells, off):
    """block * cs^3 + vrt_voxel_offset for world cells [n, 3] (cell coordinates from the world's lowest corner)."""
    c, l = cells // cs, cells % cs
    block = (c[:, 0] * dims[1] + c[:, 1]) * dims[2] + c[:, 2]
    return block * cs ** 3 + off[l[:, 0], l[:, 1], l[:, 2]]


def largest_world_table_dims(L, cs, d0=2, d2=3):
    """The largest d1 for which vrt_world_tables_bytes still gives dims (d0, d1, d2) tables: asked of the library."""
    nb, d1 = C.c_int64(0), 1
    while True:
        assert L.vrt_world_tables_bytes((C.c_int32 * 3)(d0, d1 + 1, d2), cs, C.byref(nb)) == 0
        if nb.value == 0:
            return (d0, d1, d2)
        d1 += 1


@pytest.mark.one_march
@pytest.mark.parametrize("cs", [8, 16, 32, 64])
def test_world_tables_match_voxel_offsets(cs):
    """world_tables_kernel (vrt_world_tables_build; what march_step_w reads instead of the chunk table): for dims that are
    single, non-cubic and the largest the library accepts, X[x] + Y[y] + Z[z] is the byte of world cell (x, y, z) --
    its block in table order times the block size plus vrt_voxel_offset of its cell -- for every cell (a fixed random
    200 000 where there are more), and the 32 guard words either side of each axis read 2^30."""
    import torch
    from python_raytracer_amd import _native as nat
    L = nat.lib()
    off = voxel_offset_table(cs)
    rng = np.random.default_rng(400 + cs)
    for lx, ly, lz in np.concatenate([rng.integers(0, cs, (2000, 3)), [[0, 0, 0], [cs - 1] * 3, [7, cs - 8, 3], [4, 3, cs - 1]]]):   # the restatement itself
        assert off[lx, ly, lz] == L.vrt_voxel_offset(cs, int(lx), int(ly), int(lz))
    largest = largest_world_table_dims(L, cs)
    nb = C.c_int64(-1)
    assert largest[1] > 8 and L.vrt_world_tables_bytes((C.c_int32 * 3)(largest[0], largest[1] + 1, largest[2]), cs, C.byref(nb)) == 0
    assert nb.value == 0                                    # one past the largest: no tables
    for dims in ((1, 1, 1), (2, 3, 5), (7, 1, 4), largest):
        d32 = (C.c_int32 * 3)(*dims)
        assert L.vrt_world_tables_bytes(d32, cs, C.byref(nb)) == 0
        n = [d * cs + 64 for d in dims]
        assert nb.value == 4 * sum(n), (dims, nb.value)
        out = torch.full((sum(n) + 2,), -1, dtype=torch.int32, device="cuda")
        nat.check(L.vrt_world_tables_build(d32, cs, out.data_ptr(), nb.value, None), "vrt_world_tables_build")
        raw = out.cpu().numpy().view(np.uint32)
        assert (raw[-2:] == 0xFFFFFFFF).all()               # nothing written past the tables
        X, Y, Z = (raw[:n[0]].astype(np.int64), raw[n[0]:n[0] + n[1]].astype(np.int64), raw[n[0] + n[1]:sum(n)].astype(np.int64))
        for t in (X, Y, Z):
            assert (t[:32] == 1 << 30).all() and (t[-32:] == 1 << 30).all() and (t[32:-32] < 1 << 30).all()
        ext = np.array(dims) * cs
        if int(np.prod(ext)) <= 200000:
            cells = np.stack(np.meshgrid(*[np.arange(e) for e in ext], indexing="ij"), -1).reshape(-1, 3)
        else:
            cells = np.concatenate([rng.integers(0, ext, (200000, 3)), [[0, 0, 0], ext - 1]])
        got = X[cells[:, 0] + 32] + Y[cells[:, 1] + 32] + Z[cells[:, 2] + 32]
        assert np.array_equal(got, world_tables_reference(dims, cs, cells, off)), dims
    # more than 2^30 bytes of voxels: no tables, though these would fit the LDS budget
    side = 1
    while (side ** 3) * cs ** 3 <= 1 << 30:
        side += 1
    assert 3 * (side * cs + 64) * 4 <= 16384
    assert L.vrt_world_tables_bytes((C.c_int32 * 3)(side, side, side), cs, C.byref(nb)) == 0 and nb.value == 0
    assert L.vrt_world_tables_bytes((C.c_int32 * 3)(side - 1, side - 1, side - 1), cs, C.byref(nb)) == 0 and nb.value > 0


def occupancy_reference(buf):
    """bit b of word w = (buf[64 w + b] != 0)."""
    return np.packbits(buf != 0, bitorder="little").view(np.uint64)


@pytest.mark.one_march
@pytest.mark.parametrize("zero_fraction", [0.0, 0.5, 0.97, 1.0])
def test_occupancy_words_match_numpy(zero_fraction):
    """occupancy_kernel (vrt_occupancy_build: the words the VRT_LOOKUP=1|2 variants read; four lanes build one word and
    combine their parts with __shfl_xor) against numpy's packbits, for buffers of one word, three, exactly one 256-lane
    block, one word more, and an odd number of blocks and words; bytes 0x80 and 0x01 among the non-zero ones (a test of
    part of a byte would miss one of them); nothing written past the last word."""
    import torch
    from python_raytracer_amd import _native as nat
    L = nat.lib()
    rng = np.random.default_rng(500 + int(zero_fraction * 100))
    sentinel = np.int64(0x5A5A5A5A5A5A5A5A)
    for n_bytes in (64, 64 * 3, 64 * 64, 64 * 64 + 64, 64 * 1000 + 64 * 37):
        buf = rng.choice(np.array([0x80, 0x01, 0x10, 0xFF, 0x7E], np.uint8), n_bytes)
        buf[rng.random(n_bytes) < zero_fraction] = 0
        if zero_fraction < 1.0:
            buf[[5, n_bytes - 2]] = 0x80, 0x01             # (both are there whatever the draws left)
        assert (buf == 0x80).any() == (buf == 0x01).any() == (zero_fraction < 1.0)
        want = occupancy_reference(buf)
        words = n_bytes // 64
        assert len(want) == words
        vox = torch.from_numpy(buf).cuda()
        out = torch.full((words + 2,), int(sentinel), dtype=torch.int64, device="cuda")
        nat.check(L.vrt_occupancy_build(vox.data_ptr(), n_bytes, out.data_ptr(), None), "vrt_occupancy_build")
        got = out.cpu().numpy()
        assert np.array_equal(got[:words].view(np.uint64), want), n_bytes
        assert (got[words:] == sentinel).all(), n_bytes


def plan_pixel_lists(width, height, threads):
    return ol.pixel_lists(width, height, threads)


# (width, height, samples, threads): words of the seed bitmap = width * height * samples // 32 + 1 (lod_edge 0.25: the most
# samples of a pixel are `samples`); plan_blocksum_kernel / plan_compact_kernel take 1024 words per block (VRT_SCAN_WORDS)
# and plan_scan_sums_kernel scans 256 block sums per pass
PLAN_CASES = {
    "one_word": (5, 3, 2, 1),                  # 30 seeds at most: 1 word, 1 block
    "one_block": (124, 88, 3, 4),              # 32 736: 1 024 words, exactly 1 block
    "one_block_and_a_word": (128, 128, 2, 4),  # 32 768: 1 025 words, 2 blocks
    "two_scan_passes": (2048, 1366, 3, 0),     # 8 392 704: 262 273 words, 257 blocks -- one more than a scan pass (0: a fixed list)
}


@pytest.mark.one_march
@pytest.mark.parametrize("case", list(PLAN_CASES))
def test_tile_plan_at_block_edges(case):
    """vrt_plan_build where its scan changes path: seed bitmaps of one word, of exactly one 1024-word block, of one word
    more, and of more blocks than one pass of plan_scan_sums_kernel takes; then a pixel list with repeated pixels and one
    in reverse order.  n_distinct, the sorted seed list and the seed index of every slot against numpy (check_tile_plan)."""
    width, height, samples, threads = PLAN_CASES[case]
    st = ol.make_settings(width=width, height=height, samples=samples, threads=1)
    words = width * height * samples // 32 + 1
    assert (words, (words + 1023) // 1024) == {"one_word": (1, 1), "one_block": (1024, 1), "one_block_and_a_word": (1025, 2),
                                               "two_scan_passes": (262273, 257)}[case]
    sc = ol.default_scene()
    cam = camera_for(sc, settings_store(st), sc.cam_pos, sc.cam_rot, sc.cam_lens)
    cst = cam._c_settings(0)
    rng = np.random.default_rng(600)
    if threads:
        lists = plan_pixel_lists(width, height, threads)
    else:       # a few thousand pixels of the large window, its corners among them: the first and the last word are used
        px = np.stack([rng.integers(0, width, 3000), rng.integers(0, height, 3000)], 1)
        lists = [np.unique(np.concatenate([px, [[0, 0], [width - 1, height - 1], [width - 1, 0], [0, height - 1]]]), axis=0).astype(np.int32)]
    for px in lists:
        hdr = check_tile_plan(cam._plan_for(cam.upload_pixels(px), cst), st)
        assert int(hdr[5]) == words and int(hdr[6]) == (1 if threads == 1 else 0)
    base = lists[-1]
    repeated = np.concatenate([base[:40], base[:40], base[5:25], base])
    hdr = check_tile_plan(cam._plan_for(cam.upload_pixels(repeated), cst), st)
    assert int(hdr[6]) == 0
    hdr = check_tile_plan(cam._plan_for(cam.upload_pixels(np.ascontiguousarray(base[::-1])), cst), st)
    assert int(hdr[6]) == (1 if len(base) == 1 and width * height == 1 else 0)


@pytest.mark.one_march
def test_voxelize_far_world():
    """voxelize_kernel (DeviceWorld.build) 2^24 cells from the origin: three small random objects -- two that overlap,
    one with quarter turns about every axis, one whose box crosses the last chunk border of the world on every axis, so
    that it alone decides where the world box ends -- in a world whose origin is (2^20, -2^20, 0) chunks of 16.  Voxel
    blocks, chunk presence, origin, dims and materials equal build_world() on the host, which takes this origin as it is.
    (DeviceWorld.build sizes the world box from the objects' boxes, so no object can reach beyond it: the kernel's
    clipping against each object's box, not against the world's, is what the overhanging object exercises.)"""
    from python_raytracer_amd import Material
    from python_raytracer_amd.lib import vec3, rgb, material
    from python_raytracer_amd.scene import unpack_blocks
    from python_raytracer_amd.world import DeviceWorld, Object, Sprite, build_world
    rng = np.random.default_rng(700)
    cs = 16
    far = np.array([1 << 24, -(1 << 24), 0])
    mats = [Material(function=material, albedo=rgb(30 * i, 20, 40), roughness=0.1, absorption=1, ior=0, energy=0) for i in range(1, 6)]
    objs = []
    #                     size          offset from the far corner   rotation
    for size, at, rot in (((10, 6, 8), (6, 5, 5.5), (0, 0, 0)),
                          ((8, 8, 8), (9.5, 7, 8), (90, 270, 180)),          # overlaps the first; cubic: every turn applies
                          ((6, 12, 6), (29, 14, 30.5), (0, 90, 0))):         # x 26..32, y 8..20, z 28..34: over the borders at 16 and 32
        spr = Sprite(size=vec3(*size), frames=1, lod=0)
        vox = {}
        for _ in range(120):
            vox[tuple(int(rng.integers(0, s)) for s in size)] = mats[int(rng.integers(len(mats)))]
        spr.get_frame(0).set_voxels(vox, True)
        ob = Object(pos=vec3(*[float(f + a) for f, a in zip(far, at)]), rot=vec3(*rot), sprite=spr)
        ob.visible = True
        objs.append(ob)
    w = build_world(objs, cs)
    assert np.array_equal(w.origin, far) and list(w.dims) == [3, 2, 3] and w.present.sum() > 4 and w.grid.any()
    a, b = objs[0], objs[1]
    assert all(max(lo1, lo2) < min(hi1, hi2) for lo1, hi1, lo2, hi2 in zip(a.mins.tuple(), a.maxs.tuple(), b.mins.tuple(), b.maxs.tuple()))
    dw = DeviceWorld(cs)
    ps = dw.build(objs)
    assert np.array_equal(dw.origin, w.origin) and np.array_equal(dw.dims, w.dims)
    assert [id(m) for m in dw.materials] == [id(m) for m in w.materials]
    dims = [int(v) for v in dw.dims]
    table = ps.device_tensors["chunk_table"].cpu().numpy().view(np.uint32).reshape(dims)
    blocks = unpack_blocks(ps.device_tensors["voxels"].cpu().numpy().reshape(-1, cs ** 3), cs)
    grid = blocks.reshape(dims[0], dims[1], dims[2], cs, cs, cs).transpose(0, 3, 1, 4, 2, 5).reshape(dims[0] * cs, dims[1] * cs, dims[2] * cs)
    assert np.array_equal(grid, w.grid)
    assert np.array_equal((table != 0).astype(np.uint8), w.present)
    n = np.arange(table.size, dtype=np.uint32).reshape(table.shape) + 1
    assert np.array_equal(table[table != 0], (n | (1 << 24))[table != 0])
