"""CPU-only checks of the host side: the C-ABI library loads and exports every declared symbol, host helpers,
the settings / pixel partition mirror, Frame semantics and scene flattening."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import oracle_lib as ol
from python_raytracer_amd import _native as nat
from python_raytracer_amd import Frame, Material, PackedScene, make_settings, load_settings
from python_raytracer_amd.lib import vec3, rgb, material

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_loads_and_exports_every_declared_symbol():
    L = nat.lib()
    hdr = open(os.path.join(ROOT, "include", "vrt.h")).read()
    declared = set(re.findall(r"\b(vrt_[a-z_0-9]+)\s*\(", hdr))
    assert declared == set(nat.EXPORTS), declared ^ set(nat.EXPORTS)
    for name in declared:
        assert getattr(L, name) is not None
    assert L.vrt_abi_version() == nat.ABI_VERSION
    assert L.vrt_status_string(0) == b"ok"


def test_last_plan_diagnostic_is_exported_and_checks_its_arguments():
    """vrt_diag_last_plan (outside include/vrt.h: no ABI change) reads host memory only: callable without a GPU.  A null
    pointer is VRT_ERR_ARG; before any launch every word reads 0; the return value is the number of words there are."""
    L = nat.lib()
    assert L.vrt_diag_last_plan is not None and "vrt_diag_last_plan" not in nat.EXPORTS
    assert L.vrt_diag_last_plan(None, 8) == -1                                # VRT_ERR_ARG
    buf = (C.c_int64 * 64)(*([-7] * 64))
    n = L.vrt_diag_last_plan(buf, 64)
    assert 10 <= n <= 64 and (n - 10) % 5 == 0
    assert list(buf[:n]) == [0] * n and list(buf[n:]) == [-7] * (64 - n)      # nothing written past the words
    assert L.vrt_diag_last_plan(buf, -1) == -1
    plan = nat.last_plan()
    assert plan["launches"] == 0 and plan["probes"] == [] and set(nat.PLAN_FIELDS) < set(plan)


def test_struct_layouts_match_header():
    assert C.sizeof(nat.VrtSettings) == 128
    assert C.sizeof(nat.VrtCamera) == 64
    assert C.sizeof(nat.VrtScene) == 96
    assert C.sizeof(nat.VrtTraversed) == 48
    assert np.dtype(nat.RAY_FIELDS, align=True).itemsize == nat.RAY_BYTES


def test_argument_validation_without_gpu():
    L = nat.lib()
    nb = C.c_int64(0)
    st = nat.VrtSettings(64, 48, 1, 16, 8, 1, 0, 0.875, .25, .25, .5, 0, 192, 1, 2, .5, .5, .25, .25)
    assert L.vrt_workspace_bytes(C.byref(st), 3072, 1000, 32, 0, C.byref(nb)) == 0 and nb.value > 0
    nb_ext = C.c_int64(0)   # tables passed by the caller need no room in the workspace
    assert L.vrt_workspace_bytes(C.byref(st), 3072, 1000, 32, 3, C.byref(nb_ext)) == 0
    assert nb.value - nb_ext.value >= 1000 * 32 * 8 + 3072 * 64
    assert L.vrt_workspace_bytes(C.byref(st), 3072, 1000, 32, 4, C.byref(nb)) == -1   # unknown flag
    bad = nat.VrtSettings(64, 48, 1, 12, 6, 1, 0, 0.875, .25, .25, .5, 0, 192, 1, 2, .5, .5, .25, .25)
    assert L.vrt_workspace_bytes(C.byref(bad), 3072, 1000, 32, 0, C.byref(nb)) == -1   # chunk_size not a power of two
    assert L.vrt_workspace_bytes(C.byref(st), 3072, 1000, 48, 0, C.byref(nb)) == -1    # fast_draws must be 32 or 64
    pb, sb = C.c_int64(0), C.c_int64(0)
    assert L.vrt_plan_bytes(C.byref(st), 3072, C.byref(pb), C.byref(sb)) == 0 and pb.value > 64 and sb.value > 0
    huge = nat.VrtSettings(70000, 70000, 1, 16, 8, 1, 0, 1.0, .25, .25, .5, 0, 192, 1, 2, .5, .5, .25, .25)
    assert L.vrt_plan_bytes(C.byref(huge), 10, C.byref(pb), C.byref(sb)) == -1   # seeds must fit 32 bits
    assert L.vrt_max_samples(C.byref(st)) == 1
    st.samples = 8
    assert L.vrt_max_samples(C.byref(st)) == 8
    assert L.vrt_render_tile(None, C.byref(st), None, None, 0, None, 0, 32, None, None, None, 0, None, None, None, None,
                             None, None, None) == -1
    tb = C.c_int64(0)
    assert L.vrt_draw_table_bytes(1000, 32, C.byref(tb)) == 0 and tb.value >= 1000 * 32 * 8
    assert L.vrt_draw_table_bytes(1000, 48, C.byref(tb)) == -1   # 32 or 64 draws per seed
    assert L.vrt_draw_table_build(C.byref(st), None, 10, None, 5, 32, None, 0, None) == -1
    rb = C.c_int64(0)
    assert L.vrt_ray_table_bytes(C.byref(st), 3072, C.byref(rb)) == 0 and rb.value >= 3072 * 8 * 64
    assert L.vrt_ray_table_build(C.byref(st), 35.0, None, 10, None, None, 32, None, 0, None) == -1
    assert L.vrt_occupancy_build(None, 100, None, None) == -1          # not a multiple of 64
    assert L.vrt_occupancy_build(None, 0, None, None) == 0


def test_ray_table_is_per_pixel_when_nothing_depends_on_the_sample():
    """vrt_ray_table_bytes: one 64-byte record per ray slot, but per PIXEL when dof, lod_random and lod_samples are all 0
    (lens quaternion and life are then functions of the pixel alone, include/vrt.h): BASELINE config 5's table is
    1.07 GB instead of 17.2 GB."""
    L = nat.lib()
    tb = C.c_int64(0)
    #                       w     h     spp cs r bg nonce prop shut  fall dof dmin dmax ml mb  lodb lods lodr lode
    c5 = nat.VrtSettings(4096, 4096, 16, 16, 8, 1, 0, 1.0, .25, .25, 0.0, 0, 1024, 1, 8, 0.0, 0.0, 0.0, 0.0)
    assert L.vrt_ray_table_bytes(C.byref(c5), 4096 * 4096, C.byref(tb)) == 0 and tb.value == 4096 * 4096 * 64
    for field, value in (("dof", 0.5), ("lod_random", 0.25), ("lod_samples", 0.5)):
        st = nat.VrtSettings(4096, 4096, 16, 16, 8, 1, 0, 1.0, .25, .25, 0.0, 0, 1024, 1, 8, 0.0, 0.0, 0.0, 0.0)
        setattr(st, field, value)
        assert L.vrt_ray_table_bytes(C.byref(st), 4096 * 4096, C.byref(tb)) == 0 and tb.value == 4096 * 4096 * 16 * 64
    edge = nat.VrtSettings(4096, 4096, 16, 16, 8, 1, 0, 1.0, .25, .25, 0.0, 0, 1024, 1, 8, 0.0, 0.0, 0.0, 0.25)
    assert L.vrt_ray_table_bytes(C.byref(edge), 100, C.byref(tb)) == 0
    assert tb.value == ((100 * 64 + 255) // 256) * 256   # (lod_edge only changes the sample count kept in the record)
    # the workspace needs no more either when it holds the table itself
    with_tab, without = C.c_int64(0), C.c_int64(0)
    assert L.vrt_workspace_bytes(C.byref(c5), 1 << 20, 1000, 32, 1, C.byref(with_tab)) == 0
    assert L.vrt_workspace_bytes(C.byref(c5), 1 << 20, 1000, 32, 3, C.byref(without)) == 0
    assert with_tab.value - without.value == (1 << 20) * 64


def test_camera_and_reach_are_range_checked_without_gpu():
    """The march keeps floor(pos) in 32-bit integers, so vrt_render_tile / vrt_trace_rays reject (VRT_ERR_ARG, before
    any HIP call) a camera position, dist_max / dist_min or a rotation whose reach could leave +-2^30, and NaNs."""
    L = nat.lib()
    fake = 0x1000   # never dereferenced: validation fails first
    sc = nat.VrtScene()
    sc.origin[:] = [0, 0, 0]
    sc.dims[:] = [1, 1, 1]
    sc.chunk_size, sc.n_slots, sc.n_materials = 16, 1, 1
    sc.d_chunk_table = sc.d_voxels = sc.d_materials = sc.d_occupancy = fake
    sc.max_resolution = 1

    def call(pos=(0.0, 0.0, 0.0), rot=(0.0, 0.0, 0.0, 1.0), dist_max=192.0, dist_min=0.0, lens=35.0):
        st = nat.VrtSettings(64, 48, 1, 16, 8, 1, 0, 0.875, .25, .25, .5, dist_min, dist_max, 1, 2, .5, .5, .25, .25)
        cam = nat.VrtCamera()
        cam.pos[:] = pos
        cam.rot[:] = rot
        cam.lens = lens
        # n_px = 0 and a NULL pixel list: a call that passes validation returns before touching the device only if
        # ... it does not: so only failing calls are made here, plus the workspace-too-small path (-3) as the control
        return L.vrt_render_tile(C.byref(sc), C.byref(st), C.byref(cam), fake, 1, fake, 1, 32, None, None, fake, 0,
                                 None, None, None, None, fake, None, None)

    assert call() == -3                                        # control: arguments fine, workspace of 0 bytes too small
    assert call(pos=(3e9, 0.0, 0.0)) == -1                     # beyond the 32-bit cursor
    assert call(pos=(0.0, float("nan"), 0.0)) == -1
    assert call(pos=(2.0 ** 28, 0.0, 0.0), dist_max=2.0 ** 27) == -1   # camera + reach
    assert call(dist_max=2.0 ** 29) == -1
    assert call(dist_max=float("inf")) == -1
    assert call(dist_min=-2.0 ** 29) == -1
    assert call(rot=(0.0, 0.0, 0.0, 2000.0)) == -1            # the reference's quaternion product scales the velocity
    assert call(rot=(0.0, 0.0, 0.0, 40.0), dist_max=2.0 ** 20) == -1
    assert call(lens=float("nan")) == -1


def test_voxel_offset_is_a_bijection_and_matches_numpy_packing():
    L = nat.lib()
    for cs in (8, 16, 32):
        blk = np.arange(cs ** 3, dtype=np.uint32).reshape(1, cs, cs, cs)
        lin = np.zeros(cs ** 3, np.int64)
        seen = set()
        for x in range(cs):
            for y in range(cs):
                for z in range(cs):
                    o = L.vrt_voxel_offset(cs, x, y, z)
                    seen.add(o)
                    lin[o] = blk[0, x, y, z]
        assert seen == set(range(cs ** 3))
        from python_raytracer_amd.scene import pack_blocks
        packed = pack_blocks((blk % 251).astype(np.uint8))
        assert (packed[0] == (lin % 251)).all()


def test_pixel_partition_matches_reference_order():
    s = make_settings(width=7, height=5, threads=3)
    ref = [[] for _ in range(3)]
    for x in range(7):
        for y in range(5):
            ref[(x ^ y) % 3].append((x, y))
    assert [list(p) for p in s.pixels] == ref
    assert s.proportions == ((7 + 5) / 2) / 7 and s.chunk_radius == 8 and s.window == (7, 5)
    g = ol.load_render("c1_t8")
    s = make_settings(width=96, height=54, threads=8)
    for t in range(8):
        a = s.pixels[t].array
        assert (g["owner"][a[:, 1], a[:, 0]] == t).all()


def test_load_settings_or_default_idiom(tmp_path):
    p = tmp_path / "config.cfg"
    p.write_text("[WINDOW]\nwidth = 64\nheight = 48\n[RENDER]\nsync = false\nculling = true\nstatic = true\n"
                 "samples = 0\nshutter = 0.25\nfalloff = 0.25\nchunk_size = 16\nchunk_lod = 2\nfov = 0\ndof = 0.5\n"
                 "dist_min = 0\ndist_max = 192\nmax_light = 1\nmax_bounces = 2\nlod_bounces = 0.5\nlod_samples = 0.5\n"
                 "lod_random = 0.25\nlod_edge = 0.25\nthreads = 2\n")
    s = load_settings(str(p))
    assert s.samples == 1 and s.fov == 90 and s.threads == 2 and s.dist_max == 192 and s.static is True
    assert s.proportions == 0.875 and len(s.pixels) == 2


def _mat(**kw):
    d = dict(function=material, albedo=rgb(10, 20, 30), roughness=0.5, absorption=1, ior=1, energy=0)
    d.update(kw)
    return Material(**d)


def test_frame_semantics():
    m1, m2 = _mat(), _mat(albedo=rgb(1, 2, 3))
    f = Frame(packed=True, resolution=2)
    f.set_voxels({(0, 0, 0): m1, (1, 0, 0): m2, (2, 4, -6): m2, (3, 3, 3): m1}, True)
    assert f.data3 == {(0, 0, 0): m1, (1, 2, -3): m2}          # only positions divisible by 2, keyed by p // 2
    assert f.get_voxel(vec3(1, 1, 1)) is m1 and f.get_voxel(vec3(2, 5, -5)) is m2 and f.get_voxel(vec3(4, 0, 0)) is None
    f.data6[(5, 5, 5, 6, 6, 6)] = m1                              # a box as the reference's pack() would produce
    assert f.get_voxel(vec3(12, 13, 11)) is m1
    assert len(list(f.cells())) == 2 + 8
    f.set_voxels({(10, 10, 10): None}, True)                     # unboxes, then clears one cell
    assert f.get_voxel(vec3(10, 10, 10)) is None and f.get_voxel(vec3(12, 12, 12)) is m1 and not f.data6
    assert len(f.get_voxels()) == (2 + 7) * 8


def test_flatten_chunks_equals_dense_packing():
    rng = np.random.default_rng(0)
    mats = [_mat(albedo=rgb(i, i, i), roughness=i / 10) for i in range(1, 6)]
    chunks, cs = {}, 16
    dense = np.zeros((32, 16, 48), np.uint8)
    present = np.zeros((2, 1, 3), np.uint8)
    res = np.zeros((2, 1, 3), np.uint8)
    for (cx, cz, r) in [(0, 0, 1), (1, 2, 2), (1, 0, 3)]:
        fr = Frame(resolution=r)
        post = (cx * 16 - 16, 32, cz * 16)
        vox = {}
        for _ in range(200):
            l = rng.integers(0, 16, 3)
            p = tuple(int(v) for v in (np.array(post) + l))
            vox[p] = mats[int(rng.integers(0, 5))]
        fr.set_voxels(vox, True)
        chunks[post] = fr
        present[cx, 0, cz], res[cx, 0, cz] = 1, r
        for q, m in fr.cells():
            p = np.array(q) * r - np.array([-16, 32, 0])
            dense[tuple(p)] = 1 + mats.index(m)
    sc, used = PackedScene.from_chunks(chunks, cs)
    order = [mats.index(m) for m in used]
    table = np.array([[m.albedo.r, m.albedo.g, m.albedo.b, m.roughness, m.absorption, m.ior, m.energy] for m in used])
    remap = np.zeros(6, np.uint8)
    for new, old in enumerate(order):
        remap[old + 1] = new + 1
    sd = PackedScene.from_dense([-16, 32, 0], [2, 1, 3], cs, present, res, remap[dense], table)
    assert (sc.origin == sd.origin).all() and (sc.dims == sd.dims).all()
    # same content per chunk, slot numbering may differ
    for c in range(6):
        a, b = int(sc.chunk_table[c]), int(sd.chunk_table[c])
        assert (a == 0) == (b == 0)
        if a:
            assert a >> 24 == b >> 24
            assert (sc.voxels[(a & 0xffffff) - 1] == sd.voxels[(b & 0xffffff) - 1]).all()
    assert (sc.materials == sd.materials).all()


def test_flatten_rejects_what_the_kernel_cannot_run():
    fr = Frame(resolution=1)
    fr.data3[(0, 0, 0)] = _mat(function=lambda ray, mat, settings: 1)
    with pytest.raises(TypeError):
        PackedScene.from_chunks({(0, 0, 0): fr}, 16)
    fr = Frame(resolution=1)
    fr.data3[(16, 0, 0)] = _mat()
    with pytest.raises(ValueError):
        PackedScene.from_chunks({(0, 0, 0): fr}, 16)
    m = _mat()
    del m.ior
    fr = Frame(resolution=1)
    fr.data3[(1, 0, 0)] = m
    with pytest.raises(TypeError):
        PackedScene.from_chunks({(0, 0, 0): fr}, 16)
    with pytest.raises(ValueError):
        PackedScene.from_chunks({(0, 0, 0): Frame()}, 12)
    with pytest.raises(RuntimeError):
        material(None, None, None)


def test_camera_without_gpu_fails_loudly():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from python_raytracer_amd import Camera
    cam = Camera(settings=make_settings())
    assert abs(cam.lens - 35.34291735288517) < 1e-15
    with pytest.raises(RuntimeError):
        cam.tile(0, 0)


def test_load_settings_reads_the_reference_default_config():
    """Row S: parsing the reference's own mods/default/config.cfg (a copy in tests/golden/mod_default) gives the render
    settings the golden fixtures were generated with (reference data.py:15-68)."""
    s = load_settings(os.path.join(ol.GOLDEN, "mod_default", "config.cfg"), threads=1)
    g = ol.load_render("g64")["settings"]
    for k in ("width", "height", "samples", "static", "shutter", "falloff", "chunk_size", "chunk_lod", "fov", "dof",
              "dist_min", "dist_max", "max_light", "max_bounces", "lod_bounces", "lod_samples", "lod_random", "lod_edge",
              "proportions", "chunk_radius"):
        assert getattr(s, k) == g[k], k
    assert s.culling is True and s.sync is False


def test_seed_class_partition_is_disjoint_in_seeds_and_balanced():
    """multigpu.owner_map(partition="seed"): every pixel has one owner, no static seed (1+x)(1+y)(1+s) is needed by
    two ranks, and the pixel counts are balanced."""
    from python_raytracer_amd.multigpu import owner_map, rank_pixels, rank_pixel_counts
    for w, h, g, smp in ((96, 64, 4, 8), (129, 77, 3, 5), (64, 64, 8, 1)):
        own = owner_map(w, h, g, "seed", smp)
        assert own.shape == (w, h) and own.min() == 0 and own.max() == g - 1
        cnt = rank_pixel_counts(w, h, g, "seed", smp)
        assert cnt.sum() == w * h and cnt.max() - cnt.min() <= max(2, 0.05 * cnt.mean())
        seen = {}
        for r in range(g):
            p = rank_pixels(w, h, g, r, "seed", smp).astype(np.int64)
            assert (own[p[:, 0], p[:, 1]] == r).all() and len(p) == cnt[r]
            assert (np.lexsort((p[:, 1], p[:, 0])) == np.arange(len(p))).all()  # x-major like the reference
            seeds = np.unique(((1 + p[:, 0]) * (1 + p[:, 1]))[:, None] * np.arange(1, smp + 1)[None, :])
            for q in seen.values():
                assert len(np.intersect1d(seeds, q)) == 0
            seen[r] = seeds
    # the reference's own partition is untouched
    x, y = np.meshgrid(np.arange(31), np.arange(17), indexing="ij")
    assert np.array_equal(owner_map(31, 17, 5, "xor"), (x ^ y) % 5)


def test_table_identity_detection_on_host_arrays():
    """PackedScene.table_identity (VRT_SCENE_TABLE_IS_IDENTITY): only a dense resolution-1 world in table order."""
    import numpy as np
    from python_raytracer_amd import PackedScene
    cs, dims = 8, (3, 2, 4)
    n = int(np.prod(dims))
    grid = np.ones(tuple(d * cs for d in dims), np.uint8)
    mats = np.ones((1, 7))
    dense = PackedScene.from_dense([0, 0, 0], dims, cs, np.ones(dims, np.uint8), np.ones(dims, np.uint8), grid, mats)
    assert dense.table_identity() and dense.n_slots == n
    res2 = np.ones(dims, np.uint8)
    res2[1, 1, 1] = 2
    assert not PackedScene.from_dense([0, 0, 0], dims, cs, np.ones(dims, np.uint8), res2, grid, mats).table_identity()
    hole = np.ones(dims, np.uint8)
    hole[0, 0, 0] = 0
    assert not PackedScene.from_dense([0, 0, 0], dims, cs, hole, np.ones(dims, np.uint8), grid, mats).table_identity()
    os.environ["VRT_TABLE_IDENTITY"] = "0"
    try:
        assert not dense.table_identity()
    finally:
        del os.environ["VRT_TABLE_IDENTITY"]
