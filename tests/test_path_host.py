"""Hit paths of explicit rays without a GPU: tests/path_ref.py's restatement against the oracle-derived records of
shade_ref's six ray sets, the preconditions of the cases tests/test_gpu_paths.py runs (asserted on the reference), the C
ABI's new symbols, what vrt_path_rays and vrt_pixel_rays refuse before any HIP call, and the compiler's resource report of
path_kernel (tests/kernel_report.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import kernel_report
import path_ref as pr
import shade_ref as sr
from python_raytracer_amd import _native as nat

HEADER = os.path.join(kernel_report.ROOT, "include", "vrt.h")
ALL_SETS = ["default_mb2", "default_mb8", "default_scaled_nobg", "synth64_mb4", "hand", "big_table"]


# ---- 1. the restatement against the oracle, and the sets ---------------------------------------------------------------
@pytest.mark.parametrize("name", ALL_SETS)
def test_trace_path_equals_the_oracle(name):
    """trace_path's end record is the oracle-derived record bit for bit, and every path is as long as the oracle's hit
    counter; a path's records are the ray's own states: steps never decrease, the cell is floor(pos), the material is one
    of the scene's."""
    sc, st, has_bg, origins, vels, lives, draws, exp, trav = sr.ray_set(name)
    rec, counts, paths = pr.path_set(name)
    sr.assert_records_equal(rec, exp)
    assert np.array_equal(counts, exp["counters"][:, sr.C_HIT])
    assert [len(p) for p in paths] == counts.tolist()
    for path in paths:
        steps = [h[0] for h in path]
        assert steps == sorted(steps)
        for step, pos, cell, mat in path:
            assert cell == tuple(int(np.floor(p)) for p in pos) and 1 <= mat <= len(sc.materials)


@pytest.mark.parametrize("name", ALL_SETS)
def test_sets_cover_the_cases(name):
    """What the GPU cases rely on.  Rays over 4 hits, and the largest count, per set:
        default_mb2 1 / 7, default_mb8 .. default_scaled_nobg in between, big_table 51 / 19."""
    rec, counts, paths = pr.path_set(name)
    over = int((counts > 4).sum())
    print(name, "over 4:", over, "largest:", int(counts.max()), "draws:", int(rec["counters"][:, sr.C_DRAW].max()))
    assert (counts == 0).any() and ((counts >= 1) & (counts <= 3)).any() and (counts == 4).any() and over >= 1
    assert 1 <= over <= 51 and counts.max() <= 19 < 32          # max_hits 4 truncates, 32 never does
    if name == "default_mb2":
        assert over == 1
    if name == "big_table":
        assert over == 51 and counts.max() == 19
    most = int(rec["counters"][:, sr.C_DRAW].max())
    assert 12 <= most <= 18 and (rec["counters"][:, sr.C_DRAW] > 6).any()      # a 6-draw row exhausts some rays


def test_trace_path_reports_exhaustion():
    """With six draws per row the restatement marks exactly the rays whose oracle draw count exceeds 6, and they report no
    path."""
    sc, st, has_bg, origins, vels, lives, draws, exp, trav = sr.ray_set("default_mb8")
    rec, counts, paths = pr.trace_paths(sc, st, origins[:150], vels[:150], lives[:150], draws[:150, :6], has_bg)
    out = exp["counters"][:150, sr.C_DRAW] > 6
    assert 0 < out.sum() < 150 and np.array_equal(counts == -3, out) and all(not paths[k] for k in np.nonzero(out)[0])
    sr.assert_records_equal(rec[~out], exp[:150][~out])
    rows = pr.rows(paths, counts, 4)
    assert (rows[out]["material"] == -1).all() and (rows[out]["step"] == 0).all()


# ---- 2. the C ABI ------------------------------------------------------------------------------------------------------
def test_header_declares_the_entry_points():
    text = open(HEADER).read()
    assert re.search(r"int vrt_path_workspace_bytes\(int64_t n_rays, int64_t\* bytes\);", text)
    assert re.search(r"int vrt_path_rays\(const vrt_scene\* scene, const vrt_settings\* st, const vrt_cast_ray\* d_rays, "
                     r"int64_t n_rays,\s+double max_life, const double\* d_draws, int32_t n_draws, int32_t max_hits, "
                     r"void\* d_workspace,\s+int64_t workspace_bytes, vrt_hit\* d_hits, int32_t\* d_counts, uint32_t\* d_rgba, "
                     r"uint64_t\* d_stats,\s+void\* stream\);", text)
    assert re.search(r"int vrt_pixel_rays\(const vrt_scene\* scene, const vrt_settings\* st, const vrt_camera\* cam, "
                     r"const int32_t\* d_pixels_xy,\s+int64_t n_px, const void\* d_plan, int64_t n_distinct, "
                     r"const double\* d_ray_table,\s+int32_t first_sample_only, vrt_cast_ray\* d_rays, uint64_t\* d_stats, "
                     r"void\* stream\);", text)
    assert "#define VRT_ABI_VERSION 9" in text


def test_library_exports_the_entry_points():
    L = nat.lib()
    assert L.vrt_abi_version() == 9 and nat.ABI_VERSION == 9      # the change only adds symbols
    for name in ("vrt_path_workspace_bytes", "vrt_path_rays", "vrt_pixel_rays"):
        assert name in nat.EXPORTS and getattr(L, name) is not None
    assert nat.PATH_REJECTED == -2 and nat.PATH_EXHAUSTED == -3 and nat.HIT_UNUSED == -1
    assert nat.S_PATH_TRUNCATED == 12 and nat.S_PATH_RECORDS == 13 and nat.PATH_MAX_HITS == 64
    nb, ns = C.c_int64(-1), C.c_int64(-2)
    assert L.vrt_path_workspace_bytes(0, C.byref(nb)) == 0 and nb.value > 0
    assert L.vrt_shade_workspace_bytes(0, C.byref(ns)) == 0 and ns.value == nb.value
    big = C.c_int64(-1)
    assert L.vrt_path_workspace_bytes(1 << 31, C.byref(big)) == 0 and big.value == nb.value      # nothing per ray
    assert L.vrt_path_workspace_bytes(-1, C.byref(nb)) == -1 and L.vrt_path_workspace_bytes(5, None) == -1


def _scene_and_settings():
    st = nat.VrtSettings(15, 11, 3, 8, 4, 1, 0, 0.875, .25, .25, .5, 0, 48, 1, 4, .5, .5, .25, .5)
    sc = nat.VrtScene()
    sc.origin[:] = [-24, -24, -24]
    sc.dims[:] = [6, 6, 6]
    sc.chunk_size, sc.n_slots, sc.n_materials, sc.max_resolution = 8, 10, 4, 1
    sc.d_chunk_table = sc.d_voxels = sc.d_materials = 0x1000
    return sc, st


def test_path_rays_rejects_bad_arguments_without_a_device():
    """Everything the entry point can refuse is refused before its first HIP call: these calls carry made-up device
    pointers, which nothing reads."""
    L = nat.lib()
    sc, st = _scene_and_settings()
    fake = 0x1000
    nb = C.c_int64(0)
    assert L.vrt_path_workspace_bytes(100, C.byref(nb)) == 0

    def call(scene=sc, settings=st, rays=fake, n=100, max_life=48.0, draws=fake, n_draws=8, max_hits=8, ws=fake, ws_bytes=nb.value,
             hits=fake, counts=fake, rgba=fake, stats=fake):
        return L.vrt_path_rays(C.byref(scene) if scene is not None else None, C.byref(settings) if settings is not None else None,
                               rays, n, max_life, draws, n_draws, max_hits, ws, ws_bytes, hits, counts, rgba, stats, None)

    assert call(max_hits=0) == -1 and call(max_hits=65) == -1 and call(max_hits=-1) == -1
    assert call(n=1 << 27, max_hits=16) == -1 and call(n=1 << 25, max_hits=64) == -1        # n_rays * max_hits = 2^31
    assert call(n=(1 << 31) // 3 + 1, max_hits=3) == -1                                      # ... and just above it
    assert call(hits=None) == -1 and call(counts=None) == -1
    assert call(hits=fake + 4) == -1 and call(counts=fake + 2) == -1
    assert call(rays=None) == -1 and call(rays=fake + 8) == -1        # the array is 64-byte aligned
    assert call(ws_bytes=nb.value - 1) == nat.ERR_WORKSPACE == -3 and call(ws_bytes=0) == -3 and call(ws=None) == -1
    assert call(scene=None) == -1 and call(settings=None) == -1 and call(stats=None) == -1
    assert call(n=-1) == -1 and call(n=(1 << 32) - 1, max_hits=1) == -1
    assert call(max_life=0.0) == -1 and call(max_life=float("nan")) == -1 and call(max_life=float((1 << 28) + 1)) == -1
    assert call(n_draws=-1) == -1 and call(draws=None, n_draws=3) == -1
    odd = nat.VrtSettings(15, 11, 3, 12, 6, 1, 0, 0.875, .25, .25, .5, 0, 48, 1, 4, .5, .5, .25, .5)
    assert call(settings=odd) == -1                                   # check_settings: the chunk size is a power of two


def test_pixel_rays_rejects_bad_arguments_without_a_device():
    """vrt_first_hit's checks, and the alignment the explicit-ray calls ask of the records."""
    L = nat.lib()
    sc, st = _scene_and_settings()
    fake = 0x1000
    cam = nat.VrtCamera()
    cam.rot[:] = [0, 0, 0, 1]
    cam.lens = 1.0

    def call(scene=sc, settings=st, camera=cam, px=fake, n_px=10, plan=fake, n_distinct=5, rtab=fake, first=1, rays=fake, stats=fake):
        return L.vrt_pixel_rays(C.byref(scene) if scene is not None else None, C.byref(settings) if settings is not None else None,
                                C.byref(camera) if camera is not None else None, px, n_px, plan, n_distinct, rtab, first, rays,
                                stats, None)

    assert call(scene=None) == -1 and call(settings=None) == -1 and call(camera=None) == -1 and call(stats=None) == -1
    assert call(px=None) == -1 and call(n_px=-1) == -1 and call(plan=None) == -1 and call(rtab=None) == -1
    assert call(rays=None) == -1 and call(rays=fake + 8) == -1 and call(rays=fake + 32) == -1
    assert call(n_distinct=-1) == -1 and call(n_distinct=10 ** 6) == -1
    nonce = nat.VrtSettings(15, 11, 3, 8, 4, 1, 5, 0.875, .25, .25, .5, 0, 48, 1, 4, .5, .5, .25, .5)
    assert call(settings=nonce) == -1                                 # the ray table is a static-seed run's
    far = nat.VrtCamera()
    far.rot[:] = [0, 0, 0, 1]
    far.pos[:] = [float(1 << 28), 0, 0]
    assert call(camera=far) == -1                                     # the frame's range rule


# ---- 3. the compiler's resource report ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def report():
    return kernel_report.report()


def path_name(spec, res):
    return "_Z11path_kernelILi%dELi%dEEv11MarchParams" % (spec, res)


@pytest.mark.parametrize("spec,res", [(8, 0), (8, 1), (4, 2)])
def test_path_kernel_resources(report, spec, res):
    """The three instances launch_path chooses from.  All of them, the generic one included: no vector spills, at most 16
    bytes of scratch (the pow slow path's frame: the frame kernels' bound), no AGPRs, 4 waves per SIMD."""
    assert len([k for k in report if k.startswith("_Z11path_kernel")]) == 3
    r = report[path_name(spec, res)]
    assert r["Occupancy [waves/SIMD]"] >= 4 and r["AGPRs"] == 0 and r["VGPRs"] <= 128, r
    assert r["VGPRs Spill"] == 0 and r["ScratchSize [bytes/lane]"] <= 16, r
    if res == 2:
        assert report["_Z12shade_kernelILi4ELi2ELb0EEv11MarchParams"]["VGPRs"] == 128      # the sibling has none to spare either
    # (every figure of path_kernel and pixel_rays_kernel is pinned with all the others: tests/test_kernel_resources.py)
