"""Shaded explicit rays without a GPU: that the ray sets of tests/test_gpu_shade.py are not vacuous, the Python restatement
of Camera.trace's loop in tests/shade_ref.py against the CPU oracle, the C ABI's new symbols, what vrt_shade_rays refuses
before any HIP call, and the compiler's resource report of shade_kernel (tests/kernel_report.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import kernel_report
import shade_ref as sr
from python_raytracer_amd import _native as nat

HEADER = os.path.join(kernel_report.ROOT, "include", "vrt.h")
ALL_SETS = ["default_mb2", "default_mb8", "default_scaled_nobg", "synth64_mb4", "hand", "big_table"]


# ---- 1. the sets are not vacuous ---------------------------------------------------------------------------------------
def figures(name):
    sc, st, has_bg, origins, vels, lives, draws, exp, trav = sr.ray_set(name)
    c = exp["counters"]
    return dict(hit1=float((c[:, sr.C_HIT] >= 1).mean()), hit2=float((c[:, sr.C_HIT] >= 2).mean()),
                hit3=float((c[:, sr.C_HIT] >= 3).mean()), broke=float((c[:, sr.C_BROKE] == 1).mean()),
                nbr=float((c[:, sr.C_NBR] >= 1).mean()), max_hits=int(c[:, sr.C_HIT].max()), max_draws=int(c[:, sr.C_DRAW].max()),
                colours=len(set(sr.packed(exp).tolist())), has_bg=has_bg)


@pytest.mark.parametrize("name", ALL_SETS)
def test_ray_sets_are_not_vacuous(name):
    """Conditions, not tolerances.  Measured here on the CPU oracle, 600 rays a set -- share of the rays that hit at least
    once / twice / three times, that break, that read a neighbour; most hits and most draws on one ray; distinct colours:
        default_mb2          67.7 %  33.2 %   8.5 %  46.2 %  51.5 %   7  12  245
        default_mb8          67.7 %  33.2 %  16.8 %  37.0 %  51.5 %   8  18  260
        default_scaled_nobg  68.5 %  32.5 %  17.2 %  39.0 %  50.5 %   9  18   41   (no background: a ray that hits nothing stays black)
        synth64_mb4          25.3 %   6.7 %   2.2 %  12.7 %  14.7 %   6  18  218
        hand                 39.5 %  21.2 %  13.3 %   9.8 %  32.2 %  13  12  256
        big_table            52.2 %  20.8 %  14.5 %  18.0 %  37.2 %  19  18  240"""
    f = figures(name)
    print(name, f)
    if name.startswith("default"):
        assert f["hit1"] >= 0.5 and f["hit2"] >= 0.25 and f["broke"] >= 0.3 and f["nbr"] >= 0.4, f
        assert f["max_hits"] >= 6 and f["max_draws"] >= 12, f
        if f["has_bg"]:
            assert f["colours"] >= 100, f
    elif name == "synth64_mb4":
        assert f["hit1"] >= 0.2 and f["hit2"] >= 0.03, f
    else:
        assert f["hit1"] >= 0.3 and f["hit2"] >= 0.1, f
        sc = sr.ray_set(name)[0]
        m = sc.materials
        assert len(set(m[:, 3])) >= 3 and len(set(m[:, 5])) >= 4 and len(set(m[:, 6])) >= 2      # roughness, ior, energy varied
    assert f["max_draws"] <= sr.N_DRAWS


# ---- 2. the restatement against the oracle -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL_SETS)
def test_restatement_equals_the_oracle(name):
    """shade_ref.trace, record for record and traversed list for traversed list, on every ray set the GPU tests compare
    with the oracle."""
    sc, st, has_bg, origins, vels, lives, draws, exp, trav = sr.ray_set(name)
    got, gtrav = sr.trace_records(sc, st, origins, vels, lives, draws, has_bg)
    sr.assert_records_equal(got, exp)
    assert all(np.array_equal(a, b) for a, b in zip(gtrav, trav))


def test_restatement_reports_exhaustion():
    """With two draws per row the restatement marks exactly the rays whose oracle draw count exceeds 2."""
    sc, st, has_bg, origins, vels, lives, draws, exp, trav = sr.ray_set("default_mb8")
    got, _ = sr.trace_records(sc, st, origins[:150], vels[:150], lives[:150], draws[:150, :2], has_bg)
    out = exp["counters"][:150, sr.C_DRAW] > 2
    assert 0 < out.sum() < 150 and np.array_equal(got["s"] == -3, out)
    sr.assert_records_equal(got[~out], exp[:150][~out])


# ---- 3. the C ABI ------------------------------------------------------------------------------------------------------
def test_header_declares_the_entry_points():
    text = open(HEADER).read()
    assert re.search(r"int vrt_shade_workspace_bytes\(int64_t n_rays, int64_t\* bytes\);", text)
    assert re.search(r"int vrt_shade_rays\(const vrt_scene\* scene, const vrt_settings\* st, const vrt_cast_ray\* d_rays, "
                     r"int64_t n_rays,\s+double max_life, const double\* d_draws, int32_t n_draws, void\* d_workspace, "
                     r"int64_t workspace_bytes,\s+uint32_t\* d_rgba, vrt_ray\* d_records, uint64_t\* d_stats, "
                     r"const vrt_traversed\* trav, void\* stream\);", text)
    assert "#define VRT_ABI_VERSION 9" in text


def test_library_exports_the_entry_points():
    L = nat.lib()
    assert L.vrt_abi_version() == 9 and nat.ABI_VERSION == 9      # the change only adds symbols
    assert L.vrt_shade_rays is not None and L.vrt_shade_workspace_bytes is not None
    assert "vrt_shade_rays" in nat.EXPORTS and "vrt_shade_workspace_bytes" in nat.EXPORTS
    assert nat.RAY_REJECTED == -2 and nat.RAY_EXHAUSTED == -3 and nat.S_CAST_REJECTED == 9 and nat.S_RNG_EXHAUSTED == 10
    nb = C.c_int64(-1)
    assert L.vrt_shade_workspace_bytes(0, C.byref(nb)) == 0 and nb.value > 0
    small, big = nb.value, C.c_int64(-1)
    assert L.vrt_shade_workspace_bytes(1 << 31, C.byref(big)) == 0 and big.value == small      # nothing per ray
    assert L.vrt_shade_workspace_bytes(-1, C.byref(nb)) == -1 and L.vrt_shade_workspace_bytes(5, None) == -1


def test_shade_rays_rejects_bad_arguments_without_a_device():
    """Everything the entry point can refuse is refused before its first HIP call: these calls carry made-up device
    pointers, which nothing reads."""
    L = nat.lib()
    st = nat.VrtSettings(15, 11, 3, 8, 4, 1, 0, 0.875, .25, .25, .5, 0, 48, 1, 4, .5, .5, .25, .5)
    fake = 0x1000
    sc = nat.VrtScene()
    sc.origin[:] = [-24, -24, -24]
    sc.dims[:] = [6, 6, 6]
    sc.chunk_size, sc.n_slots, sc.n_materials, sc.max_resolution = 8, 10, 4, 1
    sc.d_chunk_table = sc.d_voxels = sc.d_materials = fake
    nb = C.c_int64(0)
    assert L.vrt_shade_workspace_bytes(100, C.byref(nb)) == 0

    def call(scene=sc, settings=st, rays=fake, n=100, max_life=48.0, draws=fake, n_draws=8, ws=fake, ws_bytes=nb.value, rgba=fake,
             records=fake, stats=fake, trav=None):
        return L.vrt_shade_rays(C.byref(scene) if scene is not None else None, C.byref(settings) if settings is not None else None,
                                rays, n, max_life, draws, n_draws, ws, ws_bytes, rgba, records, stats,
                                C.byref(trav) if trav is not None else None, None)

    assert call(scene=None) == -1 and call(settings=None) == -1 and call(stats=None) == -1
    assert call(rgba=None, records=None) == -1                       # either output may be NULL, not both
    assert call(rays=None) == -1 and call(rays=fake + 8) == -1        # the array is 64-byte aligned
    assert call(n=-1) == -1 and call(n=(1 << 32) - 1) == -1 and call(n=1 << 32) == -1
    assert call(max_life=0.0) == -1 and call(max_life=-1.0) == -1 and call(max_life=float("nan")) == -1
    assert call(max_life=float((1 << 28) + 1)) == -1 and call(max_life=float("inf")) == -1
    assert call(n_draws=-1) == -1 and call(draws=None, n_draws=3) == -1
    assert call(ws=None) == -1
    assert call(ws_bytes=nb.value - 1) == nat.ERR_WORKSPACE == -3 and call(ws_bytes=0) == -3
    odd = nat.VrtSettings(15, 11, 3, 12, 6, 1, 0, 0.875, .25, .25, .5, 0, 48, 1, 4, .5, .5, .25, .5)
    assert call(settings=odd) == -1                                   # check_settings: the chunk size is a power of two
    other = nat.VrtSettings(15, 11, 3, 16, 8, 1, 0, 0.875, .25, .25, .5, 0, 48, 1, 4, .5, .5, .25, .5)
    assert call(settings=other) == -1                                 # ... and the scene's
    nowin = nat.VrtSettings(0, 11, 3, 8, 4, 1, 0, 0.875, .25, .25, .5, 0, 48, 1, 4, .5, .5, .25, .5)
    assert call(settings=nowin) == -1                                 # ... checked like every settings block
    box = nat.VrtTraversed()
    box.origin[:] = [-20, -24, -24]                                   # a traversed box off the chunk grid
    box.dims[:] = [6, 6, 6]
    box.d_keys = fake
    assert call(trav=box) == -1
    box.origin[:] = [-24, -24, -24]
    box.dims[:] = [6, 0, 6]
    assert call(trav=box) == -1


# ---- 4. the compiler's resource report ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def report():
    return kernel_report.report()


def shade_name(spec, res, record):
    return "_Z12shade_kernelILi%dELi%dELb%dEEv11MarchParams" % (spec, res, 1 if record else 0)


# shade_kernel<SPEC, RESMODE, RECORD>: the instances the library launches (launch_shade's choice)
@pytest.mark.parametrize("record", [False, True])
@pytest.mark.parametrize("spec,res", [(8, 0), (8, 1), (4, 2)])
def test_shade_kernel_resources(report, spec, res, record):
    assert len([k for k in report if k.startswith("_Z12shade_kernel")]) == 6
    name = shade_name(spec, res, record)
    assert name in report, name
    r = report[name]
    assert r["VGPRs Spill"] == 0 and r["AGPRs"] == 0, r
    assert r["Occupancy [waves/SIMD]"] >= 4 and r["VGPRs"] <= 128, r
    if not record:
        assert r["ScratchSize [bytes/lane]"] <= 16, r      # the pow slow path's frame: the frame kernels' bound
    else:
        # the one record-keeping march instance the library has had so far: vrt_trace_rays's and vrt_render_tile's
        m = report["_Z12march_kernelILi4ELi2ELb1ELb0ELi0ELi4ELb0ELb0ELi0EEv11MarchParams"]
        for f in ("TotalSGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "SGPRs Spill", "VGPRs Spill", "LDS Size [bytes/block]"):
            assert r[f] <= m[f], (f, r, m)
        assert r["Occupancy [waves/SIMD]"] >= m["Occupancy [waves/SIMD]"], (r, m)
    # (every figure of the six instances is pinned with all the others: tests/test_kernel_resources.py)
