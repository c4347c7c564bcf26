"""Explicit rays without a GPU: the references of tests/test_gpu_cast.py against each other (the Python restatement of the
reference's loop in tests/cast_ref.py, pinned to the CPU oracle), the C ABI's new symbol and record, what vrt_cast_rays
refuses before any HIP call, and the compiler's resource report of cast_kernel (tests/kernel_report.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import cast_ref as cr
import kernel_report
from python_raytracer_amd import _native as nat

HEADER = os.path.join(kernel_report.ROOT, "include", "vrt.h")


# ---- the restatement against the oracle --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["default", "synth64", "default_scaled", "default_dmin", "hand", "big_table"])
def test_restatement_equals_the_oracle(name):
    """cast_ref.march, record for record (step, pos and material; the doubles as bit patterns), on every ray set the GPU tests
    compare with the oracle.  Each set is asserted not to be vacuous when it is made (more than 10 % hits, more than 10 %
    misses, at least 3 materials).  Measured here on the CPU oracle -- rays, share of hits, materials found:
        default         1 500  50.9 %  12     (the default scene's camera grid: resolutions 1 and 2; |vel|_inf 0.58 .. 1)
        synth64         1 500  17.4 %  13     (identity table, resolution 1)
        default_scaled    500  55.2 %   9     (quaternions of norm 0.5 .. 1.5: |vel|_inf 0.18 .. 3.07)
        default_dmin      500  49.8 %  10     (dist_min = 3)
        hand              500  13.6 %   5     (origins in [-20, -12, -4] .. [20, 20, 20] around the box of resolutions 1, 2, 3)
        big_table         500  23.2 %   5     (origins in +-60)"""
    sc, origins, vels, lives, exp = cr.ray_set(name)
    cr.assert_not_vacuous(exp)
    got = cr.march_records(sc, round(sc.chunk_size / 2), origins, vels, lives)
    cr.assert_records_equal(got, exp)


# ---- the C ABI -----------------------------------------------------------------------------------------------------------
def test_header_declares_the_entry_point():
    text = open(HEADER).read()
    assert re.search(r"typedef struct vrt_cast_ray \{[^}]*double origin\[3\];[^}]*double vel\[3\];[^}]*double life;[^}]*"
                     r"double reserved;[^}]*\} vrt_cast_ray;", text, re.S)
    assert re.search(r"int vrt_cast_rays\(const vrt_scene\* scene, const vrt_settings\* st, const vrt_cast_ray\* d_rays, "
                     r"int64_t n_rays,\s+double max_life, vrt_hit\* d_hits, uint64_t\* d_stats, void\* stream\);", text)
    assert re.search(r"VRT_S_CAST_REJECTED = 9\b", text) and "#define VRT_ABI_VERSION 9" in text


def test_library_exports_the_entry_point():
    L = nat.lib()
    assert L.vrt_abi_version() == 9 and nat.ABI_VERSION == 9      # the change only adds a symbol
    assert L.vrt_cast_rays is not None and "vrt_cast_rays" in nat.EXPORTS
    assert C.sizeof(nat.VrtCastRay) == 64 == nat.CAST_RAY_BYTES
    assert [getattr(nat.VrtCastRay, f).offset for f in ("origin", "vel", "life", "reserved")] == [0, 24, 48, 56]
    assert nat.S_CAST_REJECTED == 9 and nat.HIT_REJECTED == -2


def test_cast_rays_rejects_bad_arguments_without_a_device():
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

    def call(scene=sc, settings=st, rays=fake, n=100, max_life=48.0, hits=fake, stats=fake):
        return L.vrt_cast_rays(C.byref(scene) if scene is not None else None, C.byref(settings) if settings is not None else None,
                               rays, n, max_life, hits, stats, None)

    assert call(rays=None) == -1 and call(hits=None) == -1 and call(stats=None) == -1
    assert call(max_life=0.0) == -1 and call(max_life=-1.0) == -1 and call(max_life=float("nan")) == -1
    assert call(max_life=float((1 << 28) + 1)) == -1 and call(max_life=float("inf")) == -1
    assert call(n=-1) == -1 and call(n=1 << 32) == -1
    assert call(rays=fake + 8) == -1                    # the array is 64-byte aligned
    assert call(scene=None) == -1 and call(settings=None) == -1
    odd = nat.VrtSettings(15, 11, 3, 12, 6, 1, 0, 0.875, .25, .25, .5, 0, 48, 1, 4, .5, .5, .25, .5)
    assert call(settings=odd) == -1                     # check_settings: the chunk size is a power of two
    other = nat.VrtSettings(15, 11, 3, 16, 8, 1, 0, 0.875, .25, .25, .5, 0, 48, 1, 4, .5, .5, .25, .5)
    assert call(settings=other) == -1                   # ... and the scene's


# ---- the compiler's resource report ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def report():
    return kernel_report.report()


# cast_kernel<SPEC, RESMODE>: the instances the library launches (launch_first_hit's choice)
@pytest.mark.parametrize("spec,res", [(8, 0), (8, 1), (4, 2)])
def test_cast_kernel_resources(report, spec, res):
    name = "_Z11cast_kernelILi%dELi%dEEv11MarchParams" % (spec, res)
    assert name in report, name
    r = report[name]
    siblings = [v for k, v in report.items() if k.startswith("_Z16first_hit_kernelILi%dELi%dE" % (spec, res))]
    assert len(siblings) == 4
    assert r["VGPRs Spill"] == 0 and r["AGPRs"] == 0, r
    assert r["Occupancy [waves/SIMD]"] >= 4 and r["VGPRs"] <= 128, r
    assert r["ScratchSize [bytes/lane]"] <= min(s["ScratchSize [bytes/lane]"] for s in siblings), r
    # (every figure of cast_kernel and first_hit_kernel is pinned with all the others: tests/test_kernel_resources.py)
