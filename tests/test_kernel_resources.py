"""The frame march kernels must keep four waves per SIMD without vector spills: the compiler's own resource report
(-Rpass-analysis=kernel-resource-usage) of the shipped source, cross-compiled for gfx950 (no GPU needed: tests/kernel_report.py).
A change that pushes a frame kernel over 128 VGPRs costs tens of per cent on the GPU and would otherwise only show up in a
bench run.  And every figure of every device function is pinned: the report equals profiles/kernel_resource_usage.txt."""
import re

import pytest

import kernel_report

# mangled names of the kernels a frame runs at the BASELINE configurations
# (the last template arguments: W = the look-ahead crosses chunk borders, march_step_w -- the measured variant, VRT_WADDR=1;
# DEFER = the launch's traversed box has no settled bitmap and a re-snap's key is compared after the voxel reads went out;
# march_pool_kernel's TILE = rays handed out as square pixel tiles, an eighth of the window per XCD -- the measured variant, VRT_TILED=1)
FRAME_KERNELS = {
    "_Z17march_pool_kernelILi8ELi1ELi0ELb0ELb0ELb0EEv11MarchParams": "march_pool_kernel<8,1,0,false,false,false> (config 3)",
    "_Z17march_pool_kernelILi8ELi0ELi1ELb0ELb1ELb0EEv11MarchParams": "march_pool_kernel<8,0,1,false,true,false> (config 5: keys compared late)",
    "_Z12march_kernelILi8ELi1ELb0ELb0ELi0ELi0ELb0ELb0ELi0EEv11MarchParams": "march_kernel<8,1,false,false,0,0,false,false> (config 2)",
    "_Z12march_kernelILi8ELi0ELb0ELb0ELi0ELi2ELb0ELb1ELi0EEv11MarchParams": "march_kernel<8,0,false,false,0,2,false,true>",
    "_Z17march_pool_kernelILi8ELi0ELi1ELb0ELb0ELb0EEv11MarchParams": "march_pool_kernel<8,0,1,false,false,false>",
    "_Z17march_pool_kernelILi8ELi1ELi0ELb0ELb1ELb0EEv11MarchParams": "march_pool_kernel<8,1,0,false,true,false>",
    "_Z12march_kernelILi8ELi0ELb0ELb0ELi0ELi0ELb0ELb0ELi0EEv11MarchParams": "march_kernel<8,0,false,false,0,0,false,false>",
    "_Z17march_pool_kernelILi8ELi1ELi0ELb1ELb0ELb0EEv11MarchParams": "march_pool_kernel<8,1,0,true,false,false> (look-ahead variant)",
    "_Z17march_pool_kernelILi8ELi0ELi1ELb1ELb0ELb0EEv11MarchParams": "march_pool_kernel<8,0,1,true,false,false> (look-ahead variant)",
    "_Z12march_kernelILi8ELi1ELb0ELb0ELi0ELi0ELb1ELb0ELi0EEv11MarchParams": "march_kernel<8,1,false,false,0,0,true,false> (look-ahead variant)",
    "_Z17march_pool_kernelILi8ELi0ELi1ELb0ELb1ELb1EEv11MarchParams": "march_pool_kernel<8,0,1,false,true,true> (tiled hand-out variant)",
    "_Z17march_pool_kernelILi8ELi1ELi0ELb0ELb1ELb1EEv11MarchParams": "march_pool_kernel<8,1,0,false,true,true> (tiled hand-out variant)",
}
# frames without a cached ray table: the lanes make their own ray records (take_ray, PERPIX 3) -- the sines and cosines of the
# lens quaternion bring constants (scalar registers spilled around them, in the refill only) and the out-of-line slow path's
# call frame, but must not cost the march its four waves
RAYGEN_KERNELS = {
    "_Z17march_pool_kernelILi8ELi1ELi3ELb0ELb0ELb0EEv11MarchParams": "march_pool_kernel<8,1,3,false,false,false> (config 3 --reseed)",
    "_Z17march_pool_kernelILi8ELi0ELi3ELb0ELb0ELb0EEv11MarchParams": "march_pool_kernel<8,0,3,false,false,false>",
    "_Z17march_pool_kernelILi8ELi1ELi3ELb0ELb1ELb0EEv11MarchParams": "march_pool_kernel<8,1,3,false,true,false>",
    "_Z17march_pool_kernelILi8ELi0ELi3ELb0ELb1ELb0EEv11MarchParams": "march_pool_kernel<8,0,3,false,true,false>",
    "_Z12march_kernelILi8ELi1ELb0ELb0ELi0ELi3ELb0ELb0ELi0EEv11MarchParams": "march_kernel<8,1,false,false,0,3,false,false> (config 2 --reseed)",
    "_Z12march_kernelILi8ELi0ELb0ELb0ELi0ELi3ELb0ELb0ELi0EEv11MarchParams": "march_kernel<8,0,false,false,0,3,false,false>",
    "_Z12march_kernelILi8ELi1ELb0ELb0ELi0ELi3ELb0ELb1ELi0EEv11MarchParams": "march_kernel<8,1,false,false,0,3,false,true>",
    "_Z12march_kernelILi8ELi0ELb0ELb0ELi0ELi3ELb0ELb1ELi0EEv11MarchParams": "march_kernel<8,0,false,false,0,3,false,true>",
}


@pytest.fixture(scope="module")
def report():
    return kernel_report.report()


def test_report_is_the_saved_one(report):
    """Every device function the compiler reports on -- the same names in the same order of emission -- has the eight figures
    profiles/kernel_resource_usage.txt holds for it.  A kernel change that moves one on purpose regenerates the file in the
    same commit (python tests/kernel_report.py --write)."""
    saved = kernel_report.saved()
    assert len(saved) == 132 and all(tuple(figs) == kernel_report.FIGURES for figs in saved.values())
    assert list(report) == list(saved)
    for name, figs in saved.items():
        assert report[name] == figs, (name, report[name], figs)


@pytest.mark.parametrize("name", sorted(FRAME_KERNELS))
def test_frame_kernels_keep_four_waves_without_vector_spills(report, name):
    assert name in report, "kernel %s not in the library any more" % FRAME_KERNELS[name]
    r = report[name]
    assert r["VGPRs Spill"] == 0, (FRAME_KERNELS[name], r)
    assert r["Occupancy [waves/SIMD]"] >= 4, (FRAME_KERNELS[name], r)
    assert r["VGPRs"] <= 128 and r["AGPRs"] == 0, (FRAME_KERNELS[name], r)
    # 16 bytes: the call frame of the pow slow path; anything more is ray state in scratch memory
    assert r["ScratchSize [bytes/lane]"] <= 16, (FRAME_KERNELS[name], r)
    # scalar registers spilled to vector lanes cost a v_readlane per use -- VALU work.  Round 3's kernels had 21 (ray pool) /
    # 6-9 (one ray per lane); the re-snap's wave-uniform switches now travel as one re-read word (MarchParams::snap_flags)
    # instead of as hoisted 64-bit lane masks, and the ray pool's march step re-reads its arguments (VRT_FRESH_MARCH_POOL):
    # 6 / 4 in the shipped kernels (the measured variants -- look-ahead, tiled hand-out -- up to 24)
    assert r["SGPRs Spill"] <= (24 if "variant" in FRAME_KERNELS[name] else 8), (FRAME_KERNELS[name], r)


@pytest.mark.parametrize("name", sorted(RAYGEN_KERNELS))
def test_kernels_that_make_their_ray_records_keep_four_waves(report, name):
    assert name in report, "kernel %s not in the library any more" % RAYGEN_KERNELS[name]
    r = report[name]
    assert r["VGPRs Spill"] == 0 and r["Occupancy [waves/SIMD]"] >= 4 and r["VGPRs"] <= 128 and r["AGPRs"] == 0, (RAYGEN_KERNELS[name], r)
    assert r["ScratchSize [bytes/lane]"] <= 64 and r["SGPRs Spill"] <= 112, (RAYGEN_KERNELS[name], r)


def test_static_lds_of_the_frame_kernels(report):
    """tests/test_gpu_lds_room.py places its scenes between byte thresholds that rest on the static LDS of the frame kernels
    (gpu_util.STATIC_LDS): every march_kernel / march_pool_kernel instance has the one figure or the other, by whether it
    looks ahead across chunk borders (the look-ahead variants keep their offset tables in dynamic LDS)."""
    from gpu_util import STATIC_LDS
    frame = {n: r for n, r in report.items() if re.match(r"_Z(12march_kernel|17march_pool_kernel)I", n)}
    assert len(frame) >= len(FRAME_KERNELS) + len(RAYGEN_KERNELS)
    for n, r in frame.items():
        ahead = "variant" in FRAME_KERNELS.get(n, "") and "look-ahead" in FRAME_KERNELS[n]
        if n not in FRAME_KERNELS:   # (march_pool_kernel<SPEC, RES, PERPIX, W, ...>, march_kernel<SPEC, RES, RECORD, LIST, LK, PERPIX, W, ...>)
            args = re.findall(r"L[ib](\d+)E", n)
            ahead = args[3 if "pool" in n else 6] == "1"
        assert r["LDS Size [bytes/block]"] == STATIC_LDS[ahead], (n, r["LDS Size [bytes/block]"])
    assert {STATIC_LDS[True], STATIC_LDS[False]} == {r["LDS Size [bytes/block]"] for r in frame.values()}
