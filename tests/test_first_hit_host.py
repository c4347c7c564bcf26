"""The first-hit pass without a GPU: the C ABI's new symbols and record layout, what the entry points refuse before any HIP
call, and the compiler's resource report of first_hit_kernel (cross-compiled for gfx950: tests/kernel_report.py)."""
import ctypes as C

import numpy as np
import pytest

import kernel_report
from python_raytracer_amd import _native as nat


def test_library_exports_the_first_hit_entry_points():
    L = nat.lib()
    assert L.vrt_abi_version() == 9 and nat.ABI_VERSION == 9      # the change only adds symbols
    for name in ("vrt_first_hit", "vrt_first_hit_views", "vrt_first_hit_views_workspace_bytes"):
        assert getattr(L, name) is not None and name in nat.EXPORTS


def test_hit_record_layout():
    assert C.sizeof(nat.VrtHit) == 48 == nat.HIT_BYTES
    assert [getattr(nat.VrtHit, f).offset for f in ("step", "pos", "cell", "material")] == [0, 8, 32, 44]
    dt = np.dtype(nat.HIT_FIELDS)
    assert dt.itemsize == 48 and [dt.fields[f][1] for f in ("step", "pos", "cell", "material")] == [0, 8, 32, 44]


def test_hit_result_views_one_record_buffer():
    """HitResult's tensors are views of the record buffer, and its images scatter sample 0 to (y, x)."""
    import torch
    from python_raytracer_amd import HitResult
    rec = np.zeros(6, np.dtype(nat.HIT_FIELDS))          # 3 pixels x 2 sample slots
    rec["step"] = [1.5, 2.5, 7.0, 0.0, 4.25, 4.5]
    rec["material"] = [3, 0, 0, -1, 9, 9]
    rec["pos"] = np.arange(18).reshape(6, 3) + 0.5
    rec["cell"] = np.arange(18).reshape(6, 3)
    buf = torch.from_numpy(rec.view(np.uint8).copy())
    px = np.array([[0, 0], [2, 1], [1, 2]], np.int32)
    h = HitResult(buf, px, 2, 2, 3, 4, torch.arange(16))
    assert h.step.data_ptr() == buf.data_ptr() and h.material.data_ptr() == buf.data_ptr() + 44
    assert np.array_equal(h.step.numpy(), rec["step"]) and np.array_equal(h.pos.numpy(), rec["pos"])
    assert np.array_equal(h.cell.numpy(), rec["cell"]) and np.array_equal(h.material.numpy(), rec["material"])
    assert h.step.dtype == torch.float64 and h.cell.dtype == torch.int32 and int(h.stats[8]) == 8
    inf = np.inf
    assert np.array_equal(h.depth_image().numpy(), [[1.5, inf, inf, inf], [inf, inf, inf, inf], [inf, 4.25, inf, inf]])
    assert np.array_equal(h.material_image().numpy(), [[3, -1, -1, -1], [-1, -1, 0, -1], [-1, 9, -1, -1]])


def test_first_hit_rejects_bad_arguments_without_a_device():
    """Everything the entry points can refuse is refused before their first HIP call: these calls carry made-up device
    pointers, which nothing reads."""
    L = nat.lib()
    W, H, SAMPLES, CS = 15, 11, 3, 8
    st = nat.VrtSettings(W, H, SAMPLES, CS, 4, 1, 0, 0.875, .25, .25, .5, 0, 48, 1, 4, .5, .5, .25, .5)
    fake = 0x1000
    sc = nat.VrtScene()
    sc.origin[:] = [-24, -24, -24]
    sc.dims[:] = [6, 6, 6]
    sc.chunk_size, sc.n_slots, sc.n_materials, sc.max_resolution = CS, 10, 4, 1
    sc.d_chunk_table = sc.d_voxels = sc.d_materials = fake
    n_px = W * H
    cam = nat.VrtCamera()
    cam.rot[3] = 1.0

    def call(camera=cam, settings=st, px=fake, plan=fake, rtab=fake, hits=fake, stats=fake, n_distinct=100):
        return L.vrt_first_hit(C.byref(sc), C.byref(settings), C.byref(camera), px, n_px, plan, n_distinct, rtab, 0, hits, stats, None)

    assert call(rtab=None) == -1                    # the ray table is required
    assert call(hits=None) == -1 and call(stats=None) == -1 and call(px=None) == -1 and call(plan=None) == -1
    assert call(n_distinct=-1) == -1 and call(n_distinct=10 ** 9) == -1
    far = nat.VrtCamera()
    far.rot[3] = 1.0
    far.pos[1] = float(1 << 28)
    assert call(camera=far) == -1                   # vrt_render_tile's range rule
    far.pos[1] = float("nan")
    assert call(camera=far) == -1
    nonstatic = nat.VrtSettings(W, H, SAMPLES, CS, 4, 1, 77, 0.875, .25, .25, .5, 0, 48, 1, 4, .5, .5, .25, .5)
    assert call(settings=nonstatic) == -1           # the ray table is a static-seed run's

    nb = C.c_int64(0)
    assert L.vrt_first_hit_views_workspace_bytes(5, C.byref(nb)) == 0 and nb.value >= 5 * 80
    assert L.vrt_first_hit_views_workspace_bytes(0, C.byref(nb)) == -1

    def views(cams=fake, n_views=5, rtab=fake, ws=fake, ws_bytes=1 << 20, npx=n_px):
        return L.vrt_first_hit_views(C.byref(sc), C.byref(st), cams, n_views, fake, npx, fake, 100, rtab, 0, ws, ws_bytes, fake,
                                     fake, None)

    assert views(cams=None) == -1 and views(n_views=0) == -1 and views(rtab=None) == -1 and views(ws=None) == -1
    assert views(ws_bytes=5 * 80 - 1) == nat.ERR_WORKSPACE
    assert views(n_views=1 << 20, npx=1 << 20, ws_bytes=1 << 40) == -1     # 2^32 slots and more


# ---- the compiler's resource report ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def report():
    return kernel_report.report()


# first_hit_kernel<SPEC, RESMODE, PERPIX, VIEWS>: the instances the library launches, and the frame's march_kernel of the same
# SPEC / RESMODE and ray-table layout (march_kernel<SPEC, RESMODE, false, false, 0, PERPIX 0 | 2 (asked at run time)>)
INSTANCES = [(spec, res, pp, views) for spec, res in ((8, 0), (8, 1), (4, 2)) for pp in (0, 1) for views in (0, 1)]


@pytest.mark.parametrize("spec,res,pp,views", INSTANCES)
def test_first_hit_kernel_resources(report, spec, res, pp, views):
    name = "_Z16first_hit_kernelILi%dELi%dELi%dELb%dEEv11MarchParams" % (spec, res, pp, views)
    sibling = "_Z12march_kernelILi%dELi%dELb0ELb0ELi0ELi%dELb0ELb0ELi0EEv11MarchParams" % (spec, res, 2 if pp else 0)
    assert name in report and sibling in report, (name, sibling)
    r, m = report[name], report[sibling]
    assert r["VGPRs Spill"] == 0 and r["AGPRs"] == 0, r
    assert r["ScratchSize [bytes/lane]"] == 0, r
    assert r["Occupancy [waves/SIMD]"] >= 4, r
    assert r["VGPRs"] <= m["VGPRs"], (r, m)
