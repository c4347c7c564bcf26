"""GPU: select_chunks_kernel where one ulp of the distance is a whole LOD.

The reference's chunk distance is math.dist (lib.py:297-298, init.py:448-449), which is not sqrt(dx*dx + dy*dy + dz*dz);
the two differ by an ulp on about one input in six, and min(trunc(dist / step), chunk_lod) turns that ulp into a LOD where
dist / step lands on an integer.  The random cameras of tests/test_gpu_edges.py::test_select_chunks_random_worlds never land
there, so that test cannot tell the two formulas apart.  These inputs can:

  a. every case of tests/golden/select_edges.npz -- what the real reference's Window.chunk_update gave its camera on exact
     ties, on 32 constructed pairs where the naive formula picks another LOD, with chunk_lod 0, chunk sizes 8..64, worlds
     2^24 cells out and culling -- through Camera.chunk_update;
  b. the device's distance itself, bit for bit, on the pairs of tests/golden/kat_dist.json.gz (math.dist of the CPython that
     produced the fixtures), read out of the raw vrt_select_chunks with the two-threshold bracket of tests/select_edges.py.

tests/test_select_edges_host.py holds the oracle to the same fixtures and shows on the CPU that the bracket is sharp."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as ol
from select_edges import KAT_CS, bracket_by, edge_cases, kat_dist, on_chunk_grid, oracle_select_one, thresholds

pytestmark = pytest.mark.gpu

IDENTITY = (0.0, 0.0, 0.0, 1.0)
CASES, _ = edge_cases()


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_chunk_update_selects_what_the_reference_selected(case):
    """Camera.chunk_update on a world of one presence voxel per chunk, with the fixture's settings, camera (float64) and
    traversed list: the table's presence, LOD byte and slot equal the fixture and the oracle, and the resolution bound the
    camera keeps for the frame kernels (_camera_table_max_res) is at least the largest LOD byte written."""
    from gpu_util import settings_store
    from python_raytracer_amd import Camera, PackedScene
    from python_raytracer_amd.lib import vec3, quaternion
    cs, dims = case.cs, case.dims
    sst = settings_store(ol.make_settings(width=8, height=8, chunk_size=cs, dist_max=case.dist_max, chunk_lod=case.chunk_lod))
    sst.culling = case.culling
    cam = Camera(settings=sst)
    grid = np.zeros(tuple(dims * cs), np.uint8)
    for c in case.cells:
        grid[tuple(c * cs)] = 1
    world = PackedScene.from_dense(case.origin, dims, cs, case.present, np.ones_like(case.present), grid, np.array([[1, 2, 3, 0, 1, 1, 0.0]]))
    cam.set_world_scene(world)
    cam.pos, cam.rot = vec3(*[float(v) for v in case.cam]), quaternion(*IDENTITY)
    assert (cam.pos.x, cam.pos.y, cam.pos.z) == tuple(case.cam.tolist())
    table = cam.chunk_update([tuple(int(v) for v in t) for t in case.trav]).cpu().numpy().view(np.uint32).reshape(tuple(dims))
    got_present, got_res = (table != 0).astype(np.uint8), (table >> 24).astype(np.uint8)
    assert np.array_equal(got_present, case.want_present), case.name
    assert np.array_equal(got_res, case.want_res), (case.name, got_res[case.present > 0], case.want_res[case.present > 0])
    assert np.array_equal(table[table != 0] & 0xffffff, world.chunk_table.reshape(tuple(dims))[table != 0] & 0xffffff)
    pres, res = case.oracle()
    assert np.array_equal(got_present, pres) and np.array_equal(got_res, res), case.name
    assert cam._camera_table_max_res >= int(got_res.max()), (cam._camera_table_max_res, int(got_res.max()))


def test_device_distance_is_math_dist_bit_for_bit():
    """Every kat_dist.json.gz pair whose centre lies on a chunk grid (all six families, about 1,980 pairs) through the raw
    vrt_select_chunks: a world of one chunk of size 8 at the pair's centre, chunk_lod 1, culling off, once with
    dist_max = 2 want and once with dist_max = 2 nextafter(want, inf).  The LODs 1 and 0 pin
    want <= device distance < nextafter(want, inf).  All launches go to the stream first, each into its own word of one
    output tensor; one copy reads them back.  The same bracket is first put to orc_select_chunks on the CPU."""
    import torch
    from python_raytracer_amd import _native as nat
    L = nat.lib()
    dev = torch.device("cuda", 0)
    fams = {k: [v for v in vecs if on_chunk_grid(v)] for k, vecs in kat_dist().items()}
    assert len(fams) == 6 and all(len(v) >= 100 for v in fams.values()), {k: len(v) for k, v in fams.items()}
    vecs = [v for f in fams.values() for v in f]
    assert len(vecs) >= 512
    for v in vecs:
        assert bracket_by(oracle_select_one, v), v.tolist()
    asks = [(i, t) for i, v in enumerate(vecs) for t in thresholds(float(v[6]))]
    world = torch.tensor([1 | (1 << 24)], dtype=torch.int32, device=dev)
    out = torch.full((len(asks),), -1, dtype=torch.int32, device=dev)
    dims = (C.c_int32 * 3)(1, 1, 1)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream().cuda_stream
        for n, (i, (_, dist_max, _)) in enumerate(asks):
            v = vecs[i]
            origin = (C.c_int64 * 3)(*[int(c) - KAT_CS // 2 for c in v[:3]])
            pos = (C.c_double * 3)(*[float(p) for p in v[3:6]])
            nat.check(L.vrt_select_chunks(world.data_ptr(), origin, dims, KAT_CS, pos, dist_max, 1, 0, None,
                                          out.data_ptr() + 4 * n, stream), "vrt_select_chunks")
        torch.cuda.synchronize()
    got = out.cpu().numpy().view(np.uint32)
    assert np.all((got & 0xffffff) == 1), "a chunk was dropped"
    lod = (got >> 24).astype(np.int64) - 1
    want = np.array([t[2] for _, t in asks])
    wrong = sorted({i for (i, _), g, w in zip(asks, lod, want) if g != w})
    assert not wrong, (len(wrong), [(vecs[i][:6].tolist(), float(vecs[i][6]).hex()) for i in wrong[:5]])
