"""The GPU against the REAL reference outside the reference's own operating envelope: README's claim that the fp32 image and
the integer results are the reference's, checked on what the reference itself rendered and built, not on a restatement of it.

Renders (tests/golden/edges/, made by tests/golden/make_golden_edges.py): every camera of the edge scenes, the scene without a
background and the 14 boundary-camera frames of tests/edge_scenes.py, in the kernel choice the library ships -- no VRT_*
variable is set.  Per ray: pixel, sample, colour, alpha, the eight event counters and, where stored, the traversed count; per
frame: the fp32 means, the traversed list in order and the counter totals.  (tests/test_gpu_edges.py keeps pinning the double
fields of these scenes, bit for bit, to the oracle in its portable-libm mode, under every forced kernel choice;
tests/test_oracle_edges_golden.py pins that oracle to the same fixtures.)

World (tests/golden/world_random.npz, made by tests/golden/make_world_random.py): 64 objects, one per quarter-turn triple,
through vrt_voxelize and the owner pass against the reference's voxels and its own record of which object each came from."""
import json

import numpy as np
import pytest

import edge_scenes as es
from gpu_util import active, camera_for, settings_store

pytestmark = pytest.mark.gpu

RENDERS = [r[0] for r in es.reference_renders()]
INTEGERS = ("x", "y", "s", "color", "alpha", "counters", "ntrav")


@pytest.mark.parametrize("name", RENDERS)
def test_render_equals_the_reference(name):
    from python_raytracer_amd import data
    g = es.load_reference_render(name)
    sc, st = g["scene"], g["st"]
    cs = st["chunk_size"]
    background = data.background
    try:
        if not g["has_background"]:
            data.background = None
        cam = camera_for(sc, settings_store(st), g["cam_pos"], g["cam_rot"], g["cam_lens"][0])
        r = cam.render(0, want_rays=True)
        got, exp = active(r), g["ref_rays"]
        f32 = r.rgba_f32.cpu().numpy()
        trav = np.array(r.traversed(cs), np.int64).reshape(-1, 3)
    finally:
        data.background = background
    assert len(got) == len(exp) == int(r.stats[8]) == int(g["n_rays"][0])
    for f in INTEGERS:
        if f in exp.dtype.names:
            assert np.array_equal(got[f], exp[f]), (f, np.flatnonzero((got[f] != exp[f]).reshape(len(got), -1).any(1))[:5])
    assert "ntrav" in exp.dtype.names or "rays" not in g
    px = r.pixels
    assert np.array_equal(f32, g["pix_mean"][px[:, 1], px[:, 0]].astype(np.float32))
    assert np.array_equal(trav, g["ref_traversed"])
    assert (r.stats[:8] == g["counters_total"]).all(), (r.stats[:8], g["counters_total"])


# ---- the 64-object world -----------------------------------------------------------------------------------------------------
_world = {}


def random_world():
    """world_random.npz on the device, built once: fixture, objects, DeviceWorld, its PackedScene."""
    if not _world:
        from python_raytracer_amd.world import DeviceWorld
        from test_world import build_from_random_fixture, random_fixture
        z = random_fixture()
        mats, st, objs = build_from_random_fixture(z)
        dw = DeviceWorld(16)
        ps = dw.build(objs)
        _world.update(z=z, mats=mats, st=st, objs=objs, dw=dw, ps=ps)
    return _world


def test_device_world_equals_the_reference_world():
    """vrt_voxelize (DeviceWorld.build) on the 64-object spec: voxels and chunk presence are the reference's."""
    from test_world import _device_grid, _same_voxels
    g = random_world()
    z, dw, ps, mats = g["z"], g["dw"], g["ps"], g["mats"]
    assert list(dw.order) == [o for o in g["objs"] if o.visible] and len(dw.order) == 63
    table, grid = _device_grid(dw, ps)
    remap = np.zeros(len(dw.materials) + 1, np.uint8)
    for k, m in enumerate(dw.materials):
        remap[k + 1] = 1 + mats.index(m)
    assert _same_voxels(dw.origin, remap[grid], z["origin"], z["grid_lod0"])
    # presence: the chunks the table lists are the reference's chunks, by world position
    cs = 16
    mine = {tuple(int(v) for v in (np.asarray(dw.origin, np.int64) + c * cs)) for c in np.argwhere(table != 0)}
    ref = {tuple(int(v) for v in (z["origin"] + c * cs)) for c in np.argwhere(z["present"] != 0)}
    assert mine == ref and len(ref) > 40


def test_owner_pass_equals_the_reference_owners():
    """The owner pass over a hit record for EVERY non-empty voxel of the reference's grid -- a cast that starts at the voxel's
    centre stands in it at step 0 (Camera.cast_rays, as tests/test_gpu_owners.py makes its records) -- names the object the
    reference's own dict walk names, also at the voxels two objects hold; no orphans, no ambiguous records."""
    from python_raytracer_amd import _native as nat
    from test_gpu_owners import both_stagings, check_no_hit_records, check_stats, world_camera
    g = random_world()
    z, dw, objs = g["z"], g["dw"], g["objs"]
    cam = world_camera(g["st"], g["ps"], z["cam_pos"])
    assert json.loads(bytes(z["settings"]).decode())["chunk_lod"] == 0          # every chunk at resolution 1: cell = voxel
    voxels = np.argwhere(z["grid_lod0"] != 0) + z["origin"]
    n = len(voxels)
    assert n > 4000 and n % 256 != 0
    vel = np.tile([0.0, 0.0, 1.0], (n, 1))
    hits = cam.cast_rays(voxels + 0.5, vel, np.full(n, 1.0))
    h = hits.numpy()
    at = voxels - z["origin"]
    assert np.array_equal(h["cell"], voxels) and (h["step"] == 0).all()
    remap = np.zeros(len(dw.materials) + 1, np.int32)
    for k, m in enumerate(dw.materials):
        remap[k + 1] = 1 + g["mats"].index(m)
    assert np.array_equal(remap[h["material"]], z["grid_lod0"][at[:, 0], at[:, 1], at[:, 2]])
    res, own = both_stagings(dw, hits, cam)
    assert np.array_equal(own["voxel"], voxels) and (own["resolution"] == 1).all() and (own["object"] >= 0).all()
    spec = np.array([objs.index(o) for o in dw.order])[own["object"]]
    exp = z["owner"][at[:, 0], at[:, 1], at[:, 2]]
    assert np.array_equal(spec, exp), np.flatnonzero(spec != exp)[:5]
    check_no_hit_records(own, h)
    check_stats(res.stats, own, h, 0)
    assert int(res.stats[nat.S_OWNER_ORPHANS]) == 0 and int(res.stats[nat.S_OWNER_AMBIGUOUS]) == 0
    assert int(res.stats[nat.S_OWNER_RESOLVED]) == n and len(set(spec.tolist())) == 63
