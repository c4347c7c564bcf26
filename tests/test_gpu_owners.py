"""The owner pass on the GPU (DeviceWorld.owners / Camera.pick -> vrt_hit_owners, owner_kernel): which object, and which voxel
of its model, every hit record of first_hit() and cast_rays() belongs to.  The references are independent of the kernel: the
host world's owner grid (build_world(owners=True), pinned to the real reference by tests/test_owner_host.py -- it runs forward
over voxels, the kernel backward over objects) and the restated rule "which voxel a record means" (tests/owner_ref.py, checked
against a march that knows the truth in the same file).  Every comparison runs with the object records read from memory and
staged in LDS (VRT_OWNER_LDS, read at every call)."""
import os

import numpy as np
import pytest

import cast_ref as cr
import oracle_lib as ol
import owner_ref as orf
from gpu_util import camera_for, settings_store
from python_raytracer_amd import _native as nat
from python_raytracer_amd.lib import quaternion, vec3
from python_raytracer_amd.world import DeviceWorld, build_world
from test_world import _redraw_sequence, build_from_fixture

gpu = pytest.mark.gpu
IDENTITY = (0.0, 0.0, 0.0, 1.0)
OWNER_WORDS = [nat.S_OWNER_RESOLVED, nat.S_OWNER_EXAMINED, nat.S_OWNER_ORPHANS, nat.S_OWNER_AMBIGUOUS]


def same(a, b):
    """Two arrays of vrt_owner records are equal, word for word."""
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


def both_stagings(dw, hits, cam):
    """dw.owners() with the object records read from memory and staged in LDS: the records and statistics must not differ.
    Returns (OwnerResult, records as numpy)."""
    out = []
    for v in ("0", "1"):
        os.environ["VRT_OWNER_LDS"] = v
        try:
            res = dw.owners(hits, cam)
            out.append((res, res.numpy(), res.stats.copy()))
        finally:
            del os.environ["VRT_OWNER_LDS"]
    assert same(out[0][1], out[1][1]) and np.array_equal(out[0][2], out[1][2])
    default = dw.owners(hits, cam)
    assert same(default.numpy(), out[0][1]) and np.array_equal(default.stats, out[0][2])
    return out[1][0], out[1][1]


def check_stats(stats, own, hits, ambiguous):
    assert int(stats[nat.S_OWNER_EXAMINED]) == int((hits["material"] > 0).sum()), stats
    assert int(stats[nat.S_OWNER_RESOLVED]) == int((own["object"] >= 0).sum()), stats
    assert int(stats[nat.S_OWNER_ORPHANS]) == int((own["object"] == -2).sum()), stats
    assert int(stats[nat.S_OWNER_AMBIGUOUS]) == ambiguous, stats
    assert (np.delete(stats, OWNER_WORDS) == 0).all(), stats


def check_no_hit_records(own, hits):
    """Every record that is no hit -- a miss, an unused sample slot, a rejected ray -- is -1 with zero fields."""
    none = hits["material"] <= 0
    assert (own["object"][none] == -1).all() and (own["object"][~none] != -1).all()
    assert not own["resolution"][none].any() and not own["voxel"][none].any() and not own["local"][none].any()


def camera_scene(cam, dw, w):
    """The scene the camera marches, as an oracle_lib.Scene over the host world `w` (the table of its last chunk_update())."""
    assert np.array_equal(dw.origin, w.origin) and np.array_equal(dw.dims, w.dims)
    table = (cam._camera_table if cam._camera_table is not None else cam._world.device_tensors["chunk_table"])
    table = table.cpu().numpy().view(np.uint32).reshape(tuple(int(d) for d in w.dims))
    present, res = (table != 0).astype(np.uint8), (table >> 24).astype(np.uint8)
    grid = ol.Scene.camera_grid(w.grid, w.origin, w.dims, w.chunk_size, present, res)
    return ol.Scene(w.origin, w.dims, w.chunk_size, present, res, grid, cr.id_materials(max(len(w.materials), 1)))


def world_camera(st, ps, pos):
    from python_raytracer_amd import Camera
    cam = Camera(settings=st)
    cam.pos = vec3(*[float(v) for v in pos])
    cam.rot = quaternion(0.0, 0.0, 0.0, 1.0)
    cam.set_world_scene(ps)
    cam.chunk_update(None)
    return cam


_golden = {}


def golden():
    """The world of world_build.npz on the device, its camera, a full first-hit frame and 600 casts through the region where
    the slab and the cube overlap (234 of them aimed at the 9 voxels both objects hold)."""
    if not _golden:
        z = np.load(os.path.join(ol.GOLDEN, "world_build.npz"))
        mats, st, objs = build_from_fixture(z)
        dw = DeviceWorld(16)
        ps = dw.build(objs)
        cam = world_camera(st, ps, z["cam_pos"])
        cam.lens = float(z["cam_lens"][0])
        shared = orf.shared_voxels(objs[0], objs[1], 16)
        casts = orf.casts_at(shared, shared.min(0) - 6, shared.max(0) + 7, 366, 5)
        _golden.update(z=z, st=st, ps=ps, objs=objs, dw=dw, cam=cam, shared={tuple(p) for p in shared.tolist()}, casts=casts)
    return _golden


# ---- 5. the golden world ---------------------------------------------------------------------------------------------------
@gpu
def test_golden_world_owners():
    g = golden()
    dw, cam, objs = g["dw"], g["cam"], g["objs"]
    order = list(dw.order)
    assert order == [o for o in objs if o.visible]
    w = build_world(order, 16, owners=True)
    sc = camera_scene(cam, dw, w)
    assert set(np.unique(sc.res[sc.present != 0]).tolist()) == {1, 2}
    frame = cam.first_hit(all_samples=True)
    cast = cam.cast_rays(*g["casts"])
    owned, on_shared = set(), 0
    for hits in (frame, cast):
        res, own = both_stagings(dw, hits, cam)
        h = hits.numpy()
        exp, ambiguous = orf.expect_owners(sc, w, order, h)
        assert ambiguous == 0 and not (exp["object"] == -2).any()
        for f in ("object", "resolution", "voxel", "local"):
            assert np.array_equal(own[f], exp[f]), f
        ok = own["object"] >= 0
        assert ok.sum() > 100
        r = own["resolution"][ok][:, None]
        assert np.array_equal(own["voxel"][ok], (h["cell"][ok] // r) * r)
        for k in np.flatnonzero(ok):
            ob = order[int(own["object"][k])]
            assert orf.host_owner_at(w, own["voxel"][k]) == int(own["object"][k])
            assert orf.model_material(ob, own["local"][k], dw.materials) == int(h["material"][k]), k
        check_no_hit_records(own, h)
        check_stats(res.stats, own, h, 0)
        assert int(res.stats[nat.S_OWNER_ORPHANS]) == 0
        owned |= set(own["object"][ok].tolist())
        on_shared += sum(tuple(v) in g["shared"] for v in own["voxel"][ok].tolist())
    assert len(owned) >= 3 and on_shared >= 10, (owned, on_shared)


# ---- 6. the merge order after updates --------------------------------------------------------------------------------------
@gpu
def test_owners_follow_the_merge_order_after_updates():
    """world_update.npz's two redraws through DeviceWorld.update(): the owners of the same casts are the reference's own
    (world_owners.npz, by identity), and the winner where the slab and the cube overlap flips between ticks 0 and 1."""
    z = np.load(os.path.join(ol.GOLDEN, "world_build.npz"))
    seq = np.load(os.path.join(ol.GOLDEN, "world_update.npz"))
    ref = np.load(os.path.join(ol.GOLDEN, "world_owners.npz"))
    mats, st, objs = build_from_fixture(z)
    dw = DeviceWorld(16)
    ps = dw.build(objs)
    shared = orf.shared_voxels(objs[0], objs[1], 16)
    shared_set = {tuple(p) for p in shared.tolist()}
    casts = orf.casts_at(shared, shared.min(0) - 6, shared.max(0) + 7, 366, 5)

    def tick(tag, ps):
        cam = world_camera(st, ps, z["cam_pos"])
        hits = cam.cast_rays(*casts)
        res, own = both_stagings(dw, hits, cam)
        ok = own["object"] >= 0
        assert ok.sum() > 100 and not (own["object"] == -2).any() and int(res.stats[nat.S_OWNER_AMBIGUOUS]) == 0
        spec = np.array([objs.index(o) for o in dw.order])[own["object"][ok]]
        at = own["voxel"][ok] - seq["origin_" + tag]
        assert np.array_equal(spec, ref["owner_" + tag][at[:, 0], at[:, 1], at[:, 2]]), tag
        return {tuple(v): int(s) for v, s in zip(own["voxel"][ok].tolist(), spec) if tuple(v) in shared_set}

    won = [tick("0", ps)]
    cam_pos = vec3(*[float(v) for v in z["cam_pos"]])
    for tag, changed in _redraw_sequence(objs, st, cam_pos, seq):
        for o in objs:
            if id(o) in changed:
                o.redraw = True
        before = (dw._objects_dev, dw._remap_dev)
        ps, rebuilt = dw.update(objs)
        assert rebuilt > 0 and [objs.index(o) for o in dw.order] == seq["order_" + tag].tolist()
        assert dw._objects_dev is not before[0]                 # (the records follow the new order)
        won.append(tick(tag, ps))
    both = set(won[0]) & set(won[1])
    assert len(both) > 0 and any(won[0][v] != won[1][v] for v in both)
    kept = (dw._objects_dev, dw._remap_dev)
    assert dw.update(objs)[1] == 0 and dw._objects_dev is kept[0] and dw._remap_dev is kept[1]   # nothing changed: kept


# ---- 7. LOD and the face case ----------------------------------------------------------------------------------------------
@gpu
def test_lod_chunks_and_the_face_case():
    lw = orf.lod_world()
    sc, w, objs, truth = lw["scene"], lw["world"], lw["objs"], lw["truth"]
    assert {t[4] for t in truth if t[2]} == {1, 2, 3}          # (checked on the CPU first: all three resolutions are hit)
    st = ol.make_settings(width=32, height=24, samples=1, chunk_size=16, dist_max=64)
    cam = camera_for(sc, settings_store(st), (0.0, 0.0, 0.0), IDENTITY, st["fov"] * np.pi / 8)
    assert int(cam._c_scene(cam._ensure_scene()).max_resolution) == 3
    dw = DeviceWorld(16)
    dw.build(objs)
    assert list(dw.order) == objs and [id(m) for m in dw.materials] == [id(m) for m in w.materials]
    hits = cam.cast_rays(lw["origins"], lw["vels"], lw["lives"])
    h = hits.numpy()
    for k, t in enumerate(truth):                               # the march itself is the restatement's
        assert (h["step"][k], h["pos"][k].tolist(), int(h["material"][k])) == (t[0], t[1], t[2]), k
    res, own = both_stagings(dw, hits, cam)
    faces = 0
    for k, (step, pos, mat, cell, r, c) in enumerate(truth[:-1]):
        if not mat:
            assert int(own["object"][k]) == -1
            continue
        assert (int(own["resolution"][k]), tuple(own["voxel"][k].tolist())) == (r, c), k
        assert int(own["object"][k]) == orf.host_owner_at(w, c), k
        faces += orf.is_face_case(sc, pos, cell)
    assert faces >= 5
    exp, ambiguous = orf.expect_owners(sc, w, objs, h)
    assert ambiguous == 1 and same(own, exp)
    # the constructed record: two chunks explain it, and the documented first candidate -- the chunk containing floor(pos),
    # B's voxel -- is reported although the march read A's
    a, b = len(objs) - 2, len(objs) - 1
    assert truth[-1][5] == (30, 21, 6) and orf.host_owner_at(w, (30, 21, 6)) == a
    assert (int(own["object"][-1]), int(own["resolution"][-1]), own["voxel"][-1].tolist()) == (b, 1, [32, 21, 6])
    check_no_hit_records(own, h)
    check_stats(res.stats, own, h, 1)
    assert int(res.stats[nat.S_OWNER_AMBIGUOUS]) == 1 and int(res.stats[nat.S_OWNER_ORPHANS]) == 0


# ---- 8. orphans and foreign scenes -----------------------------------------------------------------------------------------
@gpu
def test_orphans_and_foreign_scenes():
    import torch
    g = golden()
    cam = g["cam"]
    frame = cam.first_hit(all_samples=True)
    h = frame.numpy()
    assert (h["material"] > 0).sum() > 100
    # no objects at all: every hit is an orphan
    empty = DeviceWorld(16)
    empty.build([])
    res, own = both_stagings(empty, frame, cam)
    assert (own["object"][h["material"] > 0] == -2).all()
    check_no_hit_records(own, h)
    check_stats(res.stats, own, h, 0)
    assert int(res.stats[nat.S_OWNER_ORPHANS]) == int((h["material"] > 0).sum()) and int(res.stats[nat.S_OWNER_RESOLVED]) == 0
    # another world's object list against this scene, and this world's hits against another scene: an orphan, or -- where the
    # foreign data happens to explain the record -- an owner whose model does hold the record's material
    lw = orf.lod_world()
    foreign = DeviceWorld(16)
    foreign.build(lw["objs"])
    st = ol.make_settings(width=32, height=24, samples=1, chunk_size=16, dist_max=64)
    lod_cam = camera_for(lw["scene"], settings_store(st), (0.0, 0.0, 0.0), IDENTITY, st["fov"] * np.pi / 8)
    lod_hits = lod_cam.cast_rays(lw["origins"], lw["vels"], lw["lives"])
    orphans = 0
    for dw, hits, c in ((foreign, frame, cam), (g["dw"], lod_hits, cam), (g["dw"], lod_hits, lod_cam), (foreign, frame, lod_cam)):
        res, own = both_stagings(dw, hits, c)
        hh = hits.numpy()
        check_no_hit_records(own, hh)
        assert int(res.stats[nat.S_OWNER_ORPHANS]) == int((own["object"] == -2).sum())
        assert int(res.stats[nat.S_OWNER_EXAMINED]) == int((hh["material"] > 0).sum())
        assert int(res.stats[nat.S_OWNER_RESOLVED]) == int((own["object"] >= 0).sum())
        orphans += int((own["object"] == -2).sum())
        for k in np.flatnonzero(own["object"] >= 0):
            ob = dw.order[int(own["object"][k])]
            assert orf.model_material(ob, own["local"][k], dw.materials) == int(hh["material"][k]), k
    assert orphans > 100
    # unused sample slots (-1) and rejected cast records (-2) are no hits
    from python_raytracer_amd import make_settings
    st4 = make_settings(width=48, height=36, samples=4, lod_edge=0.5, dist_max=192, chunk_lod=2)
    st4.culling = False
    cam4 = world_camera(st4, g["ps"], g["z"]["cam_pos"])
    frame4 = cam4.first_hit(all_samples=True)
    hh = frame4.numpy()
    assert (hh["material"] == -1).sum() > 100 and (hh["material"] > 0).sum() > 100
    res, own = both_stagings(g["dw"], frame4, cam4)
    check_no_hit_records(own, hh)
    check_stats(res.stats, own, hh, 0)
    assert not (own["object"] == -2).any()
    o, v, l = (np.array(a[:8]) for a in g["casts"])
    o[1, 0] = np.nan
    l[2] = 1e6
    cast = cam.cast_rays(o, v, l)
    hh = cast.numpy()
    assert (hh["material"][[1, 2]] == -2).all() and (hh["material"] > 0).any()
    res, own = both_stagings(g["dw"], cast, cam)
    check_no_hit_records(own, hh)
    assert (own["object"][[1, 2]] == -1).all()
    # a raw record tensor is taken as it is
    raw = g["dw"].owners(torch.clone(cast.records), cam)
    assert same(raw.numpy(), own)


# ---- 9. many objects -------------------------------------------------------------------------------------------------------
@gpu
def test_many_overlapping_objects():
    """300 small cubes in a box of 40^3: more than two LDS tiles of object records, owners at every depth of the list, waves
    whose lanes finish at different objects."""
    from python_raytracer_amd import make_settings
    cw = orf.crowd_world()
    objs, w = cw["objs"], cw["world"]
    assert len(objs) == 300 > 2 * 128
    dw = DeviceWorld(16)
    st = make_settings(width=32, height=24, samples=1, dist_max=96, chunk_lod=0)
    st.culling = False
    cam = world_camera(st, dw.build(objs), (20.0, 20.0, -30.0))
    sc = camera_scene(cam, dw, w)
    rng = np.random.default_rng(9)
    a, b = rng.uniform(-8, 48, (2000, 3)), rng.uniform(4, 36, (2000, 3))
    d = b - a
    ref = np.abs(d).max(1)
    hits = cam.cast_rays(a, d / ref[:, None], ref + 20)
    h = hits.numpy()
    res, own = both_stagings(dw, hits, cam)
    exp, ambiguous = orf.expect_owners(sc, w, objs, h)
    assert ambiguous == 0 and same(own, exp)
    ok = own["object"] >= 0
    assert ok.sum() > 1000 and len(set(own["object"][ok].tolist())) > 150
    assert own["object"][ok].min() < 20 and own["object"][ok].max() > 280     # owners near both ends of the list
    for k in np.flatnonzero(ok)[::7]:
        assert orf.model_material(objs[int(own["object"][k])], own["local"][k], dw.materials) == int(h["material"][k]), k
    check_no_hit_records(own, h)
    check_stats(res.stats, own, h, 0)


# ---- 10. object_image, counts, pick ----------------------------------------------------------------------------------------
@gpu
def test_object_image_counts_and_pick():
    g = golden()
    dw, cam, st = g["dw"], g["cam"], g["st"]
    frame = cam.first_hit(all_samples=True)
    res = dw.owners(frame, cam)
    own, h = res.numpy(), frame.numpy()
    img = res.object_image(frame).cpu().numpy()
    assert img.shape == (int(st.height), int(st.width)) and img.dtype == np.int32
    px = frame.pixels
    exp = np.full(img.shape, -1, np.int32)
    exp[px[:, 1], px[:, 0]] = own["object"][:: frame.samples]
    assert np.array_equal(img, exp) and (img >= 0).sum() > 50 and (img == -1).any()
    assert np.array_equal(img >= 0, frame.material_image().cpu().numpy() > 0)
    counts = res.counts()
    assert counts.shape == (len(dw.order),) and int(counts.sum()) == int(res.stats[nat.S_OWNER_RESOLVED])
    assert np.array_equal(counts, np.bincount(own["object"][own["object"] >= 0], minlength=len(dw.order)))
    # pick: the first sample of one pixel
    first = own["object"][:: frame.samples]
    k_hit, k_sky = int(np.flatnonzero(first >= 0)[0]), int(np.flatnonzero(h["material"][:: frame.samples] == 0)[0])
    x, y = (int(v) for v in px[k_hit])
    ob, local, voxel, depth = cam.pick(x, y, dw)
    assert ob is dw.order[int(first[k_hit])]
    assert local == tuple(own["local"][k_hit * frame.samples].tolist()) and voxel == tuple(own["voxel"][k_hit * frame.samples].tolist())
    assert depth == float(h["step"][k_hit * frame.samples]) == float(cam.first_hit(pixels=[[x, y]]).numpy()["step"][0])
    assert cam.pick(int(px[k_sky][0]), int(px[k_sky][1]), dw) is None


# ---- 11. capturable --------------------------------------------------------------------------------------------------------
@gpu
def test_owner_pass_is_graph_capturable():
    import torch
    g = golden()
    dw, cam = g["dw"], g["cam"]
    frame = cam.first_hit(all_samples=True)
    exp = dw.owners(frame, cam)
    exp_records, exp_stats = exp.numpy(), exp.stats.copy()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        dw.owners(frame, cam)                                 # (warm-up on the capturing side: the allocator)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        res = dw.owners(frame, cam)
    for _ in range(2):
        res.records.zero_()
        res._stats_dev.fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        assert same(res.numpy(), exp_records)
        assert np.array_equal(res._stats_dev.cpu().numpy(), exp_stats)


# ---- 12. fails loudly ------------------------------------------------------------------------------------------------------
@gpu
def test_owners_fail_loudly():
    import torch
    g = golden()
    dw, cam = g["dw"], g["cam"]
    frame = cam.first_hit()
    with pytest.raises(ValueError, match="are on cpu"):
        dw.owners(frame.records.cpu(), cam)
    with pytest.raises(ValueError, match="no whole number of 48-byte"):
        dw.owners(frame.records[:100], cam)
    with pytest.raises(ValueError, match="uint8"):
        dw.owners(frame.records.view(torch.int32), cam)
    with pytest.raises(RuntimeError, match="needs build"):
        DeviceWorld(16).owners(frame, cam)
    res = dw.owners(frame, cam)
    with pytest.raises(ValueError, match="not made from that HitResult"):
        res.object_image(cam.first_hit(all_samples=True))
