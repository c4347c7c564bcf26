"""Sprite edits on the device: vrt_edit_models / vrt_stamp_model against a sequential numpy replay, and DeviceWorld.update()
draining the sprites' journals -- against build_world() of the host sprites (the CPU truth) and, tick by tick, against the real
reference (tests/golden/world_edit.npz)."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

from python_raytracer_amd import Material, make_settings
from python_raytracer_amd import _native as nat
from python_raytracer_amd.lib import vec3, rgb, material, quaternion
from python_raytracer_amd.world import Sprite, Object, DeviceWorld, EDIT_JOURNAL_LIMIT
from test_edit_host import EditWorld, N_TICKS
from test_world import _device_grid, _merge_world

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64
SHAPES = [(2, 2, 2), (6, 4, 8), (12, 12, 12)]


def _mats(n):
    return [Material(function=material, albedo=rgb(20 * i, 255 - 20 * i, 40), roughness=0.2, absorption=1, ior=0, energy=0)
            for i in range(1, n + 1)]


def _models(rng):
    """Three models one after another (2^3, 6 x 4 x 8, 12^3), a third of their voxels filled: (offsets, flat bytes)."""
    offs, parts, off = [], [], 0
    for sh in SHAPES:
        n = int(np.prod(sh))
        offs.append(off)
        parts.append(np.where(rng.random(n) < 0.33, rng.integers(1, 256, n), 0).astype(np.uint8))
        off += n
    return offs, np.concatenate(parts)


def _record(model, shape, lo, hi, value, force):
    r = np.zeros((), nat.EDIT_FIELDS)
    r["model"], r["size"], r["lo"], r["hi"], r["value"], r["force"] = model, shape, lo, hi, value, force
    return r


def _valid(r, total):
    sh = [int(v) for v in r["size"]]
    return (min(sh) >= 1 and int(r["model"]) >= 0 and int(r["model"]) + sh[0] * sh[1] * sh[2] <= total
            and all(0 <= int(l) <= int(h) < s for l, h, s in zip(r["lo"], r["hi"], sh)) and 0 <= int(r["value"]) <= 255)


def _replay(flat, records):
    """The records applied one after another (include/vrt.h); invalid ones are skipped.  Returns (bytes, invalid count)."""
    out, bad = flat.copy(), 0
    for r in records:
        if not _valid(r, len(flat)):
            bad += 1
            continue
        sh = tuple(int(v) for v in r["size"])
        m = out[int(r["model"]):int(r["model"]) + int(np.prod(sh))].reshape(sh)
        box = m[tuple(slice(int(l), int(h) + 1) for l, h in zip(r["lo"], r["hi"]))]
        if int(r["force"]):
            box[...] = int(r["value"])
        else:
            box[box == 0] = int(r["value"])
    return out, bad


def _run_edits(flat, records):
    """vrt_edit_models over `flat` with guard bytes on both sides: (bytes after, statistics, guards intact)."""
    import torch
    buf = torch.full((GUARD + len(flat) + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    buf[GUARD:GUARD + len(flat)] = torch.from_numpy(flat).cuda()
    arr = np.array(records, nat.EDIT_FIELDS) if len(records) else np.zeros(0, nat.EDIT_FIELDS)
    d_edits = torch.from_numpy(arr.view(np.uint8).reshape(-1).copy()).cuda() if len(records) else None
    stats = torch.full((nat.NSTATS,), 7, dtype=torch.int64, device="cuda")      # (the library clears it)
    rc = nat.lib().vrt_edit_models(buf.data_ptr() + GUARD, len(flat), d_edits.data_ptr() if len(records) else None, len(records),
                                   stats.data_ptr(), torch.cuda.current_stream().cuda_stream)
    nat.check(rc, "vrt_edit_models")
    torch.cuda.synchronize()
    out = buf.cpu().numpy()
    return out[GUARD:-GUARD], stats.cpu().numpy(), bool((out[:GUARD] == 0xA5).all() and (out[-GUARD:] == 0xA5).all())


def _random_records(rng, offs, n):
    recs = []
    for _ in range(n):
        k = int(rng.integers(0, 3))
        sh = SHAPES[k]
        kind = rng.random()
        if kind < 0.4:                                          # a point
            lo = hi = [int(rng.integers(0, s)) for s in sh]
        elif kind < 0.9:                                        # a box
            a, b = [int(rng.integers(0, s)) for s in sh], [int(rng.integers(0, s)) for s in sh]
            lo, hi = [min(p, q) for p, q in zip(a, b)], [max(p, q) for p, q in zip(a, b)]
        else:                                                   # the whole model
            lo, hi = [0, 0, 0], [s - 1 for s in sh]
        value = 0 if rng.random() < 0.3 else int(rng.integers(1, 256))
        recs.append(_record(offs[k], sh, lo, hi, value, int(rng.random() < 0.5)))
    return recs


# ---- 1. replay -------------------------------------------------------------------------------------------------------------
@gpu
def test_one_call_replays_200_overlapping_records_in_order():
    rng = np.random.default_rng(31)
    offs, flat = _models(rng)
    recs = _random_records(rng, offs, 200)
    assert {int(r["force"]) for r in recs} == {0, 1} and any(int(r["value"]) == 0 for r in recs)
    exp, bad = _replay(flat, recs)
    got, stats, guards = _run_edits(flat, recs)
    assert bad == 0 and not stats.any() and guards
    assert np.array_equal(got, exp) and not np.array_equal(exp, flat)
    # the order matters: the same records backwards give other bytes
    assert not np.array_equal(_replay(flat, recs[::-1])[0], exp)
    got, stats, guards = _run_edits(flat, [])
    assert np.array_equal(got, flat) and not stats.any() and guards


# ---- 2. invalid records ----------------------------------------------------------------------------------------------------
@gpu
def test_invalid_records_are_skipped_whole_and_counted():
    rng = np.random.default_rng(32)
    offs, flat = _models(rng)
    total = len(flat)
    good = _random_records(rng, offs, 40)
    bad = [_record(offs[1], SHAPES[1], [0, 0, 0], [6, 3, 7], 9, 1),              # a box outside size
           _record(offs[2], SHAPES[2], [0, 0, 12], [3, 3, 12], 9, 1),
           _record(offs[1], SHAPES[1], [2, 3, 1], [1, 3, 5], 9, 1),              # lo > hi
           _record(total - 4, SHAPES[0], [0, 0, 0], [1, 1, 1], 9, 1),            # a model that runs past models_bytes
           _record(offs[2], (12, 12, 13), [0, 0, 0], [11, 11, 12], 9, 1),
           _record(-8, SHAPES[0], [0, 0, 0], [1, 1, 1], 9, 1),
           _record(offs[2], SHAPES[2], [1, 1, 1], [4, 4, 4], 256, 1),            # value 256
           _record(offs[0], SHAPES[0], [0, 0, 0], [0, 0, 0], -1, 1)]
    # an invalid record first of all (it must not lead its model), the others spread among the valid ones
    recs = [bad[0]] + good[:]
    for k, r in enumerate(bad[1:]):
        recs.insert(3 + 5 * k, r)
    exp, n_bad = _replay(flat, recs)
    assert n_bad == len(bad) and np.array_equal(exp, _replay(flat, good)[0])
    got, stats, guards = _run_edits(flat, recs)
    assert guards
    assert np.array_equal(got, exp)
    assert int(stats[nat.S_EDIT_INVALID]) == len(bad) and not np.delete(stats, nat.S_EDIT_INVALID).any()
    # only invalid records: nothing changes
    got, stats, guards = _run_edits(flat, bad)
    assert np.array_equal(got, flat) and int(stats[nat.S_EDIT_INVALID]) == len(bad) and guards


# ---- 3. stamp --------------------------------------------------------------------------------------------------------------
@gpu
def test_stamp_model_mixes_through_the_id_map():
    import torch
    rng = np.random.default_rng(33)
    sh = (6, 4, 8)
    n = int(np.prod(sh))
    dst = np.where(rng.random(n) < 0.5, rng.integers(1, 256, n), 0).astype(np.uint8)
    src = np.where(rng.random(n) < 0.5, rng.integers(1, 256, n), 0).astype(np.uint8)
    idmap = np.concatenate([[0], rng.permutation(np.arange(1, 256))]).astype(np.uint8)
    assert (idmap[1:] != np.arange(1, 256)).any()
    flat = np.concatenate([dst, np.full(5, 0xA5, np.uint8), src])             # (the models need no alignment)
    d_map = torch.from_numpy(idmap).cuda()
    size = (C.c_int32 * 3)(*sh)
    stream = torch.cuda.current_stream().cuda_stream
    for force in (1, 0):
        buf = torch.from_numpy(np.concatenate([np.full(GUARD, 0xA5, np.uint8), flat, np.full(GUARD, 0xA5, np.uint8)])).cuda()
        nat.check(nat.lib().vrt_stamp_model(buf.data_ptr() + GUARD, len(flat), 0, n + 5, size, d_map.data_ptr(), force, stream),
                  "vrt_stamp_model")
        out = buf.cpu().numpy()
        exp = np.where((src != 0) & ((dst == 0) | bool(force)), idmap[src], dst)
        assert np.array_equal(out[GUARD:GUARD + n], exp) and not np.array_equal(exp, dst)
        assert np.array_equal(out[GUARD + n:-GUARD], flat[n:]) and (out[:GUARD] == 0xA5).all() and (out[-GUARD:] == 0xA5).all()
    base = buf.data_ptr() + GUARD
    for d, s in ((0, 0), (0, n - 1), (n - 1, 0), (10, 0)):                     # overlapping ranges
        assert nat.lib().vrt_stamp_model(base, len(flat), d, s, size, d_map.data_ptr(), 1, stream) == -1
    assert nat.lib().vrt_stamp_model(base, len(flat), 0, n + 6, size, d_map.data_ptr(), 1, stream) == -1   # src leaves the buffer
    assert nat.lib().vrt_stamp_model(base, len(flat), 0, n, size, d_map.data_ptr(), 1, stream) == 0        # adjacent: allowed
    torch.cuda.synchronize()


# ---- worlds for 4, 6, 7, 8 -------------------------------------------------------------------------------------------------
def _filled_sprite(rng, size, mats, fill):
    spr = Sprite(size=vec3(*size), frames=1, lod=0)
    vox = {p: mats[int(rng.integers(len(mats)))] for p in itertools.product(*[range(s) for s in size]) if rng.random() < fill}
    spr.get_frame(0).set_voxels(vox, True)
    return spr


def _visible(pos, rot, spr):
    ob = Object(pos=vec3(*pos), rot=vec3(*rot), sprite=spr)
    ob.visible = True
    return ob


def _update_with_sentinels(dw, objs):
    """dw.update(objs) with every voxel byte replaced by a sentinel first: (scene, count returned, chunks the update wrote).
    The chunks it did not write get their bytes back, so the world can be compared afterwards."""
    cs = dw.chunk_size
    good = dw._voxels.clone()
    dw._voxels.fill_(0xEE)
    ps, rebuilt = dw.update(objs)
    written = (dw._voxels.view(-1, cs ** 3) != 0xEE).any(1)      # (a rebuilt chunk holds ids <= 255 materials and zeros)
    dw._voxels.view(-1, cs ** 3)[~written] = good.view(-1, cs ** 3)[~written]
    return ps, rebuilt, int(written.sum().item())


def _assert_world_is_host_build(dw, ps):
    table, grid = _device_grid(dw, ps)
    g, p = _merge_world(dw, dw.chunk_size)
    assert np.array_equal(grid, g) and np.array_equal((table != 0).astype(np.uint8), p)


TURNS = [(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (2, 3, 0), (1, 1, 1), (3, 0, 2), (0, 2, 3)]


# ---- 4. semantics (b): an edit without redraw ------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("turns", TURNS, ids=["%d%d%d" % t for t in TURNS])
def test_one_voxel_edit_rebuilds_one_chunk_and_writes_no_other(turns):
    rng = np.random.default_rng(40 + sum(turns))
    mats = _mats(5)
    cube = _filled_sprite(rng, (16, 16, 16), mats, 0.5)
    flat = _filled_sprite(rng, (16, 8, 16), mats, 0.5)           # only its y turn applies (data.py:344-371)
    rot = [90 * t for t in turns]
    objs = [_visible((8, 8, 8), rot, cube), _visible((14, 10, 6), rot, flat)]   # the second overlaps the first
    dw = DeviceWorld(8)
    ps = dw.build(objs)
    assert int(np.prod(dw.dims)) >= 12
    _assert_world_is_host_build(dw, ps)
    order = dw.order
    for spr, pos, mat, force in ((cube, (5, 9, 2), None, True), (flat, (15, 0, 8), mats[4], True), (cube, (8, 7, 15), mats[0], False)):
        before = spr.dense()[0][pos]
        spr.set_voxel(None, vec3(*pos), mat, force)
        ps, rebuilt, written = _update_with_sentinels(dw, objs)
        assert rebuilt == 1 and written == 1, (pos, rebuilt, written)
        assert dw.order == order
        _assert_world_is_host_build(dw, ps)
        ids, smats = dw.model(spr)
        host, hmats = spr.dense()
        assert np.array_equal(ids != 0, host != 0)
        assert [smats[i - 1] for i in ids[ids != 0]] == [hmats[i - 1] for i in host[host != 0]]
        assert (spr.dense()[0][pos] != 0) == ((mat is not None) if (force or not before) else bool(before))
    assert dw.edit_calls == {"edit": 3, "stamp": 0, "resync": 0}
    # nothing pending: nothing rebuilt
    assert dw.update(objs)[1] == 0


# ---- 5. semantics (a): the reference's flow ---------------------------------------------------------------------------------
@gpu
def test_device_reproduces_every_tick_of_the_reference():
    w = EditWorld()
    cube = w.sprites["cube"]
    w.run(0)
    dw = DeviceWorld(w.cs)
    dw.hold(w.sprites["src"])                    # (no object shows src: held, so that the mixes run on the device)
    ps = dw.build(w.objs)
    for k in range(N_TICKS):
        if k:
            w.run(k)
            w.objs[0].redraw = w.objs[1].redraw = True
            ps, rebuilt = dw.update(w.objs)
            assert rebuilt > 0
        _, grid = _device_grid(dw, ps)
        assert w.same_world(dw.origin, w.fixture_ids(grid, dw.materials), k), k
        # (an object without voxels has no entry in the reference's dict; here it keeps its place and contributes nothing)
        shown = [w.objs.index(o) for o in dw.order if o.sprite.dense()[0].any()]
        assert shown == w.z["order_%d" % k].tolist(), k
        ids, smats = dw.model(cube)
        assert np.array_equal(w.fixture_ids(ids, smats), w.z["model_%d" % k]), k
    # ticks 1, 2 and 5 are one vrt_edit_models call each; the mixes of ticks 3 and 4 one vrt_stamp_model each
    assert dw.edit_calls == {"edit": 3, "stamp": 2, "resync": 0}


# ---- 6. a shared sprite ----------------------------------------------------------------------------------------------------
@gpu
def test_one_edit_shows_in_every_object_of_a_shared_sprite():
    rng = np.random.default_rng(6)
    mats = _mats(4)
    spr = _filled_sprite(rng, (16, 16, 16), mats, 0.5)
    objs = [_visible((8, 8, 8), (0, 0, 0), spr), _visible((40, 8, 8), (0, 90, 180), spr)]
    dw = DeviceWorld(8)
    ps = dw.build(objs)
    _, g0 = _device_grid(dw, ps)
    spr.set_voxels_area(None, vec3(1, 2, 3), vec3(1, 2, 3), mats[2] if not spr.dense()[0][1, 2, 3] else None, True)
    ps, rebuilt, written = _update_with_sentinels(dw, objs)
    assert rebuilt == 2 and written == 2
    _assert_world_is_host_build(dw, ps)
    _, g1 = _device_grid(dw, ps)
    where = np.argwhere(g0 != g1) + np.asarray(dw.origin)
    assert len(where) == 2 and sorted((where[:, 0] >= 32).tolist()) == [False, True]     # one voxel in each object's box
    # an edit that straddles a chunk border of one image: the chunk count is the union over both objects
    spr.set_voxels_area(None, vec3(7, 0, 0), vec3(8, 0, 0), mats[1], True)
    ps, rebuilt, written = _update_with_sentinels(dw, objs)
    assert rebuilt == written == 4
    _assert_world_is_host_build(dw, ps)


# ---- 7, 8. the loop: pick, edit, update, render ----------------------------------------------------------------------------
def _camera(st, ps, pos):
    from python_raytracer_amd import Camera
    cam = Camera(settings=st)
    cam.pos = vec3(*[float(v) for v in pos])
    cam.rot = quaternion(0.0, 0.0, 0.0, 1.0)
    cam.set_world_scene(ps)
    cam.chunk_update(None)
    return cam


def _loop_world():
    rng = np.random.default_rng(7)
    mats = _mats(4)
    spr = _filled_sprite(rng, (16, 16, 16), mats, 0.7)
    objs = [_visible((8, 8, 8), (0, 90, 0), spr), _visible((18, 10, 10), (0, 0, 0), _filled_sprite(rng, (8, 8, 8), mats, 0.7))]
    st = make_settings(width=32, height=24, samples=1, chunk_size=8, dist_max=96, chunk_lod=0)
    st.culling = False
    dw = DeviceWorld(8)
    ps = dw.build(objs)
    return mats, objs, st, dw, ps, (8.0, 8.0, -24.0)


def _render_equals_fresh_build(dw, cam, st, pos):
    import torch
    fresh = DeviceWorld(dw.chunk_size)
    other = _camera(st, fresh.build(list(dw.order)), pos)
    a, b = cam.render(0), other.render(0)
    assert torch.equal(a.rgba_f32, b.rgba_f32) and float(a.rgba_f32.abs().sum()) > 0
    return a


@gpu
def test_pick_edit_update_render_loop():
    mats, objs, st, dw, ps, pos = _loop_world()
    cam = _camera(st, ps, pos)
    x, y = 16, 12
    ob, local, voxel, depth = cam.pick(x, y, dw)
    first = cam.first_hit(pixels=[[x, y]]).numpy()[0]
    assert ob.sprite.dense()[0][local] != 0
    ob.sprite.set_voxel(None, vec3(*local), None, True)          # dig the voxel under the cursor
    ps, rebuilt = dw.update(objs)
    assert rebuilt == 1
    cam.set_world_scene(ps)
    cam.chunk_update(None)
    hit = cam.first_hit(pixels=[[x, y]])
    now = hit.numpy()[0]
    assert tuple(now["cell"].tolist()) != tuple(first["cell"].tolist()) and float(now["step"]) > float(first["step"])
    own = dw.owners(hit, cam)                                    # no build() in between: the object records are still good
    rec = own.numpy()[0]
    assert int(own.stats[nat.S_OWNER_ORPHANS]) == 0
    if int(now["material"]) > 0:
        o2 = dw.order[int(rec["object"])]
        assert o2.sprite.dense()[0][tuple(rec["local"].tolist())] != 0
        assert (o2, tuple(rec["local"].tolist())) != (ob, tuple(local))
    _render_equals_fresh_build(dw, cam, st, pos)
    _assert_world_is_host_build(dw, ps)


@gpu
def test_a_material_the_world_has_never_seen():
    mats, objs, st, dw, ps, pos = _loop_world()
    cam = _camera(st, ps, pos)
    rows = ps.materials.shape[0]
    ob, local, voxel, depth = cam.pick(16, 12, dw)
    glow = Material(function=material, albedo=rgb(255, 255, 0), roughness=0.0, absorption=1, ior=0, energy=3.0)
    ob.sprite.set_voxel(None, vec3(*local), glow, True)
    before = cam.render(0).rgba_f32.clone()
    ps, rebuilt = dw.update(objs)
    assert rebuilt == 1 and ps.materials.shape[0] == rows + 1 and dw.materials[-1] is glow
    assert len(dw.materials) == rows + 1
    cam.set_world_scene(ps)
    cam.chunk_update(None)
    after = _render_equals_fresh_build(dw, cam, st, pos)
    assert not np.array_equal(before.cpu().numpy(), after.rgba_f32.cpu().numpy())
    assert dw.model(ob.sprite)[1][-1] is glow
    # a 256th material of one model is refused before anything changes
    spr = ob.sprite
    for m in _mats(255 - len(dw.model(spr)[1])):
        spr.set_voxel(None, vec3(0, 0, 0), m, True)
    ids = dw.model(spr)[0]
    spr.set_voxel(None, vec3(0, 0, 1), Material(function=material, albedo=rgb(1, 2, 3), roughness=0, absorption=1, ior=0, energy=0), True)
    with pytest.raises(ValueError):
        dw.update(objs)
    assert np.array_equal(dw.model(spr)[0], ids)


# ---- 9. resync -------------------------------------------------------------------------------------------------------------
@gpu
def test_long_journals_and_lod_sprites_are_copied_anew():
    rng = np.random.default_rng(9)
    mats = _mats(6)
    spr = _filled_sprite(rng, (8, 8, 8), mats, 0.4)
    lod = Sprite(size=vec3(8, 8, 8), frames=1, lod=1)
    lod.get_frame(0).set_voxels({(2 * x, 2 * y, 2 * z): mats[(x + y + z) % 6] for x in range(4) for y in range(4) for z in range(3)}, True)
    objs = [_visible((4, 4, 4), (90, 0, 0), spr), _visible((20, 4, 4), (0, 180, 0), lod), _visible((36, 4, 4), (0, 0, 90), spr)]
    dw = DeviceWorld(8)
    ps = dw.build(objs)
    for p in rng.integers(0, 8, (EDIT_JOURNAL_LIMIT + 1, 3)):
        spr.set_voxel(None, vec3(*[int(v) for v in p]), mats[int(rng.integers(6))] if rng.random() < 0.6 else None, rng.random() < 0.5)
    ps, rebuilt = dw.update(objs)
    assert rebuilt == 2 and dw.edit_calls == {"edit": 0, "stamp": 0, "resync": 1}
    _assert_world_is_host_build(dw, ps)
    # one record fewer is replayed
    for p in rng.integers(0, 8, (EDIT_JOURNAL_LIMIT, 3)):
        spr.set_voxel(None, vec3(*[int(v) for v in p]), mats[int(rng.integers(6))] if rng.random() < 0.6 else None, rng.random() < 0.5)
    ps, rebuilt = dw.update(objs)
    assert dw.edit_calls == {"edit": 1, "stamp": 0, "resync": 1}
    _assert_world_is_host_build(dw, ps)
    lod.set_voxels_area(None, vec3(0, 0, 6), vec3(7, 7, 7), mats[0], True)
    lod.set_voxel(None, vec3(2, 2, 2), None, True)
    ps, rebuilt = dw.update(objs)
    assert rebuilt == 1 and dw.edit_calls == {"edit": 1, "stamp": 0, "resync": 2}
    _assert_world_is_host_build(dw, ps)
    # a Frame replaced wholesale
    spr.get_frame(0).clear()
    path = os.path.join(ROOT, "tests", "golden", "assets", "odd.txt")
    spr.load([path], {"ff0000": mats[0], "00ff00": mats[1], "0000ff": mats[2], "7f7f7f": mats[3]})
    assert spr.dense()[0].any()
    ps, rebuilt = dw.update(objs)
    assert rebuilt == 2 and dw.edit_calls["resync"] == 3
    _assert_world_is_host_build(dw, ps)


# ---- 10. kernel resources --------------------------------------------------------------------------------------------------
@gpu
def test_edit_kernels_use_no_scratch_and_spill_nothing():
    """The compiler's own report for gfx950 (-Rpass-analysis=kernel-resource-usage), saved in
    profiles/kernel_resource_usage.txt and compared with a fresh compilation by tests/test_kernel_resources.py."""
    import kernel_report
    rep = {k: v for k, v in kernel_report.saved().items() if "edit_models_kernel" in k or "stamp_model_kernel" in k}
    assert sorted(re.sub(r"^_Z\d+", "", k)[:12] for k in rep) == ["edit_models_", "stamp_model_"]
    for name, r in rep.items():
        assert r["ScratchSize [bytes/lane]"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, (name, r)
        assert r["AGPRs"] == 0 and r["LDS Size [bytes/block]"] == 0 and r["Occupancy [waves/SIMD]"] == 8, (name, r)


# ---- 11. the kept scene under the occupancy lookups ------------------------------------------------------------------------
def lookup_leg():
    """(a child process of the test below, VRT_LOOKUP set: the variable is read once per process)  The first nine ticks of
    script B (tests/sequences.py: moves, turns, a hide and edits with and without redraw, all incremental) on one DeviceWorld
    whose scene one Camera was given once.  After every update the scene is still that object, its occupancy words are those
    of the voxels as they are now -- bit b of word w: voxel byte 64 w + b holds a material -- and the frame of the camera
    that still holds it is the oracle's over the host build."""
    import oracle_lib as ol
    import sequences as sq
    from gpu_util import frame_equals_oracle, settings_store
    from python_raytracer_amd import Camera
    from python_raytracer_amd.scene import material_row
    S = sq.ScriptB()
    cs = S.cs
    st = ol.make_settings(**sq.SETTINGS_B)
    dw = DeviceWorld(cs)
    cam = Camera(settings=settings_store(st))
    cam.rot, cam.lens = quaternion(*sq.CAM_ROT_B), st["fov"] * np.pi / 8
    held, changed = None, 0
    for k in range(9):
        exp = S.run(k)
        ps, rebuilt = dw.update(S.objs)
        S.done()
        assert rebuilt == exp["chunks"] and bool(exp["full"]) == (k == 0)
        if k == 0:
            cam.set_world_scene(ps)
            held, before = ps, None
        assert ps is held
        vox = dw._voxels.cpu().numpy()
        want = np.packbits(vox.reshape(-1, 64) != 0, axis=1, bitorder="little").view(np.uint64).reshape(-1)
        occ = ps.device_tensors["occupancy"].cpu().numpy().view(np.uint64)
        assert np.array_equal(occ[:len(want)], want), k
        changed += before is not None and not np.array_equal(before, want)
        before = want
        cam.pos = vec3(*sq.cam_pos_b(k))
        grid, present = _merge_world(dw, cs)
        rows = np.array([material_row(m)[:7] for m in dw.materials], np.float64).reshape(-1, 7)
        scene = ol.Scene(dw.origin, dw.dims, cs, present, np.ones_like(present), grid, rows)
        frame_equals_oracle(cam.render(0, want_ray_rgba=True), sq.render_b(k, scene), cs)
    assert changed >= 6                                   # (the words really had to change under the camera)
    print("LOOKUP_LEG ok", os.environ["VRT_LOOKUP"])


@gpu
def test_incremental_updates_refresh_the_occupancy_words_of_the_kept_scene():
    """DeviceWorld.update keeps its scene object across incremental updates; with VRT_LOOKUP=1|2 the march reads the scene's
    occupancy words in place of the voxel bytes, so they have to follow every update (lookup_leg, one child per variant)."""
    from gpu_util import run_children
    lines = run_children("import test_gpu_edit as t; t.lookup_leg()", [{"VRT_LOOKUP": "1"}, {"VRT_LOOKUP": "2"}], "LOOKUP_LEG")
    assert [l[1:] for l in lines] == [["ok", "1"], ["ok", "2"]]
