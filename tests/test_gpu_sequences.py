"""One long-lived Camera and one long-lived DeviceWorld while things change underneath them: the scripts of tests/sequences.py on
the GPU.  Every step is compared bit for bit with a from-scratch answer -- the oracle's frame (oracle_lib.render, select_chunks)
or the host world (build_world over the merge order) -- and with a fresh object given the same state; which cached objects a
step rebuilds, the merge order and the number of chunks an update writes are the scripts' own.  tests/test_sequences_host.py
proves on the CPU that the scripts reach what their steps are named for.  The shipped kernel choice: no VRT_* variable is set.
(The memo leg creates 64 pow tables: it stays last in the module.)"""
import numpy as np
import pytest

import cast_ref as cr
import oracle_lib as ol
import owner_ref as orf
import sequences as sq
from gpu_util import camera_for, frame_equals_oracle, launches_of, settings_store
from python_raytracer_amd import data
from python_raytracer_amd.data import Frame, finalize_settings
from python_raytracer_amd.lib import material, material_background, quaternion, rgb, vec3
from python_raytracer_amd.scene import material_row
from python_raytracer_amd.world import DeviceWorld, World, build_world
from test_gpu_owners import check_no_hit_records, check_stats
from test_world import _assert_same_world, _merge_world

gpu = pytest.mark.gpu
CS_A = 16


def oracle_of(sc, shot, pixels, st=None):
    return ol.render(sc, st or shot.st, shot.pos, shot.rot, shot.lens, pixels, libm=ol.LIBM_PORTABLE, seed_nonce=shot.nonce,
                     has_background=shot.background)


def same_frames(a, b, cs):
    import torch
    assert torch.equal(a.rgba_f32, b.rgba_f32) and torch.equal(a.image_u8, b.image_u8) and torch.equal(a.ray_rgba, b.ray_rgba)
    assert (a.stats[:15] == b.stats[:15]).all(), (a.stats, b.stats)
    assert a.traversed(cs) == b.traversed(cs)


def cached(cam, thread):
    """(DevicePixels, plan, draw table, ray table, draws per seed of the draw table) the camera holds for a thread now."""
    entry = cam._pixel_cache.get(thread)
    if entry is None:
        return None, None, None, None, None
    dp = entry[1]
    return dp, dp.plan, dp.draw_table, dp.ray_table, dp.draw_key[1] if dp.draw_key is not None else None


def rebuilt_between(before, after):
    names = set()
    if after[0] is not before[0]:
        names.add("pixels")
    for k, name in ((1, "plan"), (2, "draw"), (3, "ray")):
        if after[k] is not before[k]:
            names.add(name)
    return names


def apply_shot(cam, store, shot):
    """Change exactly what the shot names on the live camera and store."""
    for k, v in shot.changes.items():
        setattr(store, k, v)
    for w, h, t in shot.windows:
        store.width, store.height, store.threads = w, h, t
        finalize_settings(store)
    if shot.moved:
        cam.pos, cam.rot = vec3(*shot.pos), quaternion(*shot.rot)
    if shot.lens_scale is not None:
        cam.lens = cam.lens * shot.lens_scale
    cam.cache_draws = shot.cache_draws
    # the live state is the state the script declares for the shot
    assert float(cam.lens) == shot.lens and (cam.pos.x, cam.pos.y, cam.pos.z) == shot.pos
    for k, v in shot.st.items():
        assert getattr(store, k) == v, (shot, k)


def families(cam, shot):
    poses = [(tuple(p + d for p, d in zip(shot.pos, off)), shot.rot) for off in sq.VIEW_OFFSETS]
    hit = cam.first_hit(shot.thread, all_samples=True)
    rays, used = cam.pixel_rays(shot.thread)
    views = cam.render_views(poses, shot.thread, want_ray_rgba=True)
    return hit, rays, used, views


# ---- A. one camera, one settings store, a walk through the settings ------------------------------------------------------------
@gpu
def test_walk_a_one_camera_through_every_setting():
    """Steps 0 to 17 of walk A on one Camera and one settings store.  After every shot: the frame is the oracle's of the shot's
    settings, from scratch; it equals, with its image, per-sample colours, statistics and traversed list, the frame of a fresh
    camera given the same settings; and the camera rebuilt exactly the cached objects the script declares for the shot."""
    import torch
    sc = ol.default_scene()
    shots = sq.walk_a()
    store = settings_store(shots[0].st)
    cam = camera_for(sc, store, shots[0].pos, shots[0].rot, shots[0].lens)
    ran = {}
    try:
        for n, shot in enumerate(shots):
            apply_shot(cam, store, shot)
            data.background = material_background if shot.background else None
            before = cached(cam, shot.thread)
            draws = cam.fast_draws
            if shot.kind == "families":
                got = families(cam, shot)
            r, ran[n] = launches_of(lambda: cam.render(shot.thread, want_ray_rgba=True, seed_nonce=shot.nonce or None))
            after = cached(cam, shot.thread)
            # which cached objects were rebuilt: what the step invalidates and nothing more (a draw table widened to 64
            # draws per seed by render() itself is a rebuild of both tables)
            expect = set(shot.rebuilt)
            if before[4] is not None and after[4] is not None and before[4] != after[4] and before[0] is after[0]:
                expect |= {"draw", "ray"}
            assert rebuilt_between(before, after) == expect, (shot, rebuilt_between(before, after), expect)
            # the oracle's frame of the step's settings, from scratch
            assert np.array_equal(r.pixels, shot.pixels)
            o = oracle_of(sc, shot, r.pixels)
            frame_equals_oracle(r, o, CS_A)
            # a fresh camera given the same settings
            fresh = camera_for(sc, settings_store(shot.st), shot.pos, shot.rot, shot.lens)
            fresh.cache_draws, fresh.fast_draws = shot.cache_draws, draws
            if shot.kind == "families":
                want = families(fresh, shot)
                assert torch.equal(got[0].records, want[0].records)
                assert torch.equal(got[1].view(torch.int64), want[1].view(torch.int64)) and torch.equal(got[2], want[2])
                assert bool(got[2].all()) and len(got[3]) == len(want[3]) == len(sq.VIEW_OFFSETS)
                for v, (a, b) in enumerate(zip(got[3], want[3])):
                    assert torch.equal(a.rgba_f32, b.rgba_f32) and torch.equal(a.image_u8, b.image_u8)
                    assert torch.equal(a.ray_rgba, b.ray_rgba) and a.traversed(CS_A) == b.traversed(CS_A)
                    pose = sq.Shot(17, "view", shot.st, tuple(p + d for p, d in zip(shot.pos, sq.VIEW_OFFSETS[v])), shot.rot,
                                   shot.lens, shot.thread, {}, (), ())
                    assert np.array_equal(a.rgba_f32.cpu().numpy(), oracle_of(sc, pose, r.pixels)["pix_mean"].astype(np.float32))
            same_frames(r, fresh.render(shot.thread, want_ray_rgba=True, seed_nonce=shot.nonce or None), CS_A)
    finally:
        data.background = material_background
    # step 3 runs another march instance (one ray record per pixel), step 4 the first one again
    k3 = [n for n, s in enumerate(shots) if s.step == 3][0]
    assert ran[k3] - ran[k3 - 1] and ran[k3 - 1] - ran[k3], (ran[k3 - 1], ran[k3])
    assert ran[k3 - 1] - ran[k3] <= ran[k3 + 1] and not (ran[k3] - ran[k3 - 1]) & ran[k3 + 1], (ran[k3 - 1], ran[k3], ran[k3 + 1])
    # one workspace, grown and never shrunk; the per-thread pixel lists of step 10 are all held
    assert len(cam._workspace) == 1 and sorted(cam._pixel_cache) == [0, 1, 2, 3]


@gpu
def test_step_18_a_camera_built_from_chunks_repacks_its_scene():
    """chunk_set of one more Frame, and invalidate() after a Material changed in place: the packed scene is a snapshot that the
    camera makes anew, and every frame is the oracle's over the chunks as they are then."""
    from python_raytracer_amd import Camera, Material
    rng = np.random.default_rng(18)
    st = ol.make_settings(width=24, height=18, samples=2, max_bounces=2.0, dist_max=64)
    mats = [Material(function=material, albedo=rgb(200 - 60 * i, 40 + 70 * i, 90), roughness=0.1 * i, absorption=0.5 + 0.25 * i,
                     ior=0.0, energy=0.0) for i in range(3)]
    grids = [np.where(rng.random((16, 16, 16)) < 0.2, rng.integers(1, 4, (16, 16, 16)), 0).astype(np.uint8) for _ in range(2)]
    posts = [(0, 0, 0), (16, 0, 0)]

    def frame_of(post, grid):
        fr = Frame(resolution=1)
        fr.set_voxels({tuple(int(v) + p for v, p in zip(c, post)): mats[int(grid[tuple(c)]) - 1] for c in np.argwhere(grid)}, True)
        return fr

    def oracle(n):
        grid = np.concatenate(grids[:n], 0)
        rows = np.array([material_row(m)[:7] for m in mats], np.float64)
        dims = [n, 1, 1]
        sc = ol.Scene([0, 0, 0], dims, 16, np.ones(dims, np.uint8), np.ones(dims, np.uint8), grid, rows)
        return ol.render(sc, st, pos, rot, lens, ol.pixel_lists(24, 18, 1)[0], libm=ol.LIBM_PORTABLE)

    pos, rot, lens = (14.5, 7.25, -22.0), (0.0, 0.0, 0.0, 1.0), st["fov"] * np.pi / 8
    cam = Camera(settings=settings_store(st))
    cam.pos, cam.rot, cam.lens = vec3(*pos), quaternion(*rot), lens
    cam.chunks = {posts[0]: frame_of(posts[0], grids[0])}
    frames = []
    for change in ("first", "chunk_set", "material"):
        if change == "chunk_set":
            cam.chunk_set(posts[1], frame_of(posts[1], grids[1]))
        if change == "material":
            mats[0].albedo = rgb(15, 240, 200)
            mats[1].absorption = 2.0
            r = cam.render(0, want_ray_rgba=True)            # not invalidated yet: the snapshot still renders
            frame_equals_oracle(r, frames[-1][1], 16)
            assert cam._scene is frames[-1][2]
            cam.invalidate()
        for again in range(2):                               # rendered before and after: the second frame repacks nothing
            r = cam.render(0, want_ray_rgba=True)
            o = oracle(1 if change == "first" else 2)
            frame_equals_oracle(r, o, 16)
            assert again == 0 or cam._scene is packed
            packed = cam._scene
        assert not frames or packed is not frames[-1][2]     # the scene was packed anew
        assert not frames or not np.array_equal(o["pix_mean"], frames[-1][1]["pix_mean"])
        frames.append((r, o, packed))
    assert (frames[-1][1]["rays"]["counters"][:, ol.COUNTERS.index("hit")] > 0).mean() > 0.3


@gpu
def test_two_streams_while_the_tables_are_rebuilt():
    """A frame on a side stream while the lens (step 2: a new ray table) and the sample count (step 5: a new plan and both
    tables) change on the current stream: the side frames were launched with the old tables, which must outlive them."""
    import torch
    sc = ol.default_scene()
    shots = sq.walk_a()
    base = shots[0]
    store = settings_store(base.st)
    cam = camera_for(sc, store, base.pos, base.rot, base.lens)
    cam.render(0)                                            # the tables exist, built on the current stream
    side = torch.cuda.Stream()
    states, got = [], []

    def launch(stream):
        states.append(sq.Shot(0, "two streams", dict(base.st, samples=int(store.samples)), base.pos, base.rot, float(cam.lens),
                              0, {}, (), ()))
        if stream is None:
            got.append(cam.render(0, want_ray_rgba=True))
        else:
            with torch.cuda.stream(stream):
                got.append(cam.render(0, want_ray_rgba=True, check=False))

    launch(side)
    ray0 = cached(cam, 0)[3]
    cam.lens = cam.lens * 0.8
    launch(None)
    assert cached(cam, 0)[3] is not ray0
    launch(side)
    plan0 = cached(cam, 0)[1]
    store.samples = 5
    launch(None)
    assert cached(cam, 0)[1] is not plan0
    launch(side)
    torch.cuda.synchronize()
    assert len(cam._workspace) == 2
    for shot, r in zip(states, got):
        if r.stats is None:
            r.stats = r._stats_dev.cpu().numpy()
        frame_equals_oracle(r, oracle_of(sc, shot, r.pixels), CS_A)
    assert [s.st["samples"] for s in states] == [2, 2, 2, 5, 5] and len({s.lens for s in states}) == 2


# ---- B. one DeviceWorld, one Camera, 40 scripted ticks -------------------------------------------------------------------------
def update_with_sentinels(dw, objs):
    """dw.update(objs) with every voxel byte replaced by a sentinel first: (scene, count returned, mask of the chunks the update
    wrote).  The chunks it did not write get their bytes back, so that the world can be compared afterwards."""
    cs = dw.chunk_size
    buf = dw._voxels
    good = buf.clone()
    buf.fill_(0xEE)
    ps, rebuilt = dw.update(objs)
    assert dw._voxels is buf                                     # an incremental update keeps its buffer
    written = (buf.view(-1, cs ** 3) != 0xEE).any(1)             # (a rebuilt chunk holds ids of <= 255 materials and zeros)
    buf.view(-1, cs ** 3)[~written] = good.view(-1, cs ** 3)[~written]
    return ps, rebuilt, written.cpu().numpy()


@gpu
def test_script_b_one_world_one_camera_40_ticks():
    """Script B on one DeviceWorld watched by one Camera.  After every tick: the merge order, the number of chunks rebuilt and
    the very chunks written are the script's; voxels, presence and material rows are the host build's over that order (and a
    fresh DeviceWorld's); the models of the edited sprites are the host Frames; the owners of the same 256 rays are the host
    owner volume's; and the frame is the oracle's over the tick's grid seen through the chunk table of the camera's last
    selection -- made every third tick, stale in between, dropped when a full rebuild hands out a new scene."""
    from python_raytracer_amd import Camera
    S, H = sq.ScriptB(), sq.CameraB()
    cs = S.cs
    st = ol.make_settings(**sq.SETTINGS_B)
    dw = DeviceWorld(cs)
    cam = Camera(settings=settings_store(st))
    cam.rot, cam.lens = quaternion(*sq.CAM_ROT_B), st["fov"] * np.pi / 8
    held, prev, rays = None, None, None
    renumbered = 0
    for k in range(sq.N_TICKS_B):
        exp = S.run(k)
        mats_before = [id(m) for m in dw.materials]
        if exp["full"]:
            ps, rebuilt = dw.update(S.objs)
            written = None
        else:
            ps, rebuilt, written = update_with_sentinels(dw, S.objs)
        assert not any(o.redraw for o in dw.order), k                # update() cleared the flags of what it voxelised
        S.done()
        # ---- order, chunk count, untouched chunks
        assert [id(o) for o in dw.order] == [id(o) for o in exp["order"]], k
        assert rebuilt == exp["chunks"], (k, rebuilt, exp["chunks"])
        if written is not None:
            dims = [int(d) for d in S.dims]
            cells = sorted((x * dims[1] + y) * dims[2] + z for x, y, z in exp["cells"])
            assert np.flatnonzero(written).tolist() == cells, (k, np.flatnonzero(written).tolist(), cells)
        # ---- world: voxels, presence, material rows
        grid, present = _merge_world(dw, cs)
        _assert_same_world(dw, ps, World(S.origin, S.dims, cs, present, grid, dw.materials))
        w, hgrid, hown = S.host_world()
        assert np.array_equal(grid != 0, hgrid != 0) and int((grid != 0).sum()) > 500
        ids = [id(m) for m in dw.materials]
        assert len(set(ids)) == len(ids) and {id(m) for m in w.materials} <= set(ids)
        rows = np.array([material_row(m)[:7] for m in dw.materials], np.float64).reshape(-1, 7)
        assert np.array_equal(ps.materials[:, :7], rows)
        assert np.array_equal(ps.device_tensors["materials"].cpu().numpy()[:rows.size + len(rows)].reshape(-1, 8)[:, :7], rows)
        if k and exp["full"]:
            both = [m for m in mats_before if m in ids]
            renumbered += [m for m in ids if m in mats_before] != both
        # ---- a fresh DeviceWorld over the same order is the host build
        fresh = DeviceWorld(cs)
        _assert_same_world(fresh, fresh.build(list(dw.order)), build_world(list(dw.order), cs))
        # ---- models of the edited sprites
        shown = {(id(o.sprite), int(o.sprite.frame)) for o in dw.order}
        for name in sorted(S.edited):
            spr = S.sprites[name]
            for f in range(len(spr.frames)):
                if (id(spr), f) not in shown:
                    try:                                             # a frame nothing shows: resident only if it was shown before
                        dw.model(spr, f)
                    except ValueError:
                        continue
                got, smats = dw.model(spr, f)
                host, hmats = spr.dense(f)
                assert np.array_equal(got != 0, host != 0), (k, name, f)
                assert [id(smats[i - 1]) for i in got[got != 0]] == [id(hmats[i - 1]) for i in host[host != 0]], (k, name, f)
        # ---- the camera: a new scene object only after a full rebuild
        assert (ps is not held) == bool(exp["full"]), k
        cam.pos = vec3(*sq.cam_pos_b(k))
        if ps is not held:
            cam.set_world_scene(ps)
            held = ps
            H.new_scene()
        if k == 0:
            rays = S.make_rays()
            prev = cam.render(0, want_ray_rgba=True)                 # every present chunk at resolution 1
            o = sq.render_b(k, H.scene(S.origin, S.dims, cs, grid, rows))
            frame_equals_oracle(prev, o, cs)
            H.traversed = o["traversed"]
        if k % sq.SELECT_EVERY == 0:
            cam.chunk_update(prev)
            H.select(k, S.origin, S.dims, cs, present)
        scene = H.scene(S.origin, S.dims, cs, grid, rows)
        table = (cam._camera_table if cam._camera_table is not None else ps.device_tensors["chunk_table"])
        table = table.cpu().numpy().view(np.uint32).reshape(scene.present.shape)
        assert np.array_equal((table != 0).astype(np.uint8), scene.present), k
        assert np.array_equal((table >> 24).astype(np.uint8)[table != 0], scene.res[table != 0]), k
        # ---- owners of the same 256 rays
        hits = cam.cast_rays(*rays)
        h = hits.numpy()
        cr.assert_records_equal(h, cr.march_records(scene, round(cs / 2), *rays))
        res = dw.owners(hits, cam)
        own = res.numpy()
        want, ambiguous = orf.expect_owners(scene, World(S.origin, S.dims, cs, present, grid, dw.materials, hown), list(dw.order), h)
        for f in ("object", "resolution", "voxel", "local"):
            assert np.array_equal(own[f], want[f]), (k, f)
        check_no_hit_records(own, h)
        check_stats(res.stats, own, h, ambiguous)
        # ---- the frame
        prev = cam.render(0, want_ray_rgba=True)
        o = sq.render_b(k, scene)
        frame_equals_oracle(prev, o, cs)
        H.traversed = o["traversed"]
    assert renumbered >= 1 and len(dw.materials) == 10
    assert dw.edit_calls["edit"] > 10 and dw.edit_calls["stamp"] >= 2 and dw.edit_calls["resync"] >= 3, dw.edit_calls


# ---- the pow memo past its capacity (last: it fills the library's 64 tables) ----------------------------------------------------
@gpu
def test_pow_memo_past_its_capacity():
    import torch
    from python_raytracer_amd import _native as nat
    from python_raytracer_amd.camera import release_caches
    sc = ol.default_scene()
    base = sq.walk_a()[0]
    st = ol.make_settings(**dict(sq.MEMO_SETTINGS, falloff=sq.MEMO_FALLOFFS[0]))
    store = settings_store(st)
    cam = camera_for(sc, store, base.pos, base.rot, base.lens)

    def held(r, falloff):
        shot = sq.Shot(0, "memo", dict(st, falloff=falloff), base.pos, base.rot, base.lens, 0, {}, (), ())
        o = oracle_of(sc, shot, r.pixels)
        assert len(np.unique(o["rays"]["bounces"])) >= 3             # (several bases go through the memo)
        frame_equals_oracle(r, o, CS_A)

    assert len(set(sq.MEMO_FALLOFFS)) == 70
    release_caches()
    try:
        for k, falloff in enumerate(sq.MEMO_FALLOFFS):
            store.falloff = falloff
            r = cam.render(0, want_ray_rgba=True)
            if k in sq.MEMO_HELD:
                held(r, falloff)
        # the library's tables are all taken: one more falloff gets none (and the last six frames memoised on their own)
        with torch.cuda.device(cam._device):
            assert nat.lib().vrt_pow_memo_create(7.5) == nat.ERR_WORKSPACE
        release_caches()
        held(cam.render(0, want_ray_rgba=True), sq.MEMO_FALLOFFS[-1])
    finally:
        release_caches()
