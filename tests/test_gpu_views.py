"""Many camera poses of one scene in one launch (Camera.render_views -> vrt_render_views, march_views_kernel): every view of
a batch must be, bit for bit, the frame Camera.render gives for that pose -- per-sample colours, fp32 means, the RGBA8
image and the traversed keys cell by cell -- and the batch's statistics the sum of the single frames'.  Two views are also
compared with the oracle directly, so that the batch is not only held against code that shares its bodies.

The windows are tiny on purpose: 15 x 11 x 3 samples is 495 ray slots per view, no multiple of 64, so waves (and the
128-ray hand-outs) straddle view boundaries; lod_edge leaves sample slots unused."""
import ctypes as C
import hashlib

import numpy as np
import pytest

import oracle_lib as ol
from gpu_util import HANDOUT_KNOBS, camera_for, launches_of, run_children, settings_store, sparse_scene
from python_raytracer_amd import _native as nat

gpu = pytest.mark.gpu

CS = 8
W, H, SAMPLES = 15, 11, 3
IDENTITY = (0.0, 0.0, 0.0, 1.0)
ROTATED = tuple(np.array([0.35, -0.2, 0.55, 0.73]) / np.linalg.norm([0.35, -0.2, 0.55, 0.73]))
# the sparse world is 6^3 chunks of 8 cells round the origin: [-24, 24)^3
POSES = [
    ((0.3, 0.6, -10.45), IDENTITY),            # the default pose: inside the world, looking along +z
    ((1.3, 2.6, 3.45), ROTATED),               # a rotated camera (the reference's product does not keep the norm: a larger box)
    ((8.01, -3.5, 15.99), IDENTITY),           # another chunk, a hundredth of a cell from two chunk faces
    ((5000.5, 4000.5, -3000.5), IDENTITY),     # far outside the world: every ray ends in the sky
    ((0.3, 0.6, -10.45), IDENTITY),            # the first again
]


# The instance a batch's march runs, by the highest resolution of the scene's chunks, and the two re-trace instances every batch
# launches behind it (they return at once when their lists are empty): what the launch census must show for a render_views call
VIEWS_INSTANCE = {1: 'march_views_kernel<8,0,false,0>', 2: 'march_views_kernel<8,1,false,0>', 3: 'march_views_kernel<4,2,false,0>'}
VIEWS_RETRACES = {'march_views_kernel<4,2,true,1>', 'march_views_kernel<4,2,true,2>'}


def settings(**kw):
    return ol.make_settings(**dict(dict(width=W, height=H, samples=SAMPLES, chunk_size=CS, dist_max=48, max_bounces=4.0,
                                        lod_edge=0.5), **kw))


def lens_of(st):
    return st["fov"] * np.pi / 8


_scenes = {}


def scene(res_max):
    if res_max not in _scenes:
        _scenes[res_max] = sparse_scene(300 + res_max, res_max, chunk_size=CS, fill=0.05)
    return _scenes[res_max]


def set_pose(cam, pose):
    from python_raytracer_amd.lib import vec3, quaternion
    cam.pos = vec3(*[float(v) for v in pose[0]])
    cam.rot = quaternion(*[float(v) for v in pose[1]])


def singles(cam, poses, **kw):
    out = []
    for p in poses:
        set_pose(cam, p)
        out.append(cam.render(0, want_ray_rgba=True, **kw))
    return out


def keys_in_box(r, origin, dims, cs):
    """r's traversed keys as a [dims] array whose cell (0, 0, 0) is the chunk at `origin`: cells r's own box does not cover
    read -1 (never visited); r's box must lie inside the other."""
    k = r.traversed_keys.cpu().numpy().reshape(r.trav_dims)
    lo = (np.array(r.trav_origin) - np.array(origin)) // cs
    assert (lo >= 0).all() and (lo + np.array(r.trav_dims) <= np.array(dims)).all(), (r.trav_origin, r.trav_dims, origin, dims)
    out = np.full(tuple(dims), -1, np.int64)
    out[lo[0]:lo[0] + r.trav_dims[0], lo[1]:lo[1] + r.trav_dims[1], lo[2]:lo[2] + r.trav_dims[2]] = k
    return out


def assert_view_equals_single(b, s, cs):
    assert np.array_equal(b.ray_rgba.cpu().numpy(), s.ray_rgba.cpu().numpy())
    assert np.array_equal(b.rgba_f32.cpu().numpy().view(np.uint32), s.rgba_f32.cpu().numpy().view(np.uint32))
    assert np.array_equal(b.image_u8.cpu().numpy(), s.image_u8.cpu().numpy())
    assert b.traversed(cs) == s.traversed(cs)
    # the raw keys, cell by cell: the batch's boxes take the largest dimensions of the batch, centred on the same chunk
    assert np.array_equal(b.traversed_keys.cpu().numpy().reshape(b.trav_dims), keys_in_box(s, b.trav_origin, b.trav_dims, cs))


def digest(results):
    h = hashlib.sha256()
    for r in results:
        for t in (r.ray_rgba, r.rgba_f32, r.image_u8):
            h.update(t.cpu().numpy().tobytes())
        h.update(repr(r.traversed(CS)).encode())
    return h.hexdigest()


@gpu
@pytest.mark.parametrize("res_max", [1, 2, 3])   # the resolution-1, resolution <= 2 and generic instances of the kernel
def test_batch_equals_single_frames(res_max):
    st = settings()
    sc = scene(res_max)
    cam = camera_for(sc, settings_store(st), *POSES[0], lens_of(st))
    ref = singles(cam, POSES)
    assert int(cam._c_scene(cam._ensure_scene()).max_resolution) == res_max
    smax = ref[0].max_samples
    assert (W * H * smax) % 64 != 0
    assert (ref[0].ray_rgba.cpu().numpy().reshape(-1, smax)[:, -1] == 0).any(), "no pixel with fewer than smax samples"
    set_pose(cam, POSES[2])   # (the camera's own pose plays no part in a batch)
    got, ran = launches_of(lambda: cam.render_views(POSES, want_ray_rgba=True))
    assert ran == {VIEWS_INSTANCE[res_max]} | VIEWS_RETRACES, ran   # the instance the parametrisation names, and no other
    assert len(got) == len(POSES)
    for b, s in zip(got, ref):
        assert_view_equals_single(b, s, CS)
    total = np.sum([s.stats[:12] for s in ref], axis=0)
    assert (got[0].stats[:12] == total).all(), (got[0].stats, total)
    assert int(got[0].stats[8]) > 0 and (got[0].stats[12:] == 0).all()
    assert got[0].stats is got[4].stats
    for name in ("ray_rgba", "rgba_f32", "image_u8", "traversed_keys"):
        assert np.array_equal(getattr(got[0], name).cpu().numpy(), getattr(got[4], name).cpu().numpy())
    # the far camera saw nothing but sky, and its list is its own
    assert int(ref[3].stats[4]) == 0 and got[3].trav_origin != got[0].trav_origin
    # a [V, 7] array is the same batch
    arr = np.array([list(p) + list(q) for p, q in POSES])
    again = cam.render_views(arr, want_ray_rgba=True)
    assert digest(again) == digest(got)


@gpu
@pytest.mark.parametrize("res_max", [1, 2, 3])
def test_batch_against_the_oracle(res_max):
    st = settings()
    sc = scene(res_max)
    cam = camera_for(sc, settings_store(st), *POSES[0], lens_of(st))
    got, ran = launches_of(lambda: cam.render_views(POSES, want_ray_rgba=True))
    assert ran == {VIEWS_INSTANCE[res_max]} | VIEWS_RETRACES, ran
    px = got[0].pixels
    for v in (1, 2):   # the rotated camera, the one beside the chunk faces
        o = ol.render(sc, st, POSES[v][0], POSES[v][1], lens_of(st), px, libm=ol.LIBM_PORTABLE)
        r = got[v]
        assert np.array_equal(r.rgba_f32.cpu().numpy(), o["pix_mean"].astype(np.float32))
        assert np.array_equal(np.array(r.traversed(CS), np.int64).reshape(-1, 3), np.asarray(o["traversed"]).reshape(-1, 3))
        rays = o["rays"]
        where = {(int(x), int(y)): i for i, (x, y) in enumerate(r.pixels)}
        slot = np.array([where[(int(x), int(y))] for x, y in zip(rays["x"], rays["y"])], np.int64) * r.max_samples + rays["s"]
        packed = (rays["color"][:, 0].astype(np.uint32) | (rays["color"][:, 1].astype(np.uint32) << 8) |
                  (rays["color"][:, 2].astype(np.uint32) << 16) | (rays["alpha"].astype(np.uint32) << 24))
        assert np.array_equal(r.ray_rgba.cpu().numpy().view(np.uint32)[slot], packed)
    # the counters of the whole batch are the oracle's, summed over the views
    total = np.sum([ol.render(sc, st, p, q, lens_of(st), px, libm=ol.LIBM_PORTABLE, want_rays=False, want_traversed=False)["counters"]
                    for p, q in POSES], axis=0)
    assert (got[0].stats[:8] == total).all(), (got[0].stats[:8], total)


@gpu
def test_one_view_equals_render():
    st = settings()
    cam = camera_for(scene(2), settings_store(st), *POSES[1], lens_of(st))
    ref = singles(cam, POSES[1:2])[0]
    got = cam.render_views(POSES[1:2], want_ray_rgba=True)
    assert len(got) == 1
    assert_view_equals_single(got[0], ref, CS)
    assert got[0].trav_dims == ref.trav_dims and got[0].trav_origin == ref.trav_origin
    assert (got[0].stats[:12] == ref.stats[:12]).all()


@gpu
def test_batch_calls_share_the_pose_records_and_leave_the_camera_alone():
    """16 x 9 x 1, an unrotated and a rotated pose: first_hit_views and render_views of the same poses use one device copy of
    the records; the boxes are sized from the poses' rotations, not by moving the camera; every view's box has the largest
    dimensions of the batch."""
    st = settings(width=16, height=9, samples=1)
    poses = POSES[:2]
    cam = camera_for(scene(2), settings_store(st), *POSES[2], lens_of(st))
    pos, rot = cam.pos, cam.rot
    assert len(cam.first_hit_views(poses)) == 2
    cams = cam._views_cams[1]
    ptr = cams.data_ptr()
    got = cam.render_views(poses, want_traversed=True)
    assert cam._views_cams[1] is cams and cams.data_ptr() == ptr
    assert cam.pos is pos and cam.rot is rot
    n = [2 * cam._box_radius(q) + 1 for _, q in poses]
    assert n[1] > n[0]
    for r in got:
        assert r.trav_dims == [n[1]] * 3 and r.traversed_keys.numel() == n[1] ** 3
    assert got[0].trav_origin != got[1].trav_origin


@gpu
def test_batch_with_one_ray_record_per_pixel():
    """dof, lod_random and lod_samples all 0: the ray table holds one record per PIXEL, and a ray's first-hit draws come from
    the draw table (the other layout of take_ray_views)."""
    st = settings(dof=0.0, lod_random=0.0, lod_samples=0.0)
    cam = camera_for(scene(2), settings_store(st), *POSES[0], lens_of(st))
    ref = singles(cam, POSES[:3])
    got = cam.render_views(POSES[:3], want_ray_rgba=True)
    for b, s in zip(got, ref):
        assert_view_equals_single(b, s, CS)
    assert (got[0].stats[:12] == np.sum([s.stats[:12] for s in ref], axis=0)).all()


@gpu
@pytest.mark.parametrize("n_views", [70, 100])
def test_more_views_than_a_workgroup_has_waves(n_views):
    """8 x 6 x 1: 48 slots per view, so a wave holds rays of two views and a 128-ray hand-out of three or four; 70 views are
    more than a workgroup has waves, 100 more than the view records staged in LDS (96: the rest is read from memory)."""
    st = settings(width=8, height=6, samples=1, lod_edge=0.0)
    rng = np.random.default_rng(70)
    poses = []
    for _ in range(n_views):
        q = rng.normal(size=4)
        poses.append((tuple(rng.uniform(-20, 20, 3)), tuple(q / np.linalg.norm(q))))
    cam = camera_for(scene(2), settings_store(st), *poses[0], lens_of(st))
    ref = singles(cam, poses)
    got = cam.render_views(poses, want_ray_rgba=True)
    assert digest(got) == digest(ref)
    assert (got[0].stats[:12] == np.sum([s.stats[:12] for s in ref], axis=0)).all()


def _split_child():
    """Run in a child process with VRT_BATCH_LOG2=12 (read once per process): 20 views of 495 slots are then marched as three
    launches of 8 + 8 + 4 views, more views than the first launch holds; prints one digest of the batch and one of the
    single frames."""
    st = settings(max_bounces=16.0, max_light=100.0, lod_bounces=0.0)   # (the re-trace tests' settings; this scene's rays stay within 32 draws: _handout_child)
    rng = np.random.default_rng(20)
    poses = []
    for _ in range(20):
        q = rng.normal(size=4)
        poses.append((tuple(rng.uniform(-20, 20, 3)), tuple(q / np.linalg.norm(q))))
    cam = camera_for(scene(3), settings_store(st), *poses[0], lens_of(st))
    ref = []
    for p in poses:
        cam.fast_draws = 32
        ref += singles(cam, [p])
    cam.fast_draws = 32
    got = cam.render_views(poses, want_ray_rgba=True)
    for b, s in zip(got, ref):
        assert_view_equals_single(b, s, CS)
    total = np.sum([s.stats[:12] for s in ref], axis=0)
    assert (got[0].stats[:12] == total).all(), (got[0].stats, total)
    print("SPLIT", digest(got), digest(ref), int(got[0].stats[8]), int(got[0].stats[9]))


@gpu
def test_batch_split_into_launches_at_view_boundaries():
    """A batch beyond the slots of one march launch (2^28; VRT_BATCH_LOG2 lowers it, once per process -- hence the child) is
    marched as several launches that end at view boundaries: each clears its counters and re-trace lists, begins at its
    own first view and stages that view's records."""
    import os
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, VRT_BATCH_LOG2="12", PYTHONPATH=os.pathsep.join([here, os.path.dirname(here)]))
    out = subprocess.run([sys.executable, "-c", "import test_gpu_views as t; t._split_child()"], env=env, cwd=here,
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    words = [l for l in out.stdout.splitlines() if l.startswith("SPLIT")][0].split()
    assert words[1] == words[2] and int(words[3]) > 20 * 400


def _handout_child():
    """_split_child's scene and settings (rays that re-trace: the LIST instances hand out too), 5 views of 495 slots -- 2 475 is
    no multiple of 64 or 128; prints one digest per batch and the statistics."""
    st = settings(max_bounces=16.0, max_light=100.0, lod_bounces=0.0)
    rng = np.random.default_rng(20)
    poses = []
    for _ in range(5):
        q = rng.normal(size=4)
        poses.append((tuple(rng.uniform(-20, 20, 3)), tuple(q / np.linalg.norm(q))))
    cam = camera_for(scene(3), settings_store(st), *poses[0], lens_of(st))
    cam.fast_draws = 32
    got = cam.render_views(poses, want_ray_rgba=True)
    assert len(got) == 5 and got[0].ray_rgba.numel() == 495
    # (the CPU oracle finds at most 4 rough hits per ray in that scene -- 15 draws -- so none of its rays outruns 32 draws;
    # the re-trace instances get their rays from the weakly absorbing scene of test_retraces_in_a_batch, 5 views as well)
    st2 = settings(max_bounces=16.0, max_light=100.0, lod_bounces=0.0, falloff=0.0)
    poses2 = BOUNCY_POSES + [((-1.2, 0.9, 1.1), IDENTITY), ((0.3, 0.6, 0.45), ROTATED)]
    cam2 = camera_for(bouncy_scene(), settings_store(st2), *poses2[0], lens_of(st2))
    cam2.fast_draws = 32
    got2 = cam2.render_views(poses2, want_ray_rgba=True)
    assert len(got2) == 5 and got2[0].ray_rgba.numel() == 495
    print("HANDOUT", digest(got), digest(got2), " ".join(str(int(v)) for v in list(got[0].stats[:12]) + list(got2[0].stats[:12])))


@gpu
def test_batch_does_not_depend_on_the_hand_out():
    """march_views_kernel and its two re-trace instances under the scheduling knobs the frame kernels are tested with
    (test_scheduling_knobs_do_not_change_results): images, per-ray colours, traversed lists and statistics are the same."""
    lines = run_children("import test_gpu_views as t; t._handout_child()", HANDOUT_KNOBS, "HANDOUT")
    for knobs, words in zip(HANDOUT_KNOBS, lines):
        print(knobs, words[1][:16], words[2][:16], words[3:])
    assert len(lines[0]) == 3 + 24
    assert int(lines[0][3 + 12 + 9]) > 0, "no ray was re-traced"
    for knobs, words in zip(HANDOUT_KNOBS[1:], lines[1:]):
        assert words[1:] == lines[0][1:], (knobs, words, lines[0])


# weakly absorbing rough materials: many rough hits per ray, three draws each
MATS_BOUNCY = np.array([[200, 180, 160, 1.0, 0.05, 1.0, 0.0], [90, 120, 250, 0.5, 0.05, 0.5, 0.0], [60, 200, 90, 0.1, 0.5, 0.75, 0.0],
                        [230, 230, 230, 0.0, 2.0, 1.0, 0.0]])
BOUNCY_POSES = [((0.3, 0.6, 0.45), IDENTITY), ((1.3, -0.4, 0.45), ROTATED), ((0.3, 0.6, 0.45), IDENTITY)]


def bouncy_scene():
    rng = np.random.default_rng(411)
    dims = np.array([4, 4, 4])
    origin = -(dims // 2) * CS
    shape = tuple(dims * CS)
    present = np.ones(tuple(dims), np.uint8)
    res = np.ones(tuple(dims), np.uint8)
    grid = np.where(rng.random(shape) < 0.3, rng.integers(1, 5, shape), 0).astype(np.uint8)
    grid[12:20, 12:20, 12:20] = 0   # a pocket round the cameras
    return ol.Scene(origin, dims, CS, present, res, ol.Scene.camera_grid(grid, origin, dims, CS, present, res), MATS_BOUNCY)


@gpu
def test_retraces_in_a_batch():
    """Rays that outrun the 32-draw table are re-traced from a list of batch offsets, with 113-draw rows and (the few that
    outrun those) 1 024-draw rows: both tiers must find their ray's view again.  15 x 11 x 3 is enough: the single frames
    re-trace at this size (asserted)."""
    sc = bouncy_scene()
    st = settings(max_bounces=16.0, max_light=100.0, lod_bounces=0.0, falloff=0.0)
    poses = BOUNCY_POSES
    cam = camera_for(sc, settings_store(st), *poses[0], lens_of(st))
    ref = []
    for p in poses:
        cam.fast_draws = 32   # (render() moves on to 64 draws per seed once many rays re-trace: every frame here starts at 32)
        ref += singles(cam, [p])
    assert all(int(s.stats[9]) > 0 for s in ref), [int(s.stats[9]) for s in ref]
    assert max(int(s.stats[5]) for s in ref) > 0
    cam.fast_draws = 32
    got, ran = launches_of(lambda: cam.render_views(poses, want_ray_rgba=True))
    assert ran == {VIEWS_INSTANCE[1]} | VIEWS_RETRACES, ran   # (the two re-trace instances with work to do: stats[9], and below)
    assert int(got[0].stats[9]) > 0
    for b, s in zip(got, ref):
        assert_view_equals_single(b, s, CS)
    assert (got[0].stats[:12] == np.sum([s.stats[:12] for s in ref], axis=0)).all()


@gpu
def test_batches_fail_loudly():
    st = settings()
    sc = scene(1)
    cam = camera_for(sc, settings_store(st), *POSES[0], lens_of(st))
    with pytest.raises(ValueError, match="at least one pose"):
        cam.render_views([])
    cam.cache_draws = False
    with pytest.raises(ValueError, match="cache_draws"):
        cam.render_views(POSES)
    cam.cache_draws = True
    # unequal lenses: vrt_camera records as the C ABI takes them ([V, 8]: pos, rot, lens) -- the library cannot read the
    # records on the device, so the wrapper compares them before the upload
    rec = np.array([list(p) + list(q) + [lens_of(st)] for p, q in POSES])
    rec[3, 7] *= 1.5
    with pytest.raises(ValueError, match="lens"):
        cam.render_views(rec)
    far = list(POSES)
    far[2] = ((float(1 << 28), 0.0, 0.0), IDENTITY)
    with pytest.raises(ValueError, match="outside the range"):
        cam.render_views(far)
    nan = list(POSES)
    nan[1] = ((0.0, float("nan"), 0.0), IDENTITY)
    with pytest.raises(ValueError):
        cam.render_views(nan)
    moving = camera_for(sc, settings_store(settings(static=False)), *POSES[0], lens_of(st))
    with pytest.raises(ValueError, match="static"):
        moving.render_views(POSES)
    assert len(cam.render_views(POSES)) == len(POSES)   # ... and the camera still renders


@gpu
def test_batched_frame_is_graph_capturable():
    import torch
    st = settings()
    cam = camera_for(scene(2), settings_store(st), *POSES[0], lens_of(st))
    ref = cam.render_views(POSES, want_ray_rgba=True)      # also warms the plan, the tables, the workspace and the pow memo
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        cam.render_views(POSES, want_ray_rgba=True, check=False)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        r = cam.render_views(POSES, want_ray_rgba=True, check=False)
    for _ in range(2):
        for v in r:
            v.rgba_f32.zero_()
            v.image_u8.zero_()
            v.ray_rgba.zero_()
            v.traversed_keys.zero_()
        g.replay()
        torch.cuda.synchronize()
        for a, b in zip(r, ref):
            for name in ("ray_rgba", "rgba_f32", "image_u8", "traversed_keys"):
                assert torch.equal(getattr(a, name), getattr(b, name)), name
        assert (r[0]._stats_dev.cpu().numpy()[:12] == ref[0].stats[:12]).all()


# ---- without a GPU ---------------------------------------------------------------------------------------------------
def test_abi_9_exports_the_batched_entry_points():
    L = nat.lib()
    assert L.vrt_abi_version() == 9 and nat.ABI_VERSION == 9
    assert L.vrt_render_views is not None and L.vrt_views_workspace_bytes is not None
    assert "vrt_render_views" in nat.EXPORTS and "vrt_views_workspace_bytes" in nat.EXPORTS


def test_render_views_rejects_bad_arguments_without_a_device():
    """Everything vrt_render_views can refuse is refused before its first HIP call: these calls carry made-up device
    pointers, which nothing reads."""
    L = nat.lib()
    st = nat.VrtSettings(W, H, SAMPLES, CS, 4, 1, 0, 0.875, .25, .25, .5, 0, 48, 1, 4, .5, .5, .25, .5)
    fake = 0x1000
    sc = nat.VrtScene()
    sc.origin[:] = [-24, -24, -24]
    sc.dims[:] = [6, 6, 6]
    sc.chunk_size, sc.n_slots, sc.n_materials, sc.max_resolution = CS, 10, 4, 1
    sc.d_chunk_table = sc.d_voxels = sc.d_materials = fake
    n_px, smax = W * H, L.vrt_max_samples(C.byref(st))
    nb = C.c_int64(0)
    assert L.vrt_views_workspace_bytes(C.byref(st), 5, n_px, C.byref(nb)) == 0 and nb.value >= 5 * n_px * smax * 4 + 5 * 80
    assert L.vrt_views_workspace_bytes(C.byref(st), 0, n_px, C.byref(nb)) == -1
    assert L.vrt_views_workspace_bytes(C.byref(st), 1 << 20, 1 << 20, C.byref(nb)) == -1     # 2^32 slots and more

    def call(cams=fake, n_views=2, settings=st, draw=fake, rtab=fake, rays=None, trav=None):
        return L.vrt_render_views(C.byref(sc), C.byref(settings), cams, n_views, fake, n_px, fake, 100, 32, draw, rtab, fake,
                                  nb.value, None, None, None, rays, fake, trav, None)

    assert call(cams=None) == -1
    assert call(n_views=0) == -1
    nonstatic = nat.VrtSettings(W, H, SAMPLES, CS, 4, 1, 77, 0.875, .25, .25, .5, 0, 48, 1, 4, .5, .5, .25, .5)
    assert call(settings=nonstatic) == -1          # seed_nonce != 0
    assert call(draw=None) == -1 and call(rtab=None) == -1
    assert call(rays=fake) == -1                   # no debug records of a batch

    def boxes(origins, dims=((3, 3, 3), (3, 3, 3)), keys=(fake, fake + 27 * 8)):
        t = (nat.VrtTraversed * 2)()
        for v in range(2):
            t[v].origin[:] = origins[v]
            t[v].dims[:] = dims[v]
            t[v].d_keys = keys[v]
        return t

    assert call(trav=boxes([(0, 0, 0), (1 << 28, 0, 0)])) == -1              # the second view's origin out of range
    assert call(trav=boxes([(0, 0, 0), (0, 4, 0)])) == -1                    # ... not a multiple of the chunk size
    assert call(trav=boxes([(0, 0, 0), (8, 0, 0)], dims=((3, 3, 3), (3, 3, 4)))) == -1   # unequal dims
    assert call(trav=boxes([(0, 0, 0), (8, 0, 0)], keys=(fake, fake + 28 * 8))) == -1    # keys not view after view
