"""The frame march at the operating points it ships at.

tests/test_gpu_parity.py forces the kernel choice for every test (VRT_POOL, VRT_POOL_MIN_RAYS, VRT_WADDR) and holds small
scenes bit-exact against the oracle.  This file has NO fixture that sets a VRT_* variable: frames of real size run with the
environment the library ships with, so the launch policy itself (launch_march, pool_plan, march_defer and the bm_window
branch of fill_params in python_raytracer_amd/csrc/vrt_kernels.hip) is under test.  A leg that needs a knob sets it for that
leg only (`knobs`) and restores it.

  A  BASELINE config 5 at full size (1024^3 volume, 4096 x 4096, 16 spp) against the oracle on every 64th pixel, and its
     `traversed` against the oracle's list and against the instances the small-scene tests pin to the oracle.
  B  config 5 as the eight shards BASELINE defines it on.
  C  which instantiation runs where: kernel names of profiled bench.py children against the committed profiles/ set, and
     the ray pool's size threshold through stats[12].
  D  the settled-bitmap window and traversed boxes the caller supplies through the C ABI, small scenes, every ray.

Wall time of this file on an MI355X, measured (the tests print their own figures, run with -s): 26 s in all -- the whole
GPU suite with it took 158 s in the same session, the suite without it was recorded at 97 s (GPUTEST_r04.json) -- A 6.4 s (2.3 s to build the volume and the camera, 0.6 s for the shipped frame, 2.2 s to
copy the volume back and check its slabs, 0.7 s of oracle on 16 threads, 0.5 s for the two instance legs), B 3.7 s (both
partitions), C 15.2 s (the four profiled bench.py children 3.0, 3.0, 3.2 and 5.1 s; the threshold legs 1.0 s), D 0.7 s
(twelve boxes of twelve legs each, 0.05 s a box).
"""
import contextlib
import hashlib
import math
import os
import shutil
import signal
import subprocess
import sys
import time

import numpy as np
import pytest

import oracle_lib as ol
import profile_util as pu
from gpu_util import bitmap_window, camera_for, settings_store, sparse_scene, window_split

pytestmark = pytest.mark.gpu

# the knobs of the launch policy: none of them may be set where the shipped environment is what a test is about
POLICY_KNOBS = ("VRT_POOL", "VRT_POOL_MIN_RAYS", "VRT_WADDR", "VRT_DEFER_VISIT", "VRT_TRAV_WINDOW", "VRT_TRAV_LDS", "VRT_TILED",
                "VRT_LOOKUP", "VRT_SPEC_DEEP", "VRT_RESMODE", "VRT_FUSE_RAYGEN", "VRT_TABLE_IDENTITY", "VRT_BATCH_LOG2")


def shipped_environment():
    set_ = [k for k in POLICY_KNOBS if k in os.environ]
    assert not set_, "this test is about the library's defaults, but the environment sets %s" % set_


@contextlib.contextmanager
def knobs(**kw):
    """Set VRT_* variables for one leg (the library reads these at every launch) and put the old state back."""
    old = {k: os.environ.get(k) for k in kw}
    os.environ.update({k: str(v) for k, v in kw.items()})
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def pool_groups(stats):
    return int(stats[12]) & 0xffffffff          # (bits 32+: the workgroups that took their rays as tiles)


def report(part, what, t0):
    print("[operating points %s] %s: %.1f s" % (part, what, time.perf_counter() - t0))


# ------------------------------------------------------------------------------------------------- config 5
C5 = dict(n=1024, cs=16, width=4096, height=4096, samples=16, rays=268435456)


class Config5:
    """The 1024^3 volume on the device (vrt_synth_volume) and a camera over it with bench.py's c5 settings and
    test_config5_full_size_properties' camera; built once per module."""

    def __init__(self):
        import torch
        import bench
        from python_raytracer_amd import Camera, PackedScene, _native as nat
        from python_raytracer_amd.lib import vec3, quaternion
        n, cs = C5["n"], C5["cs"]
        d = n // cs
        cfg = bench.CONFIGS["c5"]
        assert (cfg["width"], cfg["height"], cfg["samples"]) == (C5["width"], C5["height"], C5["samples"])
        self.mats = ol.default_scene().materials
        table = torch.zeros(d ** 3, dtype=torch.int32, device="cuda")
        vox = torch.zeros(n ** 3, dtype=torch.uint8, device="cuda")
        nat.check(nat.lib().vrt_synth_volume(n, cs, table.data_ptr(), vox.data_ptr(), None), "vrt_synth_volume")
        self.st = ol.make_settings(width=cfg["width"], height=cfg["height"], samples=cfg["samples"],
                                   max_bounces=float(cfg["max_bounces"]), **cfg["over"])
        assert self.st["chunk_size"] == cs
        self.cam = Camera(settings=settings_store(self.st))
        self.scene = PackedScene.from_device([-n // 2] * 3, [d] * 3, cs, table, vox, d ** 3, self.mats, max_resolution=1)
        self.cam.set_packed_scene(self.scene)
        self.pos, self.rot = [0.5, 0.5, 0.5], [0.0, 0.0, 0.0, 1.0]
        self.cam.pos, self.cam.rot = vec3(*self.pos), quaternion(*self.rot)
        self._host = None

    def host_scene(self):
        """The oracle's scene, unpacked from the device volume the way bench.host_volume does."""
        if self._host is None:
            import bench
            self._host = bench.host_volume(self.cam._ensure_scene(), self.mats)
        return self._host


@pytest.fixture(scope="module")
def c5():
    import torch
    c = Config5()
    yield c
    del c
    torch.cuda.empty_cache()


def test_config5_full_size_vs_oracle(c5):
    """BASELINE config 5 as bench.py runs it -- default environment, march_pool_kernel's DEFER instance with the settled
    bitmap over the 32^3 cells around the camera, the identity chunk table and one ray record per pixel over 1 GiB of
    voxels -- against the oracle on every 64th pixel in x and y (4096 pixels, 65536 rays): per-sample packed RGBA, fp32
    means and RGBA8 bit-identical; ray count, no exhausted or out-of-box rays; the pool kernel ran.
    The oracle's scene is the DEVICE volume copied back (bench.host_volume); a few z-slabs of it are compared with
    oracle_lib.synth_scene's hash so that it is itself tied to the reference generator.
    `traversed`, two ways: (1) every chunk in the oracle's list for the sampled pixels is marked visited in the GPU frame;
    (2) the whole frame's keys are bit-identical to those of the same frame with VRT_DEFER_VISIT=0 VRT_TRAV_WINDOW=0 (no
    deferral, no bitmap: every visit compares its key) and with VRT_POOL=0 (one ray per lane); those legs share the
    per-sample colours and stats[:9] too.  (2) compares kernel instances with each other, NOT with the reference: it is
    there because the plain instance is the one the small-scene tests pin to the oracle."""
    import torch
    t0 = time.perf_counter()
    shipped_environment()
    W, H, S, n, cs = C5["width"], C5["height"], C5["samples"], C5["n"], C5["cs"]
    cam, st = c5.cam, c5.st
    r = cam.render(0, want_ray_rgba=True)
    torch.cuda.synchronize()
    report("A", "volume + shipped frame", t0)
    print("[operating points A] stats", r.stats.tolist())
    assert r.stats[8] == C5["rays"] and r.stats[10] == 0 and r.stats[11] == 0
    assert pool_groups(r.stats) > 0
    # the device volume against the reference generator's hash, on z-slabs
    t1 = time.perf_counter()
    host = c5.host_scene()
    x = np.arange(n, dtype=np.uint32)
    for z in (0, 1, 15, 16, 511, 512, 777, 1023):
        lin = x[:, None] + np.uint32(n) * (x[None, :] + np.uint32(n) * np.uint32(z))
        h = ol.murmur_fmix32(lin ^ np.uint32(0x5EED5EED))
        ids = np.where((h & np.uint32(0xFFFF)) >= 1311, 0, 1 + ((h >> np.uint32(16)) % np.uint32(13))).astype(np.uint8)
        assert np.array_equal(host.grid[:, :, z], ids), z
    assert np.array_equal(ol.synth_scene(64, c5.mats).grid, ol.synth64_scene().grid)   # (that IS synth_scene's hash)
    report("A", "volume to the host + slabs", t1)
    # the oracle on every 64th pixel
    t1 = time.perf_counter()
    xs, ys = np.meshgrid(np.arange(0, W, 64), np.arange(0, H, 64), indexing="ij")
    sub = np.stack([xs.ravel(), ys.ravel()], 1).astype(np.int32)
    assert len(sub) == 4096
    n_cells = int(np.prod(r.trav_dims))
    o = ol.render(host, st, c5.pos, c5.rot, cam.lens, sub, libm=ol.LIBM_PORTABLE, threads=16, trav_cap=n_cells)
    report("A", "oracle, %d rays, %d chunks traversed" % (len(o["rays"]), len(o["traversed"])), t1)
    exp = o["rays"]
    assert len(exp) == len(sub) * S == 65536
    assert np.array_equal(r.pixels[:: H][:, 0], np.arange(W)) and np.array_equal(r.pixels[:H, 1], np.arange(H))   # x-major
    rows = torch.from_numpy(sub[:, 0].astype(np.int64) * H + sub[:, 1]).cuda()
    got = r.ray_rgba.view(-1, r.max_samples)[rows].cpu().numpy().view(np.uint32)
    assert r.max_samples == S
    packed = (exp["color"][:, 0] | (exp["color"][:, 1] << 8) | (exp["color"][:, 2] << 16) | (exp["alpha"] << 24)).astype(np.uint32)
    assert np.array_equal(exp["x"].reshape(-1, S)[:, 0], sub[:, 0]) and np.array_equal(exp["s"].reshape(-1, S)[0], np.arange(S))
    assert np.array_equal(got, packed.reshape(-1, S))
    assert np.array_equal(r.rgba_f32[rows].cpu().numpy(), o["pix_mean"].astype(np.float32))
    img = r.image_u8[torch.from_numpy(sub[:, 1].astype(np.int64)).cuda(), torch.from_numpy(sub[:, 0].astype(np.int64)).cuda()]
    assert np.array_equal(img.cpu().numpy(), o["pix_rgba8"])
    # traversed (1): the oracle's chunks are marked
    cells = (o["traversed"] - np.asarray(r.trav_origin, np.int64)) // cs
    assert len(cells) > 32 and (cells >= 0).all() and (cells < np.asarray(r.trav_dims)).all()
    idx = (cells[:, 0] * r.trav_dims[1] + cells[:, 1]) * r.trav_dims[2] + cells[:, 2]
    keys = r.traversed_keys
    assert bool((keys[torch.from_numpy(idx).cuda()] != -1).all())
    # (the box is one the window applies to, and the frame has visits on both sides of it)
    win = bitmap_window(c5.pos, cs, r.trav_origin, r.trav_dims)
    assert win is not None and n_cells > 65536
    visited = torch.nonzero(keys != -1).flatten().cpu().numpy()
    vc = np.stack([visited // (r.trav_dims[1] * r.trav_dims[2]), (visited // r.trav_dims[2]) % r.trav_dims[1], visited % r.trav_dims[2]], 1)
    inside = ((vc >= np.asarray(win)) & (vc < np.asarray(win) + 32)).all(1)
    print("[operating points A] chunks visited: %d inside the window, %d outside" % (int(inside.sum()), int((~inside).sum())))
    assert inside.any() and (~inside).any()
    # traversed (2): instance against instance
    t1 = time.perf_counter()
    for leg in (dict(VRT_DEFER_VISIT=0, VRT_TRAV_WINDOW=0), dict(VRT_POOL=0)):
        with knobs(**leg):
            r2 = cam.render(0, want_ray_rgba=True, want_image=False, want_f32=False)
        assert (pool_groups(r2.stats) > 0) == ("VRT_POOL" not in leg), (leg, r2.stats)
        assert (r2.stats[:9] == r.stats[:9]).all() and r2.stats[10] == 0 and r2.stats[11] == 0, (leg, r2.stats, r.stats)
        assert torch.equal(r2.traversed_keys, keys), leg
        assert torch.equal(r2.ray_rgba, r.ray_rgba), leg
        del r2
    report("A", "plain and lanes legs", t1)
    report("A", "total", t0)


@pytest.mark.parametrize("partition", ["xor", "seed"])
def test_config5_eight_shards_equal_the_single_gpu_frame(c5, partition):
    """BASELINE config 5 on the 8 GPUs it is defined on, here one after the other on one: the 8 shards of
    multigpu.rank_pixels -- the reference's (x ^ y) % 8 and the seed-class partition bench.py uses for N > 1 -- assemble to
    the single-shard frame bit for bit (RGBA8 SHA-256 as bench.py reports it), are disjoint, their event counters and ray
    counts add up to the full frame's, the union of their traversed keys is the full frame's traversed set, and no shard
    reports exhausted draws or visits outside the box.  Default environment."""
    import torch
    from python_raytracer_amd.multigpu import rank_pixels, rank_pixel_counts, merge_traversed
    t0 = time.perf_counter()
    shipped_environment()
    W, H, S = C5["width"], C5["height"], C5["samples"]
    cam = c5.cam
    full = cam.render(0, pixels=rank_pixels(W, H, 1, 0), want_f32=False)
    assert full.stats[8] == C5["rays"] and full.stats[10] == 0 and full.stats[11] == 0
    sha_full = hashlib.sha256(full.image_u8.cpu().numpy().tobytes()).hexdigest()
    image = torch.zeros_like(full.image_u8)
    total = np.zeros(9, np.int64)
    keys = []
    counts = rank_pixel_counts(W, H, 8, partition, S)
    assert counts.sum() == W * H
    for rank in range(8):
        px = rank_pixels(W, H, 8, rank, partition, S)
        assert len(px) == counts[rank]
        r = cam.render(0, pixels=px, want_f32=False)
        assert r.stats[10] == 0 and r.stats[11] == 0
        assert pool_groups(r.stats) > 0                                     # (33.5 M rays: far above the pool's threshold)
        own = torch.from_numpy(px.astype(np.int64)).cuda()
        assert int((image[own[:, 1], own[:, 0]] != 0).sum()) == 0          # shards are disjoint
        image += r.image_u8                                                 # non-owned pixels of a tile are 0
        total += r.stats[:9].astype(np.int64)
        keys.append(r.traversed_keys)
        del r
    assert hashlib.sha256(image.cpu().numpy().tobytes()).hexdigest() == sha_full
    assert np.array_equal(total, full.stats[:9].astype(np.int64))
    merged = merge_traversed(keys)
    assert torch.equal(merged != -1, full.traversed_keys != -1)
    report("B", partition, t0)


# ------------------------------------------------------------------------------------------------- census
CENSUS = [("c2", []), ("c3", []), ("c3_reseed", ["--reseed"]), ("c5", [])]    # committed set's name, bench.py arguments


def _profiled_bench(cfg, extra, out_dir, timeout):
    """One bench.py child under `rocprofv3 --kernel-trace --stats` (the command tools/profile_all.sh profiles, fewer steps);
    returns (exit status, tail of its output, rows of the kernel statistics it wrote)."""
    import glob
    root = pu.ROOT
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", str(out_dir), "--",
           sys.executable, os.path.join(root, "bench.py"), "--full", "--config", cfg.split("_")[0], "--steps", "2", "--warmup", "1",
           "--no-cpu", "--no-context"] + extra
    p = subprocess.Popen(cmd, cwd=root, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, start_new_session=True)
    try:
        out, _ = p.communicate(timeout=timeout)
    except subprocess.TimeoutExpired:
        os.killpg(p.pid, signal.SIGKILL)
        out, _ = p.communicate()
        return 124, out[-3000:], []
    rows = []
    for path in sorted(glob.glob(os.path.join(str(out_dir), "**", "*kernel_stats.csv"), recursive=True)):
        rows += pu.kernel_stats_rows(path)
    return p.returncode, out[-3000:], rows


def test_instances_that_run_are_those_of_the_committed_profiles(tmp_path):
    """Which instantiation of the frame march a configuration runs, observed with the tool the project profiles with:
    `rocprofv3 --kernel-trace --stats` around the bench command of tools/profile_all.sh (2 steps), once each for c2, c3,
    c3 --reseed and c5, strictly one after the other.  The frame-march instances each child ran (full template-argument
    strings) are exactly those of the newest committed profiles/<TAG>_<cfg>_kernel_stats.csv, the dominant one is the
    same, and the re-trace instances appear wherever the committed file has them.  The expected side is the committed
    record of what was measured, not a restatement of launch_march.  Skips only where there is no rocprofv3."""
    if shutil.which("rocprofv3") is None:
        pytest.skip("no rocprofv3 here")
    shipped_environment()
    t0 = time.perf_counter()
    wrong = []
    for cfg, extra in CENSUS:
        t1 = time.perf_counter()
        rc, tail, rows = _profiled_bench(cfg, extra, tmp_path / cfg, timeout=420 if cfg == "c5" else 300)
        assert rc == 0, (cfg, rc, tail)                      # (nothing more is started after a child that failed)
        report("C", "profiled bench.py %s" % cfg, t1)
        want = pu.committed_kernel_stats(cfg)
        got_march, want_march = pu.frame_march_rows(rows), pu.frame_march_rows(want)
        assert want_march, cfg
        got_set, want_set = {pu.instance(r["Name"]) for r in got_march}, {pu.instance(r["Name"]) for r in want_march}
        print("[operating points C] %s ran %s" % (cfg, [(pu.instance(r["Name"]), int(r["Calls"])) for r in got_march]))
        if got_set != want_set:
            wrong.append((cfg, "frame-march instances", sorted(got_set), sorted(want_set)))
        elif pu.instance(got_march[0]["Name"]) != pu.instance(want_march[0]["Name"]):
            wrong.append((cfg, "dominant instance", pu.instance(got_march[0]["Name"]), pu.instance(want_march[0]["Name"])))
        got_re = {pu.instance(r["Name"]) for r in rows if pu.retrace_march(r["Name"])}
        want_re = {pu.instance(r["Name"]) for r in want if pu.retrace_march(r["Name"])}
        if not want_re <= got_re:
            wrong.append((cfg, "re-trace instances", sorted(got_re), sorted(want_re)))
    report("C", "census total", t0)
    assert not wrong, wrong


def test_pool_threshold_at_the_documented_default():
    """pool_plan's documented default (VRT_POOL_MIN_RAYS: launches of 5 Mi rays and more use the ray pool), in-process and
    with the default environment, through stats[12] (march_pool_kernel's workgroups count themselves there): a config 2
    frame (2.07 M rays) runs without pool groups, a full config 3 frame with; one eighth of config 3 by seed classes
    (about 7.8 M rays) with, one sixteenth (about 3.9 M) without.  Results, not only routing: the shards' fp32 means are
    the matching rows of the full config 3 frame, the config 2 frame's are those of the same frame with the pool forced."""
    import torch
    from python_raytracer_amd.multigpu import rank_pixels
    shipped_environment()
    t0 = time.perf_counter()
    floor = 5 << 20
    sc = ol.default_scene()
    st2 = ol.make_settings(width=1920, height=1080, samples=1, max_bounces=4)
    cam2 = camera_for(sc, settings_store(st2), sc.cam_pos, sc.cam_rot, sc.cam_lens)
    r = cam2.render(0)
    assert r.stats[8] == 1920 * 1080 < floor and pool_groups(r.stats) == 0, r.stats
    with knobs(VRT_POOL_MIN_RAYS=0):
        forced = cam2.render(0)
    assert pool_groups(forced.stats) > 0 and torch.equal(forced.rgba_f32, r.rgba_f32) and (forced.stats[:9] == r.stats[:9]).all()
    assert torch.equal(forced.traversed_keys, r.traversed_keys)
    W, H, S = 3840, 2160, 8
    st3 = ol.make_settings(width=W, height=H, samples=S, max_bounces=8)
    cam3 = camera_for(sc, settings_store(st3), sc.cam_pos, sc.cam_rot, sc.cam_lens)
    full = cam3.render(0)
    assert full.stats[8] >= floor and pool_groups(full.stats) > 0, full.stats
    assert np.array_equal(full.pixels[:H, 1], np.arange(H)) and full.pixels[H, 0] == 1     # x-major: row = x * H + y
    for world, pooled in ((8, True), (16, False)):
        for rank in (0, world - 1):
            px = rank_pixels(W, H, world, rank, "seed", S)
            part = cam3.render(0, pixels=px)
            print("[operating points C] 1/%d of config 3, rank %d: %d rays, %d pool groups"
                  % (world, rank, int(part.stats[8]), pool_groups(part.stats)))
            assert (part.stats[8] >= floor) == pooled, (world, rank, part.stats[8])    # (the case is on the side it is meant for)
            assert (pool_groups(part.stats) > 0) == pooled, (world, rank, part.stats)
            rows = torch.from_numpy(px[:, 0].astype(np.int64) * H + px[:, 1]).cuda()
            assert torch.equal(part.rgba_f32, full.rgba_f32[rows]), (world, rank)
    report("C", "pool threshold", t0)


# ------------------------------------------------------------------------------------------------- traversed boxes
BOX_SCENES = {"res2": (1, 2, 139, (1.5, 2.25, -3.5)), "res3": (2, 3, 136, (-2.5, 1.25, 3.5))}   # seed, resolutions, dist_max, camera
# box: lowest cell relative to the camera's cell, cells per side.  The rays of both scenes (oracle, on the CPU) stay within
# [-10, 10] x [-8, 8] x [-2, 17] cells of the camera's: forward is +z, where the cells 16 and 17 ahead lie outside a window
# that is centred on the camera -- so every box but the last two leaves z unclamped and has visits on both sides of it.
BOXES = {
    "unequal-33-40-57": ((-16, -20, -28), (33, 40, 57)),     # window 0 / 4 / 12: x pushed to the low face
    "unequal-64-32-45": ((-32, -16, -22), (64, 32, 45)),     # a side of exactly 32: the window is that whole side
    # the camera's cell as near a corner of the box's x-y section as the rays' back-scatter allows: the window clamps to 0
    # in x and to dims - 32 in y
    "corner": ((-11, -30, -20), (40, 40, 44)),
    "face": ((-11, -17, -20), (35, 35, 40)),                 # the camera in the middle of the low-x face's side of the box
    "side-31": ((-15, -20, -22), (31, 40, 44)),              # below 32 on one side: no window, whatever VRT_TRAV_WINDOW says
    "too-small": ((-16, -20, -20), (33, 40, 34)),            # ends 13 cells ahead of the camera: rays leave it
}
# oracle, per scene: chunks traversed inside / outside the window of the first four boxes; chunks outside "too-small"
BOX_COUNTS = {"res2": (2059, 72, 340), "res3": (2012, 47, 310)}


def _packed_by_slot(r, rays):
    where = {(int(x), int(y)): i for i, (x, y) in enumerate(r.pixels)}
    slot = np.array([where[(int(x), int(y))] for x, y in zip(rays["x"], rays["y"])], np.int64) * r.max_samples + rays["s"]
    packed = (rays["color"][:, 0].astype(np.uint32) | (rays["color"][:, 1].astype(np.uint32) << 8) |
              (rays["color"][:, 2].astype(np.uint32) << 16) | (rays["alpha"].astype(np.uint32) << 24))
    return slot, packed


@pytest.mark.parametrize("box", list(BOXES))
@pytest.mark.parametrize("case", sorted(BOX_SCENES))
def test_caller_supplied_traversed_box(case, box):
    """vrt_render_tile with a traversed box that is NOT Camera._trav_box's camera-centred cube (replaced as
    test_traversed_keys_reset_by_the_call_or_kept_for_the_caller does): unequal sides, the camera near a corner and at a
    face so that the 32^3 settled-bitmap window clamps to 0 on some axes and to dims - 32 on others, a side of 31 (no
    window), and one box that is too small on its far side -- a legal argument: rays leave it, stats[11] counts them.
    Resolutions 1..2 (the kernels with instances that compare a key behind the voxel reads) and 1..3 (the generic ones);
    the ray pool and one ray per lane, forced as tests/test_gpu_parity.py forces them; VRT_TRAV_WINDOW 2, 1, 0 crossed
    with VRT_DEFER_VISIT 2, 0.  For each leg: the traversed list equals the oracle's (restricted to the box), order
    included; stats[:8] equal the oracle's counters; stats[11] is 0, or -- too small -- non-zero and the same in every
    leg; per-sample colours and fp32 means bit-exact (`traversed` never affects a colour); the keys are equal across all
    legs.  That the box holds every ray, where the window lies and that chunks are visited on both sides of it is worked
    out from the oracle's list before anything runs on the GPU."""
    import torch
    from python_raytracer_amd import _native as nat
    t0 = time.perf_counter()
    seed, res_max, dist_max, pos = BOX_SCENES[case]
    cs = 8
    sc = sparse_scene(seed, res_max, cs)
    st = ol.make_settings(width=48, height=36, samples=2, max_bounces=4.0, chunk_size=cs, dist_max=dist_max)
    q, lens = np.array([0.0, 0.0, 0.0, 1.0]), st["fov"] * np.pi / 8
    cam = camera_for(sc, settings_store(st), np.array(pos), q, lens)
    first = cam.render(0)                               # (checked: lets the camera settle its draw-table width)
    o = ol.render(sc, st, np.array(pos), q, lens, first.pixels, libm=ol.LIBM_PORTABLE)
    # the box, the oracle's list inside it, the window
    cc = np.array([int(math.floor(p / cs)) for p in pos])
    lo, dims = (np.array(v) for v in BOXES[box])
    origin = (cc + lo) * cs
    rel = o["traversed"] // cs - cc
    inbox = ((rel >= lo) & (rel < lo + dims)).all(1)
    want_list = o["traversed"][inbox]
    win = bitmap_window(pos, cs, origin, dims)
    n_in, n_out, n_left = BOX_COUNTS[case]
    if box == "too-small":
        assert int((~inbox).sum()) == n_left and inbox.any()
    else:
        assert inbox.all()
    if box == "side-31":
        assert win is None
    else:
        assert win is not None
        inside = window_split(want_list, cs, origin, win)
        if box != "too-small":
            assert (int(inside.sum()), int((~inside).sum())) == (n_in, n_out)
    if box == "corner":
        assert win[0] == 0 and win[1] == dims[1] - 32 and 0 < win[2] < dims[2] - 32
    if box == "face":
        assert win[0] == 0 and 0 < win[1] < dims[1] - 32 and 0 < win[2] < dims[2] - 32

    def supplied(want):
        tr = nat.VrtTraversed()
        if not want:
            return tr, None
        keys = torch.empty(int(dims.prod()), dtype=torch.int64, device="cuda")
        tr.origin[:] = [int(v) for v in origin]
        tr.dims[:] = [int(v) for v in dims]
        tr.reset = 1
        tr.d_keys = keys.data_ptr()
        return tr, keys
    cam._trav_box = supplied
    slot, packed = _packed_by_slot(first, o["rays"])
    all_keys, outside = None, set()
    for kernel in ("pool", "lanes"):
        for window in (2, 1, 0):
            for defer in (2, 0):
                leg = (kernel, window, defer)
                with knobs(VRT_POOL=1 if kernel == "pool" else 0, VRT_POOL_MIN_RAYS=0, VRT_WADDR=0, VRT_TRAV_WINDOW=window,
                           VRT_DEFER_VISIT=defer):
                    r = cam.render(0, want_ray_rgba=True, check=False)     # (unchecked: render() refuses a frame with stats[11])
                    stats = r._stats_dev.cpu().numpy()
                assert r.trav_dims == [int(v) for v in dims]
                assert (pool_groups(stats) > 0) == (kernel == "pool"), (leg, stats)
                assert stats[10] == 0 and stats[13] == 0, (leg, stats)
                assert (stats[:8] == o["counters"]).all() and stats[8] == len(o["rays"]), (leg, stats[:9], o["counters"])
                outside.add(int(stats[11]))
                assert np.array_equal(np.array(r.traversed(cs), np.int64).reshape(-1, 3), want_list), leg
                assert np.array_equal(r.ray_rgba.cpu().numpy().view(np.uint32)[slot], packed), leg
                assert np.array_equal(r.rgba_f32.cpu().numpy(), o["pix_mean"].astype(np.float32)), leg
                if all_keys is None:
                    all_keys = r.traversed_keys.clone()
                assert torch.equal(r.traversed_keys, all_keys), leg
    assert len(outside) == 1, outside                   # the same in the DEFER and the plain legs
    assert (outside.pop() > 0) == (box == "too-small")
    report("D", "%s %s" % (case, box), t0)
