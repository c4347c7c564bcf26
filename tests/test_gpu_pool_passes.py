"""The ray pool's pass logic (march_pool_kernel) where a pass that feeds the march and then marches
(-DVRT_POOL_FUSE, python_raytracer_amd/csrc/vrt_kernels.hip) can go wrong: the policy's extremes, launches that run dry
inside such a pass, both resolution instances, scenes whose HIT passes leave few marchers.  tests/test_gpu_parity.py already
holds every scene against the oracle through the pool kernel; these cases hold whatever schedule the shipped library was
built with, so they pass with the switch off as well as on.

Every case: gpu_util.sparse_scene (6 x 6 x 6 chunks of 8 voxels), 64 x 48 pixels or a list of them, 2-4 samples, the pool
forced (VRT_POOL_MIN_RAYS=0), bit-exact against the oracle through gpu_util.check_frame_march(..., "pool") -- per-sample
colours, fp32 means, stats[:8], the traversed list, and its legs without the settled bitmap, with the bitmap window and
without the cached ray table --, no wave that gave up (stats[13] == 0) and the pool kernel's workgroups counted
(stats[12] > 0)."""
import numpy as np
import pytest

import oracle_lib as ol
from gpu_util import camera_for, check_frame_march, run_children, settings_store, sparse_scene

pytestmark = pytest.mark.gpu

CS = 8
W, H = 64, 48
IDENTITY = np.array([0.0, 0.0, 0.0, 1.0])
# seed, highest resolution, dist_max, camera: the two sparse worlds of test_gpu_parity.py's bitmap-window test (rays fly out
# of the world and on to dist_max; hits, bounces and rays that end are all there)
SCENES = {"res2": (1, 2, 139, (1.5, 2.25, -3.5)), "res3": (2, 3, 136, (-2.5, 1.25, 3.5))}


@pytest.fixture(autouse=True)
def pool_forced(monkeypatch):
    """The pool kernel for launches of any size, without the look-ahead (as test_gpu_parity.py's "pool" leg forces it); read
    at every launch, and inherited by the children of the policy cases."""
    monkeypatch.setenv("VRT_POOL", "1")
    monkeypatch.setenv("VRT_POOL_MIN_RAYS", "0")
    monkeypatch.setenv("VRT_WADDR", "0")


def frame(case, samples=2, n_pixels=None, has_background=True, **settings):
    """One frame of SCENES[case] through march_pool_kernel against the oracle; n_pixels: only that many pixels of the window,
    spread over it in a fixed shuffled order.  Returns the statistics."""
    seed, res_max, dist_max, pos = SCENES[case]
    sc = sparse_scene(seed, res_max, CS)
    assert int(sc.res[sc.present != 0].max()) == res_max
    st = ol.make_settings(width=W, height=H, samples=samples, chunk_size=CS, dist_max=dist_max,
                          **dict({"max_bounces": 4.0}, **settings))
    lens = st["fov"] * np.pi / 8
    cam = camera_for(sc, settings_store(st), np.array(pos), IDENTITY, lens)
    kw = {}
    if n_pixels is not None:
        xs, ys = np.meshgrid(np.arange(W), np.arange(H), indexing="ij")
        every = np.stack([xs.ravel(), ys.ravel()], 1).astype(np.int32)
        kw["pixels"] = np.ascontiguousarray(every[np.random.default_rng(7).permutation(len(every))[:n_pixels]])
        px = kw["pixels"]
    else:
        px = cam.render(0).pixels
    o = ol.render(sc, st, np.array(pos), IDENTITY, lens, px, libm=ol.LIBM_PORTABLE,
                  **({} if has_background else {"has_background": False}))
    assert len(o["rays"]) > 0
    r = check_frame_march(cam, o, CS, "pool", **kw)
    stats = [int(v) for v in r.stats]
    assert stats[8] == len(o["rays"]), (stats[8], len(o["rays"]))
    assert stats[13] == 0, stats          # no wave gave up
    assert stats[12] > 0, stats           # the pool kernel ran
    return stats, o


# ------------------------------------------------------------------------------------------------- the policy's extremes
# pool_policy reads its knobs once per process: one child per setting, one child at a time
POLICIES = {"keep-1": {"VRT_POOL_KEEP": "1"},                                  # every ENDED / HIT pass that may march does
            "keep-64": {"VRT_POOL_KEEP": "64"},                                # almost none does
            "single-rays": {"VRT_POOL_T_END": "1", "VRT_POOL_T_HIT": "1"},     # the slow bodies run for single rays
            "iters-1": {"VRT_POOL_ITERS": "1"},
            "defaults": {}}


def _policy_child():
    stats, o = frame("res2")
    stats3, o3 = frame("res3")
    print("POOLPASS", stats[8], stats[12], stats[13], stats3[8], stats3[12], stats3[13])


@pytest.mark.parametrize("policy", list(POLICIES))
def test_policy_extremes(policy):
    """Both worlds under a setting of the pass policy that drives the fused passes to an end of their range: the frame is
    the oracle's whatever the schedule (asserted in the child, which fails otherwise), no wave stalls, the pool ran."""
    words = run_children("import test_gpu_pool_passes as t; t._policy_child()", [POLICIES[policy]], "POOLPASS")[0]
    rays2, groups2, stalled2, rays3, groups3, stalled3 = (int(w) for w in words[1:])
    assert rays2 > 0 and rays3 > 0 and groups2 > 0 and groups3 > 0 and stalled2 == 0 and stalled3 == 0, words


# ------------------------------------------------------------------------------------------------- launches that run dry
@pytest.mark.parametrize("n_pixels", [1, 31, 33, 257])
def test_launch_runs_dry_inside_a_pass(n_pixels):
    """Pixel lists of 1, 31, 33 and 257 pixels at 2 samples (up to 2, 62, 66 and 514 rays): fewer rays than a wave's 64
    lanes, about the lanes, and more than one hand-out -- the refill of an ENDED pass finds the launch empty, or finds it empty half way, and the pass that
    follows it must neither count as a stall nor march a lane that got no ray."""
    stats, o = frame("res2", n_pixels=n_pixels)
    assert n_pixels <= stats[8] <= 2 * n_pixels     # (lod_edge takes the second sample off some pixels)


# ------------------------------------------------------------------------------------------------- both resolution instances
@pytest.mark.parametrize("case", sorted(SCENES))
def test_both_resolution_instances(case):
    """Resolutions 1..2 (march_pool_kernel<8, 1, ..>) and 1..3 (<4, 2, ..>) at 4 samples: 12 288 rays, 48 waves' worth, so
    that pools fill and every kind of pass runs many times."""
    stats, o = frame(case, samples=4)
    assert stats[4] > 0 and stats[6] > 0       # voxels were hit, rays advanced


# ------------------------------------------------------------------------------------------------- few marchers after HIT
def test_no_background():
    """Without a background (init.py:119) the rays that leave the world keep their colour un-energised: the ENDED body's
    other arm, in passes that now may march afterwards."""
    from python_raytracer_amd import data
    try:
        data.background = None
        stats, o = frame("res2", has_background=False)
    finally:
        data.background = data.material_background
    assert stats[4] > 0


def test_one_bounce():
    """max_bounces = 1: every ray ends at its first hit, so a HIT pass leaves no lane that marches on -- fewer than any
    P.pool_keep -- and the ENDED passes that follow refill whole waves."""
    stats, o = frame("res3", samples=3, max_bounces=1.0)
    assert stats[4] > 0
