"""CPU-only: the host rules every Camera entry point shares, each through the one function that states it -- the velocity
bound and the traversed box, the check of a frame's or a batch's statistics, pose records and their range, the coercion of
ray arguments, the traversed list of a key box, and the result classes' views.  No test here touches a device:
Camera(settings=...) constructs without one, and the helpers that allocate do so on the device they are given.

The numbers in BOUNDS, BOXES and BATCH were recorded once from Camera._velocity_bound, Camera._trav_box and render_views' own
radius loop as they were before these rules were gathered (each camera's `rot` and `pos` set, the method called)."""
import math

import numpy as np
import pytest
import torch

from python_raytracer_amd import Camera, CastResult, HitResult, OwnerResult, ShadeResult, make_settings
from python_raytracer_amd import _native as nat
from python_raytracer_amd import camera as cm
from python_raytracer_amd.lib import quaternion, vec3
from python_raytracer_amd.results import _traversed_positions

CPU = torch.device("cpu")
H = math.sqrt(0.5)
# rotation (x, y, z, w): the velocity bound, the box radius in cells for chunk_size 8 and 16 (dist_max 192)
BOUNDS = [
    ((0, 0, 0, 1), 1.0, 26, 14),                                  # identity
    ((0, 0, 0, 0), 1.0, 26, 14),                                  # the reference's initial quaternion
    ((H, 0, 0, H), 3.000000000000001, 75, 39),                    # a quarter turn about x: the reference's product is no rotation
    ((0, H, 0, H), 1.0000000000000009, 26, 14),                   # ... about y
    ((0, 0, 1, 0), 1.0, 26, 14),                                  # a half turn about z
    ((0.65, -0.26, 0.78, 0.754), 5.573221983684192, 139, 72),     # norm 1.29
    ((999.0, -500.0, 250.0, 125.0), 4775251.058878944, 117590559, 59989093),   # near the 1e3 a pose may have
]
# camera position, rotation: origin of _trav_box's box for chunk_size 8, dist_max 192; its dims are 2 r + 1 each
BOXES = [
    ((0, 0, 0), (0, 0, 0, 1), [-208, -208, -208], 53),
    ((0, 0, 0), (H, 0, 0, H), [-600, -600, -600], 151),
    ((-13.5, -8.0, -0.25), (0, 0, 0, 1), [-224, -216, -216], 53),           # negative, no multiple of chunk_size
    ((-13.5, -8.0, -0.25), (H, 0, 0, H), [-616, -608, -608], 151),
    ((7.999, 15.999999, 8.0), (0, 0, 0, 1), [-208, -200, -200], 53),        # just below a chunk border, and on one
    ((7.999, 15.999999, 8.0), (H, 0, 0, H), [-600, -592, -592], 151),
]
# three poses of one batch: radii 26, 75, 26 -> every view 151 cells a side, around its own chunk
BATCH = [((0.3, 0.6, -10.45), (0, 0, 0, 1)), ((1.5, -2.5, 3.0), (H, 0, 0, H)), ((-100.0, 7.0, 64.0), (0.0, 0.6, 0.0, 0.8))]
BATCH_ORIGINS = [[-600, -600, -616], [-600, -608, -600], [-704, -600, -536]]


def camera(**kw):
    cam = Camera(settings=make_settings(**dict(dict(chunk_size=8, dist_max=192), **kw)))
    cam._device = CPU   # (what the helpers allocate, they allocate here: on a machine with a GPU too)
    return cam


# ---- velocity bound, box radius, box geometry ----------------------------------------------------------------------------
@pytest.mark.parametrize("rot,bound,r8,r16", BOUNDS)
def test_velocity_bound_and_box_radius(rot, bound, r8, r16):
    """The bound is the square of a 4 x 4 matrix's largest singular value, which LAPACK gives to a few units in the last
    place, not the same ones on every host: 1e-13 relative is some 450 of them.  The radii are integers, and none of them
    is nearer than 1e-2 cells to the next (201 * 5.5732 / 16 = 70.014 is the closest)."""
    for cs, r in ((8, r8), (16, r16)):
        cam = camera(chunk_size=cs)
        pos, own = cam.pos, cam.rot
        assert cam._velocity_bound(rot) == pytest.approx(bound, rel=1e-13, abs=0) and cam._box_radius(rot) == r
        assert cam.pos is pos and cam.rot is own            # an explicit rotation leaves the camera alone
        cam.rot = quaternion(*[float(v) for v in rot])      # ... and is the bound of a camera that has it
        assert cam._velocity_bound() == cam._velocity_bound(rot) and cam._box_radius() == r


@pytest.mark.parametrize("pos,rot,origin,n", BOXES)
def test_box_around_the_camera(pos, rot, origin, n):
    cam = camera()
    cam.pos, cam.rot = vec3(*pos), quaternion(*[float(v) for v in rot])
    assert cam._box_around(pos, cam._box_radius()) == (origin, [n, n, n])
    tr, keys = cam._trav_box(True)
    assert (list(tr.origin), list(tr.dims), tr.reset) == (origin, [n, n, n], 1)
    assert keys.dtype == torch.int64 and keys.numel() == n ** 3 and tr.d_keys == keys.data_ptr()


def test_no_box_and_a_callers_keys():
    cam = camera()
    tr, keys = cam._trav_box(False)
    assert (list(tr.origin), list(tr.dims), tr.reset, tr.d_keys, keys) == ([0, 0, 0], [0, 0, 0], 0, None, None)
    mine = torch.full((24,), -1, dtype=torch.int64)
    tr, keys = cam._key_box([8, -16, 0], [2, 3, 4], mine)   # the caller's keys are used as they are: no reset
    assert keys is mine and (list(tr.origin), list(tr.dims), tr.reset, tr.d_keys) == ([8, -16, 0], [2, 3, 4], 0, mine.data_ptr())


def test_batch_boxes_share_the_largest_radius():
    cam = camera()
    pos, rot = cam.pos, cam.rot
    rec = Camera._pose_records(BATCH, cam.lens)
    assert [cam._box_radius(q) for q in rec[:, 3:7]] == [26, 75, 26]
    assert cam._view_boxes(rec) == (BATCH_ORIGINS, [151, 151, 151])
    assert cam._view_boxes(rec[:1]) == ([[-208, -208, -224]], [53, 53, 53])    # alone, a view has _trav_box's own box
    assert cam.pos is pos and cam.rot is rot
    with pytest.raises(nat.VrtError, match=r"would need 1 x \d+\^3 cells"):
        cam._view_boxes(Camera._pose_records([((0, 0, 0), BOUNDS[-1][0])], cam.lens))


# ---- the statistics check -------------------------------------------------------------------------------------------------
def stats(**words):
    a = np.zeros(nat.NSTATS, np.int64)
    a[:8] = np.arange(8) + 3          # event sums: no part of the check
    for k, v in words.items():
        a[getattr(nat, "S_" + k)] = v
    return a


# name: the words, then what the check says with 32 draws and with 64, for a frame and for a batch -- (retry, draws64), or
# the words its VrtError must contain
NO, SWITCH, RETRY = (False, False), (False, True), (True, True)
STATS = {
    "clean": (dict(RAYS=1000), NO, NO, NO, NO),
    "exhausted": (dict(RAYS=1000, RNG_EXHAUSTED=5), RETRY, "5 rays could not be completed", RETRY,
                  "5 rays of the batch could not be completed"),
    "exhausted and outside: the retry comes first": (dict(RAYS=1000, RNG_EXHAUSTED=1, TRAV_OUTSIDE=9), RETRY, "1 rays could not",
                                                     RETRY, "1 rays of the batch"),
    "stalled": (dict(RAYS=1000, STALLED=3), "3 waves of the march found nothing to run", "3 waves of the march", NO, NO),
    "outside": (dict(RAYS=1000, TRAV_OUTSIDE=2), "2 chunk visits fell outside the traversed box ", "outside the traversed box ",
                "2 chunk visits fell outside the traversed boxes ", "outside the traversed boxes "),
    "re-traced, 2 % of the rays": (dict(RAYS=1000, RNG_RETRACED=20), NO, NO, NO, NO),
    "re-traced, one ray more": (dict(RAYS=1000, RNG_RETRACED=21), SWITCH, NO, SWITCH, NO),
    "no rays, none re-traced": (dict(), NO, NO, NO, NO),
    "no rays, one re-traced": (dict(RNG_RETRACED=1), SWITCH, NO, SWITCH, NO),
}


@pytest.mark.parametrize("what", ["frame", "batch"])
@pytest.mark.parametrize("name", list(STATS))
def test_statistics_check(name, what):
    words = STATS[name][0]
    for draws, want in zip((32, 64), STATS[name][1:3] if what == "frame" else STATS[name][3:5]):
        if isinstance(want, str):
            with pytest.raises(nat.VrtError) as e:
                cm._check_stats(stats(**words), draws, what)
            assert want in str(e.value)
            if "RNG_EXHAUSTED" in words:
                assert cm._EXHAUSTED_RULE % what in str(e.value)
        else:
            assert cm._check_stats(stats(**words), draws, what) == want


# ---- pose records and their range ----------------------------------------------------------------------------------------
def test_pose_records_from_pairs_arrays_and_records():
    lens = 35.34291735288517
    want = np.array([list(p) + list(q) + [lens] for p, q in BATCH], np.float64)
    pairs = Camera._pose_records(BATCH, lens)
    vecs = Camera._pose_records([(vec3(*p), quaternion(*[float(v) for v in q])) for p, q in BATCH], lens)
    wide7 = Camera._pose_records(want[:, :7].copy(), lens)
    wide8 = Camera._pose_records(want.copy(), lens)
    for got in (pairs, vecs, wide7, wide8):
        assert got.dtype == np.float64 and np.array_equal(got, want)
    camera()._check_pose_range(want, make_settings(chunk_size=8, dist_max=192))


def test_pose_records_refused():
    cam = camera()
    s, lens = cam._settings(), cam.lens
    good = Camera._pose_records(BATCH, lens)
    wrong_lens = good.copy()
    wrong_lens[1, 7] *= 1.5
    with pytest.raises(ValueError, match="lens"):
        Camera._pose_records(wrong_lens, lens)
    with pytest.raises(ValueError, match="at least one pose"):
        Camera._pose_records([], lens)
    with pytest.raises(ValueError, match=r"\[V, 7\] array"):
        Camera._pose_records(good[:, :6].copy(), lens)
    for col, value, words in ((1, float("nan"), "not finite"), (0, float("inf"), "not finite"), (4, 1e3 + 1, "exceeds 1e3"),
                              (2, float(1 << 28), "outside the range")):
        bad = good.copy()
        bad[2, col] = value
        with pytest.raises(ValueError, match=words):
            cam._check_pose_range(bad, s)
    edge = good.copy()
    edge[2, 3:7] = [1e3, 0, 0, 0]
    with pytest.raises(ValueError, match="outside the range"):     # 1e3 itself passes the rotation rule: its reach does not
        cam._check_pose_range(edge, s)


# ---- coercion of ray arguments ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("value", [[[1, 2, 3], [4.5, 5, 6]], np.array([[1, 2, 3], [4.5, 5, 6]], np.float32),
                                   np.array([[1, 2, 3], [4, 5, 6]], np.int16), torch.tensor([[1, 2, 3], [4.5, 5, 6]], dtype=torch.float32)])
def test_floats_accepted(value):
    got = cm._floats(value, "origins", "cast_rays", ("n", 3), CPU)
    assert got.dtype == torch.float64 and got.device == CPU and list(got.shape) == [2, 3]
    assert np.array_equal(got.numpy(), np.asarray(value, np.float64))


def test_floats_refused():
    for bad, words in ((np.array([[True, False, True]]), "cast_rays: origins must be numbers, not bool"),
                       (np.array([["a", "b", "c"]]), "cast_rays: origins must be numbers, not <U1"),
                       (torch.zeros((4, 2), dtype=torch.float64), "cast_rays: origins must have shape [n, 3], not [4, 2]"),
                       (torch.zeros((4, 3), dtype=torch.int64), "cast_rays: origins must be floating point, not torch.int64")):
        with pytest.raises(ValueError) as e:
            cm._floats(bad, "origins", "cast_rays", ("n", 3), CPU)
        assert str(e.value) == words
    with pytest.raises(ValueError) as e:
        cm._floats(np.zeros((5, 31)), "draws", "shade_rays", (5, 32), CPU)
    assert str(e.value) == "shade_rays: draws must have shape [5, 32], not [5, 31]"
    with pytest.raises(ValueError) as e:
        cm._floats(np.zeros((4, 31)), "draws", "shade_rays", (5, "n_draws"), CPU)
    assert str(e.value) == "shade_rays: draws must have shape [5, n_draws], not [4, 31]"
    assert list(cm._floats(np.zeros((5, 31)), "draws", "shade_rays", (5, "n_draws"), CPU).shape) == [5, 31]


def test_cast_records_from_arrays():
    cam = camera()
    o, v = [[0, 0, 0], [1, 2, 3]], np.array([[1, 0, 0], [0, -1, 0.5]], np.float32)
    rec = cam._cast_records(o, v, None, 190.0)
    assert rec.dtype == torch.float64 and np.array_equal(rec.numpy(), [[0, 0, 0, 1, 0, 0, 190, 0], [1, 2, 3, 0, -1, 0.5, 190, 0]])
    rec = cam._cast_records(o, v, torch.tensor([7, 9]), 190.0, "shade_rays")      # lives: any numbers, converted
    assert np.array_equal(rec.numpy()[:, 6], [7.0, 9.0])
    with pytest.raises(ValueError) as e:
        cam._cast_records(o, v, [1.0, 2.0, 3.0], 190.0, "shade_rays")
    assert str(e.value) == "shade_rays: lives must have shape [2], not [3]"
    with pytest.raises(ValueError) as e:
        cam._cast_records(o, torch.zeros((2, 3), dtype=torch.int32), None, 190.0)
    assert str(e.value) == "cast_rays: velocities must be floating point, not torch.int32"
    with pytest.raises(ValueError) as e:
        cam._cast_records(o, np.zeros((3, 3)), None, 190.0)
    assert str(e.value) == "cast_rays: 2 origins but 3 velocities"


def test_seeds():
    got = cm._seeds([3, 0, (1 << 63) - 1], 3, "shade_rays", CPU)
    assert got.dtype == torch.int64 and got.is_contiguous() and got.tolist() == [3, 0, (1 << 63) - 1]
    assert cm._seeds(torch.arange(8, dtype=torch.int32)[::2], 4, "shade_rays", CPU).is_contiguous()
    for bad in ([1, -1, 2], np.array([0, 1 << 63, 2], np.uint64), [1.0, 2.0, 3.0]):
        with pytest.raises(ValueError) as e:
            cm._seeds(bad, 3, "shade_rays", CPU)
        assert str(e.value) == "shade_rays: seeds must be integers in [0, 2**63)"
    with pytest.raises(ValueError) as e:
        cm._seeds(torch.zeros(3, dtype=torch.float32), 3, "shade_rays", CPU)
    assert str(e.value) == "shade_rays: seeds must be integers, not torch.float32"
    with pytest.raises(ValueError) as e:
        cm._seeds([1, 2], 3, "shade_rays", CPU)
    assert str(e.value) == "shade_rays: seeds must have shape [3], not [2]"


def test_max_life():
    assert cm._max_life(None, 192, "cast_rays") == 192.0
    assert cm._max_life(1 << 28, 192, "cast_rays") == float(1 << 28)
    for bad in (0, float("nan"), (1 << 28) + 1):
        with pytest.raises(ValueError) as e:
            cm._max_life(bad, 192, "shade_rays")
        assert str(e.value) == "shade_rays: max_life must lie in (0, 2**28], not %r" % float(bad)


# ---- the traversed list of a key box -----------------------------------------------------------------------------------------
def test_traversed_positions_in_key_order():
    dims, origin, cs = [2, 3, 2], [-8, 0, 16], 8
    keys = torch.full((12,), -1, dtype=torch.int64)
    keys[1], keys[6], keys[11] = 50, 7, 20           # cells (0, 0, 1), (1, 0, 0), (1, 2, 1): visited second-to-last, first, then
    want = [(0.0, 0.0, 16.0), (0.0, 16.0, 24.0), (-8.0, 0.0, 24.0)]
    assert _traversed_positions(keys, origin, dims, cs) == want
    assert _traversed_positions(torch.full((12,), -1, dtype=torch.int64), origin, dims, cs) == []
    assert _traversed_positions(None, None, None, cs) == []
    res = ShadeResult(None, None, None, (keys, origin, dims))
    assert res.traversed(cs) == want and ShadeResult(None, None, None).traversed(cs) == []


# ---- result classes ------------------------------------------------------------------------------------------------------------
def test_hit_and_cast_results_share_their_views():
    rec = np.zeros(3, np.dtype(nat.HIT_FIELDS))
    rec["step"] = [1.5, 200.0, 0.0]
    rec["pos"] = [[1, 2, 3.5], [-4, 5, 6], [0, 0, 0]]
    rec["cell"] = [[1, 2, 3], [-4, 5, 6], [0, 0, 0]]
    rec["material"] = [7, 0, nat.HIT_REJECTED]
    buf = torch.from_numpy(rec.view(np.uint8).copy())
    block = torch.arange(nat.NSTATS, dtype=torch.int64)
    cast = CastResult(buf, block)
    hit = HitResult(buf, np.array([[0, 0], [1, 0], [2, 0]], np.int32), 1, 1, 1, 3, block)
    for name in ("step", "pos", "cell", "material"):
        assert torch.equal(getattr(cast, name), getattr(hit, name)) and getattr(cast, name).data_ptr() == getattr(hit, name).data_ptr()
        assert np.array_equal(getattr(cast, name).numpy(), rec[name])
    assert np.array_equal(cast.numpy(), rec) and np.array_equal(hit.numpy(), rec)
    assert cast.hit_mask().tolist() == [True, False, False] and cast.rejected_mask().tolist() == [False, False, True]
    assert hit.material_image().tolist() == [[7, 0, -2]] and hit.depth_image().tolist() == [[1.5, float("inf"), float("inf")]]


def test_stats_are_copied_once():
    block = torch.arange(nat.NSTATS, dtype=torch.int64)
    buf = torch.zeros(nat.HIT_BYTES, dtype=torch.uint8)
    for res in (CastResult(buf, block), HitResult(buf, np.zeros((1, 2), np.int32), 1, 1, 1, 1, block),
                ShadeResult(None, None, block), OwnerResult(torch.zeros(nat.OWNER_BYTES, dtype=torch.uint8), 0, block)):
        assert res._stats_dev is block
        first = res.stats
        assert isinstance(first, np.ndarray) and first.dtype == np.int64 and first.tolist() == list(range(nat.NSTATS))
        assert res.stats is first
