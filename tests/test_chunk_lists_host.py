"""Per-chunk object lists on the host (python_raytracer_amd.world.chunk_object_lists / chunk_object_total, the host statement
of vrt_chunk_lists_build's rule): against a brute-force triple loop, against the reference's own record of which object every
voxel came from, and the equality argument of the list-driven voxelisation executed with build_world.  Then the new translation
unit's compiler report, its symbols and the arguments its entry points refuse before any HIP call."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import chunk_lists_report
import kernel_report
import oracle_lib as ol
from python_raytracer_amd import _native as nat
from python_raytracer_amd.lib import vec3
from python_raytracer_amd.world import DeviceWorld, build_world, chunk_object_lists, chunk_object_total
from test_world import _redraw_sequence, build_from_fixture, build_from_random_fixture, random_fixture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def brute_lists(boxes, origin, dims, cs):
    """The rule, chunk by chunk and object by object: object k is in the list of chunk c iff its half-open box is not empty
    and overlaps the chunk's half-open box on all three axes."""
    offsets, items = [0], []
    for cx in range(dims[0]):
        for cy in range(dims[1]):
            for cz in range(dims[2]):
                lo = [origin[0] + cx * cs, origin[1] + cy * cs, origin[2] + cz * cs]
                for k, (mn, mx) in enumerate(boxes):
                    if all(mn[a] < mx[a] and mn[a] < lo[a] + cs and mx[a] > lo[a] for a in range(3)):
                        items.append(k)
                offsets.append(len(items))
    return np.array(offsets, np.uint32), np.array(items, np.int32)


def check(boxes, origin, dims, cs):
    boxes = np.asarray(boxes, np.int64).reshape(-1, 2, 3)
    off, items = chunk_object_lists(boxes, origin, dims, cs)
    exp_off, exp_items = brute_lists(boxes.tolist(), list(origin), list(dims), cs)
    assert off.dtype == np.uint32 and items.dtype == np.int32
    assert np.array_equal(off, exp_off) and np.array_equal(items, exp_items)
    assert chunk_object_total(boxes, origin, dims, cs) == len(items) == int(off[-1])
    return off, items


# ---- 1. the rule against a triple loop ---------------------------------------------------------------------------------------
def test_boxes_on_chunk_faces():
    """[0, 16) touches one chunk and [0, 17) touches two: the classic off-by-one, on every axis and at the lower face too."""
    off, items = check([[[0, 0, 0], [16, 16, 16]]], [0, 0, 0], [2, 2, 2], 16)
    assert off.tolist() == [0, 1, 1, 1, 1, 1, 1, 1, 1] and items.tolist() == [0]
    for axis in range(3):
        mx = [16, 16, 16]
        mx[axis] = 17
        off, items = check([[[0, 0, 0], mx]], [0, 0, 0], [2, 2, 2], 16)
        assert len(items) == 2
        mn = [16, 16, 16]
        mn[axis] = 15
        off, items = check([[mn, [32, 32, 32]]], [0, 0, 0], [2, 2, 2], 16)
        assert len(items) == 2


@pytest.mark.parametrize("cs", [8, 16, 32])
def test_random_boxes_against_brute_force(cs):
    rng = np.random.default_rng(cs)
    origin, dims = np.array([-2 * cs, -cs, 0]), np.array([4, 3, 2])
    hi = origin + dims * cs
    boxes = []
    for _ in range(60):
        mn = rng.integers(origin - cs, hi + cs // 2, 3)                 # negative coordinates, partly or wholly outside
        boxes.append([mn, mn + rng.integers(1, 2 * cs + 2, 3)])
    for _ in range(20):                                                   # faces exactly on chunk faces
        mn = origin + rng.integers(0, dims, 3) * cs
        boxes.append([mn, mn + rng.integers(1, 3, 3) * cs])
    boxes.append([[0, 0, 0], [0, 5, 5]])                                  # empty boxes: mins == maxs, and inverted
    boxes.append([[3, 3, 3], [9, 2, 9]])
    boxes.append([origin - 5, hi + 5])                                    # covers the whole world
    boxes.append([hi + 1, hi + 9])                                        # wholly outside
    boxes = np.array(boxes, np.int64)
    order = rng.permutation(len(boxes))
    off, items = check(boxes[order], origin, dims, cs)
    whole = int(np.flatnonzero(order == len(boxes) - 2)[0])
    n = int(dims.prod())
    for c in range(n):
        row = items[off[c]:off[c + 1]]
        assert whole in row.tolist() and (np.diff(row) > 0).all()         # ascending k: the merge order
    for k in np.flatnonzero(order >= len(boxes) - 4):
        if order[k] != len(boxes) - 2:
            assert int(k) not in items.tolist()                           # the empty ones and the outside one are in no list


def test_no_objects_and_objects_as_input():
    off, items = check(np.zeros((0, 2, 3)), [0, 0, 0], [2, 1, 3], 16)
    assert off.tolist() == [0] * 7 and len(items) == 0
    z = np.load(os.path.join(ol.GOLDEN, "world_build.npz"))
    mats, st, objs = build_from_fixture(z)
    vis = [o for o in objs if o.visible]
    w = build_world(vis, 16)
    boxes = [[[o.mins.x, o.mins.y, o.mins.z], [o.maxs.x, o.maxs.y, o.maxs.z]] for o in vis]
    a, b = chunk_object_lists(vis, w.origin, w.dims, 16), chunk_object_lists(boxes, w.origin, w.dims, 16)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and len(a[1]) >= len(vis)
    assert chunk_object_total(vis, w.origin, w.dims, 16) == len(a[1])


# ---- 2. the reference's own record -------------------------------------------------------------------------------------------
def listed(off, items, c, k):
    return k in items[off[c]:off[c + 1]].tolist()


def owners_are_listed(owner, owner_origin, order_spec, boxes, cs):
    """Every voxel's recorded object (an index into the fixture's spec list) is in the list of that voxel's chunk.  The lists
    are a SUPERSET of the reference's chunks_objects dict, which names only the chunks in which the object has a voxel; the
    record shows the dict's members, so containment is what can be asserted."""
    origin = np.asarray(owner_origin, np.int64)
    dims = np.array(owner.shape) // cs
    off, items = chunk_object_lists(boxes, origin, dims, cs)
    to_list = {spec: k for k, spec in enumerate(order_spec)}
    at = np.argwhere(owner >= 0)
    chunk = ((at[:, 0] // cs) * dims[1] + at[:, 1] // cs) * dims[2] + at[:, 2] // cs
    pairs = {(int(c), int(s)) for c, s in zip(chunk, owner[owner >= 0])}
    assert len(pairs) > 0
    for c, spec in pairs:
        assert listed(off, items, c, to_list[spec]), (c, spec)
    return len(pairs), len(items)


def test_reference_owners_are_in_their_chunks_lists():
    z = random_fixture()
    mats, st, objs = build_from_random_fixture(z)
    vis = [k for k, o in enumerate(objs) if o.visible]
    boxes = [[z["obj_mins"][k], z["obj_maxs"][k]] for k in vis]
    assert z["owner"].shape[0] % 16 == 0
    pairs, total = owners_are_listed(z["owner"], z["origin"], vis, boxes, 16)
    assert pairs >= 63 and total >= pairs                                  # (a superset: boxes reach chunks their voxels do not)


def test_reference_owner_ticks_are_in_their_chunks_lists():
    z = np.load(os.path.join(ol.GOLDEN, "world_build.npz"))
    seq = np.load(os.path.join(ol.GOLDEN, "world_update.npz"))
    own = np.load(os.path.join(ol.GOLDEN, "world_owners.npz"))
    mats, st, objs = build_from_fixture(z)
    cam_pos = vec3(*[float(v) for v in z["cam_pos"]])
    vis = [o for o in objs if o.visible]
    order = list(vis)
    owners_are_listed(own["owner_0"], seq["origin_0"], [objs.index(o) for o in order], order, 16)
    for tag, changed in _redraw_sequence(objs, st, cam_pos, seq):
        stay, moved = DeviceWorld.merge_order(order, vis, changed)
        order = stay + moved
        owners_are_listed(own["owner_" + tag], seq["origin_" + tag], [objs.index(o) for o in order], order, 16)


# ---- 3. the equality argument, executed --------------------------------------------------------------------------------------
def test_build_world_per_chunk_from_the_listed_objects_only():
    """Every chunk of build_world's grid equals that chunk of a world built from the chunk's listed objects alone, in list
    order: an object outside the list cannot supply a voxel of the chunk, and the list keeps the merge order."""
    z = random_fixture()
    mats, st, objs = build_from_random_fixture(z)
    vis = [o for o in objs if o.visible]
    w = build_world(vis, 16, owners=True)
    off, items = chunk_object_lists(vis, w.origin, w.dims, 16)
    assert int(np.diff(off.astype(np.int64)).max()) < len(vis)              # (no chunk lists everything: the restriction is real)
    checked = 0
    for c in range(int(np.prod(w.dims))):
        cell = np.array(np.unravel_index(c, tuple(int(d) for d in w.dims)))
        lo = cell * 16
        want = w.grid[lo[0]:lo[0] + 16, lo[1]:lo[1] + 16, lo[2]:lo[2] + 16]
        sub = [vis[int(k)] for k in items[off[c]:off[c + 1]]]
        if not sub:
            assert not want.any()
            continue
        part = build_world(sub, 16, owners=True)
        ids = np.array([0] + [1 + [id(m) for m in w.materials].index(id(m)) for m in part.materials], np.uint8)
        p = w.origin + lo - part.origin                                    # the chunk inside the partial world's box, if it reaches it
        got = np.zeros((16, 16, 16), np.uint8)
        if (p >= 0).all() and (p + 16 <= part.grid.shape).all():
            got = ids[part.grid[p[0]:p[0] + 16, p[1]:p[1] + 16, p[2]:p[2] + 16]]
        assert np.array_equal(got, want), c
        checked += bool(want.any())
    assert checked >= 10


# ---- 4. the translation unit: report, symbols, refusals ----------------------------------------------------------------------
def test_chunk_lists_report_is_the_saved_one():
    if not os.path.exists(kernel_report.HIPCC):
        pytest.skip("no hipcc")
    fresh = kernel_report.parse(chunk_lists_report.compile_report())
    saved = chunk_lists_report.saved()
    assert list(fresh) == list(saved) and fresh == saved
    assert len(fresh) == 6        # the wave pass twice (count, fill), the scan, the two consumers, the statistics clear
    for name, fig in fresh.items():
        assert fig["VGPRs Spill"] == 0 and fig["ScratchSize [bytes/lane]"] == 0, (name, fig)   # no vector spills, no scratch
        assert fig["VGPRs"] <= 64, (name, fig)                         # eight waves per SIMD
    vox = [f for n, f in fresh.items() if "voxelize_lists_kernel" in n]
    assert len(vox) == 1 and 128 * 64 <= vox[0]["LDS Size [bytes/block]"] <= 128 * 64 + 512   # one tile of 128 records


def test_symbols_build_and_header():
    text = open(os.path.join(ROOT, "include", "vrt.h")).read()
    L = nat.lib()
    for name in ("vrt_chunk_lists_build", "vrt_voxelize_lists", "vrt_hit_owners_lists"):
        assert name in nat.EXPORTS and getattr(L, name) is not None and re.search(r"\bint %s\(" % name, text)
    assert L.vrt_abi_version() == 9 and nat.ABI_VERSION == 9 and "#define VRT_ABI_VERSION 9" in text   # the change only adds
    assert re.search(r"VRT_S_LISTS_ITEMS = 8\b", text) and re.search(r"VRT_S_LISTS_OVERFLOW = 9\b", text)
    assert (nat.S_LISTS_ITEMS, nat.S_LISTS_OVERFLOW) == (8, 9) and C.sizeof(nat.VrtChunkLists) == 64
    assert [os.path.basename(u) for u in nat.CHUNK_LISTS_UNITS] == ["vrt_chunk_lists.hip"] and set(nat.CHUNK_LISTS_UNITS) <= set(nat.SOURCES)
    assert not set(nat.CHUNK_LISTS_UNITS) & set(nat.UNITS + nat.PHYSICS_UNITS + nat.PHYSICS_DRAWS_UNITS + nat.PHYSICS_RUN_UNITS +
                                                nat.PHYSICS_ANIM_UNITS + nat.PHYSICS_RUN_DRAWS_UNITS)
    assert "csrc/vrt_chunk_lists.hip" in open(os.path.join(ROOT, "tools", "build_variant.sh")).read()
    src = open(nat.CHUNK_LISTS_UNITS[0]).read()
    for helper in ("voxel_offset", "rotate_index", "owner_probe", "owner_snap", "owner_candidate"):
        assert re.search(r"\b%s\(" % helper, src)
    assert "originals are in vrt_kernels.hip" in src
    import python_raytracer_amd
    assert python_raytracer_amd.ChunkLists is not None and "ChunkLists" in python_raytracer_amd.__all__
    assert DeviceWorld.LISTS_MIN >= 1


def lists_struct(**change):
    v = dict(origin=(0, 0, 0), dims=(2, 2, 2), chunk_size=16, n_items_cap=64, d_offsets=0x1000, d_items=0x2000)
    v.update(change)
    s = nat.VrtChunkLists()
    s.origin[:], s.dims[:] = v["origin"], v["dims"]
    s.chunk_size, s.n_items_cap, s.d_offsets, s.d_items = v["chunk_size"], v["n_items_cap"], v["d_offsets"], v["d_items"]
    return s


BAD_LISTS = [dict(chunk_size=0), dict(chunk_size=12), dict(chunk_size=4), dict(chunk_size=512), dict(dims=(0, 2, 2)), dict(dims=(2, -1, 2)),
             dict(dims=(256, 256, 256)), dict(origin=(8, 0, 0)), dict(origin=(1 << 31, 0, 0)), dict(n_items_cap=-1),
             dict(n_items_cap=1 << 31), dict(d_offsets=None), dict(d_items=None), dict(d_offsets=0x1002)]


def test_entry_points_refuse_bad_arguments_without_a_device():
    """Everything the three entry points can refuse is refused before their first HIP call: these calls carry made-up device
    pointers, which nothing reads."""
    L = nat.lib()
    fake = 0x1000

    def build(objects=fake, n=4, lists=lists_struct(), stats=fake):
        return L.vrt_chunk_lists_build(objects, n, C.byref(lists) if lists is not None else None, stats, None)

    assert build(lists=None) == -1 and build(stats=None) == -1 and build(stats=fake + 4) == -1
    assert build(n=-1) == -1 and build(objects=None) == -1 and build(objects=fake + 8) == -1
    for bad in BAD_LISTS:
        assert build(lists=lists_struct(**bad)) == -1, bad
    assert build(n=0, objects=None, lists=lists_struct(n_items_cap=0, d_items=None, chunk_size=3)) == -1

    o64, d32 = (C.c_int64 * 3)(0, 0, 0), (C.c_int32 * 3)(2, 2, 2)

    def voxelize(objects=fake, n=4, models=fake, remap=fake, origin=o64, dims=d32, cs=16, chunk_list=None, n_list=0, table=fake, voxels=fake,
                 lists=lists_struct()):
        return L.vrt_voxelize_lists(objects, n, models, remap, origin, dims, cs, chunk_list, n_list, table, voxels,
                                    C.byref(lists) if lists is not None else None, None)

    # vrt_voxelize's refusals
    assert voxelize(n=-1) == -1 and voxelize(origin=None) == -1 and voxelize(dims=None) == -1 and voxelize(table=None) == -1
    assert voxelize(voxels=None) == -1 and voxelize(objects=None) == -1 and voxelize(models=None) == -1 and voxelize(remap=None) == -1
    assert voxelize(cs=12) == -1 and voxelize(n_list=3) == -1 and voxelize(n_list=-1) == -1 and voxelize(chunk_list=fake, n_list=9) == -1
    # ... the lists', and lists of another box or chunk size
    assert voxelize(lists=None) == -1 and voxelize(voxels=fake + 4) == -1 and voxelize(objects=fake + 8) == -1
    for bad in BAD_LISTS:
        assert voxelize(lists=lists_struct(**bad)) == -1, bad
    assert voxelize(lists=lists_struct(dims=(2, 2, 1))) == -1 and voxelize(lists=lists_struct(origin=(16, 0, 0))) == -1
    assert voxelize(lists=lists_struct(chunk_size=8)) == -1
    assert voxelize(chunk_list=fake, n_list=0) == 0                        # nothing to rebuild: no launch

    sc = nat.VrtScene()
    sc.origin[:], sc.dims[:] = (0, 0, 0), (2, 2, 2)
    sc.chunk_size, sc.n_slots, sc.d_chunk_table, sc.d_voxels = 16, 8, fake, fake

    def owners(scene=sc, hits=fake, n=8, objects=fake, n_obj=4, models=fake, remap=fake, out=fake, lists=lists_struct(), stats=fake):
        return L.vrt_hit_owners_lists(C.byref(scene) if scene is not None else None, hits, n, objects, n_obj, models, remap, out,
                                      C.byref(lists) if lists is not None else None, stats, None)

    assert owners(scene=None) == -1 and owners(stats=None) == -1 and owners(n=-1) == -1 and owners(n=1 << 32) == -1 and owners(n_obj=-1) == -1
    assert owners(hits=None) == -1 and owners(out=None) == -1 and owners(hits=fake + 4) == -1 and owners(out=fake + 8) == -1
    assert owners(objects=None) == -1 and owners(models=None) == -1 and owners(remap=None) == -1 and owners(objects=fake + 8) == -1
    assert owners(lists=None) == -1
    for bad in BAD_LISTS:
        assert owners(lists=lists_struct(**bad)) == -1, bad
