"""The per-chunk object lists and both voxelisers at their limits, on the GPU, against brute force (inputs, references and reach
conditions: tests/chunk_lists_limits.py, held to the triple loop and to owner_ref by tests/test_chunk_lists_limits_host.py).

A. vrt_chunk_lists_build alone on raw box records: chunk counts around every edge of lists_scan_kernel (four counts per thread,
   256 per wave, 4096 per iteration and its 64-bit carry into the next), object counts around the 64-lane ballot word, overflow
   beyond one iteration, the chunk box at +-2^30.
B. vrt_voxelize_lists and vrt_voxelize against build_world at every chunk size from 8 to 256 (1 to 32 bricks per axis).
C. vrt_hit_owners_lists and vrt_hit_owners asked about every filled voxel, the lower chunk faces, empty cells and records that are
   no hits, against World.owner; lists of another chunk size than the scene's; a lists box over half the world.
Every expected value is exact.  Nothing here can fault by design: every call is inside the contract of include/vrt.h or is
refused before any HIP call."""
import ctypes as C
import types

import numpy as np
import pytest

import chunk_lists_limits as cl
from python_raytracer_amd import _native as nat, make_settings
from python_raytracer_amd.scene import unpack_blocks
from python_raytracer_amd.world import DeviceWorld, chunk_object_lists
from test_gpu_chunk_lists import Abi, same_owners, same_world
from test_gpu_owners import OWNER_WORDS, same, world_camera

pytestmark = pytest.mark.gpu
OFFSETS_PATTERN, ITEMS_PATTERN = 0x5a5a5a5a, -77


# ---- A. the build alone --------------------------------------------------------------------------------------------------------
def upload(array):
    import torch
    return torch.from_numpy(np.ascontiguousarray(array)).cuda()


class Build:
    """vrt_chunk_lists_build over a device array of object records (a uint8 tensor, or None for no objects) for ANY chunk box,
    into buffers filled with a pattern (`room`: items they hold if not `cap`) -- or into those of an earlier Build (`into`)."""

    def __init__(self, d_objects, n_objects, origin, dims, cs, cap, into=None, room=None):
        import torch
        n = int(np.prod(np.asarray(dims, np.int64)))
        if into is None:
            self.offsets = torch.full((n + 1,), OFFSETS_PATTERN, dtype=torch.int32, device="cuda")
            self.items = torch.full((max(cap if room is None else room, 1),), ITEMS_PATTERN, dtype=torch.int32, device="cuda")
        else:
            self.offsets, self.items = into.offsets, into.items
        self.d_objects = d_objects
        stats = torch.full((nat.NSTATS,), -1, dtype=torch.int64, device="cuda")
        self.lists = nat.VrtChunkLists()
        self.lists.origin[:] = [int(v) for v in origin]
        self.lists.dims[:] = [int(v) for v in dims]
        self.lists.chunk_size, self.lists.n_items_cap = int(cs), int(cap)
        self.lists.d_offsets, self.lists.d_items = self.offsets.data_ptr(), self.items.data_ptr()
        self.rc = nat.lib().vrt_chunk_lists_build(d_objects.data_ptr() if n_objects else None, n_objects, C.byref(self.lists), stats.data_ptr(),
                                                  torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        self.stats = stats.cpu().numpy()

    def numpy(self):
        return self.offsets.cpu().numpy().view(np.uint32), self.items.cpu().numpy()


def build_of(c, cap, **buffers):
    return Build(upload(cl.object_records(c["boxes"])) if len(c["boxes"]) else None, len(c["boxes"]), c["origin"], c["dims"], c["cs"], cap, **buffers)


# The 32-bit wrap of an offset in lists_scan_kernel (its running total is 64 bits wide, the stored word 32) needs lists of more
# than 2^32 items: out of reach of a test, and untested.
@pytest.mark.parametrize("name", list(cl.BUILD_CASES))
def test_build_equals_the_host_lists(name):
    """Offsets and items byte for byte, the statistics words, at every chunk and object count of BUILD_CASES."""
    cl.build_reach(name)
    c = cl.build_case(name)
    n, need = c["n_chunks"], len(c["items"])
    if name == "c12293":
        assert n > 3 * cl.SCAN_SPAN
    counts = np.diff(c["offsets"].astype(np.int64))
    if len(c["boxes"]):
        assert all(counts[base:base + cl.SCAN_SPAN].any() for base in range(0, n, cl.SCAN_SPAN)) and counts[-1] > 0
    got = build_of(c, need)
    assert got.rc == 0
    off, items = got.numpy()
    assert off.tobytes() == c["offsets"].tobytes()
    assert items[:need].tobytes() == c["items"].tobytes() and (items[need:] == ITEMS_PATTERN).all()
    assert int(got.stats[nat.S_LISTS_ITEMS]) == need and int(got.stats[nat.S_LISTS_OVERFLOW]) == 0
    assert (np.delete(got.stats, [nat.S_LISTS_ITEMS]) == 0).all()
    if len(c["boxes"]) == 0:
        assert not off.any() and len(off) == n + 1


@pytest.mark.parametrize("short", ["one", "all"])
def test_overflow_beyond_one_iteration_of_the_scan(short):
    """8193 chunks, a capacity one item short of the need and a capacity of none: the needed total and the flag, the sentinel, no
    item written; then the same buffers with room for all: the full lists, and nothing of the sentinel."""
    c = cl.build_case(cl.OVERFLOW_CASE)
    n, need = c["n_chunks"], len(c["items"])
    assert n > 2 * cl.SCAN_SPAN
    small = build_of(c, need - 1 if short == "one" else 0, room=need)
    assert small.rc == 0
    off, items = small.numpy()
    assert off[-1] == nat.LISTS_SENTINEL and len(items) == need and (items == ITEMS_PATTERN).all()
    assert int(small.stats[nat.S_LISTS_ITEMS]) == need and int(small.stats[nat.S_LISTS_OVERFLOW]) == 1
    assert (np.delete(small.stats, [nat.S_LISTS_ITEMS, nat.S_LISTS_OVERFLOW]) == 0).all()
    full = build_of(c, need, into=small)
    off, items = full.numpy()
    assert full.rc == 0 and off.tobytes() == c["offsets"].tobytes() and items.tobytes() == c["items"].tobytes()
    assert int(full.stats[nat.S_LISTS_ITEMS]) == need and int(full.stats[nat.S_LISTS_OVERFLOW]) == 0


def test_one_chunk_beyond_the_coordinate_limits_is_refused():
    """lo30 and hi30 (accepted: test_build_equals_the_host_lists) moved one chunk further out: VRT_ERR_ARG, offsets untouched."""
    boxes = cl.build_case("lo30")["boxes"]
    for origin, dims, cs in cl.REFUSED_BOXES.values():
        got = Build(upload(cl.object_records(boxes)), len(boxes), origin, dims, cs, 1000)
        off, items = got.numpy()
        assert got.rc == -1 and (off == OFFSETS_PATTERN).all() and (items == ITEMS_PATTERN).all() and (got.stats == -1).all()


# ---- B. both voxelisers against build_world ------------------------------------------------------------------------------------
_twins = {}


def twins(cs):
    """(world with lists, world without, their PackedScenes) over the world of chunk size cs, built once."""
    if cs not in _twins:
        objs = cl.world_case(cs)["objs"]
        a, b = DeviceWorld(cs, lists=True), DeviceWorld(cs, lists=False)
        _twins[cs] = (a, b, a.build(objs), b.build(objs))
        assert a.list_calls == {"build": 1, "voxelize": 1, "owners": 0} and b.list_calls == {"build": 0, "voxelize": 0, "owners": 0}
    return _twins[cs]


@pytest.mark.parametrize("cs", cl.SMALL_CS + cl.BIG_CS)
def test_both_voxelisers_equal_build_world(cs):
    """The dense grid, the chunks present, the table words and the material order, by lists and by the scan."""
    c = cl.world_reach(cs)
    w, objs = c["w"], c["objs"]
    assert cs // 8 == {8: 1, 16: 2, 32: 4, 64: 8, 128: 16, 256: 32}[cs]
    a, b, psa, psb = twins(cs)
    dims = [int(v) for v in w.dims]
    n = np.arange(int(np.prod(dims)), dtype=np.uint32).reshape(dims) + 1
    for dw, ps in ((a, psa), (b, psb)):
        assert np.array_equal(dw.origin, w.origin) and np.array_equal(dw.dims, w.dims) and list(dw.order) == objs
        assert [id(m) for m in dw.materials] == [id(m) for m in w.materials]
        table = ps.device_tensors["chunk_table"].cpu().numpy().view(np.uint32).reshape(dims)
        blocks = unpack_blocks(ps.device_tensors["voxels"].cpu().numpy().reshape(-1, cs ** 3), cs)
        grid = blocks.reshape(dims[0], dims[1], dims[2], cs, cs, cs).transpose(0, 3, 1, 4, 2, 5).reshape(dims[0] * cs, dims[1] * cs, dims[2] * cs)
        assert np.array_equal(grid, w.grid)
        assert np.array_equal((table != 0).astype(np.uint8), w.present)
        assert np.array_equal(table[table != 0], (n | (1 << 24))[table != 0])
    assert same_world(a, b)
    off, items = a.chunk_lists().numpy()
    assert np.array_equal(off, c["offsets"]) and np.array_equal(items, c["items"])
    if cs in cl.SMALL_CS:
        assert int(np.diff(off.astype(np.int64)).max()) > cl.TILE


# ---- C. the owner passes asked about every voxel -------------------------------------------------------------------------------
_asked = {}


def asked(cs):
    """dict(cam, hits, abi, scan): the camera over the scan world's scene (every chunk at resolution 1), the host-made records
    on the device, the entry points over the scan world's records, and vrt_hit_owners' answer (records, statistics)."""
    if cs not in _asked:
        a, b, psa, psb = twins(cs)
        st = make_settings(width=32, height=24, samples=1, dist_max=96, chunk_lod=0, chunk_size=cs)
        st.culling = False
        cam = world_camera(st, psb, (0.0, 0.0, -30.0))
        table, world = (t.cpu().numpy().view(np.uint32) for t in (cam._camera_table, b._table))
        assert np.array_equal(table != 0, world != 0) and (table != 0).sum() > 4 and (table[table != 0] >> 24 == 1).all()   # resolution 1
        r = cl.owner_records(cs)
        hits = types.SimpleNamespace(records=upload(np.frombuffer(r["hits"].tobytes(), np.uint8).copy()))
        abi = Abi(b)
        _asked[cs] = dict(cam=cam, hits=hits, abi=abi, scan=abi.owners(False, hits, cam), st=st)
    return _asked[cs]


def check_owner_stats(stats, examined, resolved, orphans):
    assert int(stats[nat.S_OWNER_EXAMINED]) == examined and int(stats[nat.S_OWNER_RESOLVED]) == resolved, stats
    assert int(stats[nat.S_OWNER_ORPHANS]) == orphans and int(stats[nat.S_OWNER_AMBIGUOUS]) == 0, stats
    assert (np.delete(stats, OWNER_WORDS) == 0).all(), stats


@pytest.mark.parametrize("cs", cl.SMALL_CS)
def test_owner_passes_on_every_voxel(cs):
    """Every record's object, resolution, voxel and local index, and the statistics, by the lists and by the scan, through the
    entry points and through DeviceWorld.owners, against World.owner and _rotate_index."""
    c, r = cl.records_reach(cs)
    a, b, psa, psb = twins(cs)
    g = asked(cs)
    objs, expect = c["objs"], r["expect"]
    assert list(a.order) == objs == list(b.order)                          # (World.owner's index is the index into `order`)
    for axis in range(3):
        assert ((r["kind"] == 1) & (r["face"] == 1 << axis)).any()
    cam_a = world_camera(g["st"], psa, (0.0, 0.0, -30.0))
    res_a, res_b = a.owners(g["hits"].records, cam_a), b.owners(g["hits"].records, g["cam"])
    assert a.list_calls["owners"] >= 1 and b.list_calls["owners"] == 0 and same_owners(res_a, res_b)
    for rec, stats in (g["abi"].owners(True, g["hits"], g["cam"]), g["scan"], (res_a.numpy(), res_a.stats), (res_b.numpy(), res_b.stats)):
        for f in ("object", "resolution", "voxel", "local"):
            assert np.array_equal(rec[f], expect[f]), f
        assert same(rec, expect)
        check_owner_stats(stats, r["examined"], r["resolved"], r["orphans"])
        own = rec["object"] >= 0
        assert (rec["resolution"][own] == 1).all() and np.array_equal(rec["voxel"][own], r["hits"]["cell"][own])
        got = cl.model_materials(objs, b.materials, rec["object"][own], rec["local"][own].astype(np.int64))
        assert np.array_equal(got, r["hits"]["material"][own])
        assert 0 in rec["object"] and len(objs) - 1 in rec["object"]


def test_lists_of_another_chunk_size_than_the_scenes():
    """The scene at chunk size 16, the lists over its box rounded outward to multiples of 32, at chunk sizes 8, 16 and 32: the
    owner pass keeps the lists' chunk size apart from the scene's, and the records and statistics are the scan's."""
    cs = 16
    c, r = cl.records_reach(cs)
    g = asked(cs)
    b = twins(cs)[1]
    abi = g["abi"]
    own = abi.lists
    lo, hi = cl.rounded_box(cs, 32)
    assert (lo < np.asarray(b.origin)).any()
    try:
        for to in (8, 32, 16):
            dims = (hi - lo) // to
            made = Build(b._objects_dev, abi.n_obj, lo, dims, to, len(chunk_object_lists(c["boxes"], lo, dims, to)[1]))
            exp_off, exp_items = chunk_object_lists(c["boxes"], lo, dims, to)
            off, items = made.numpy()
            assert made.rc == 0 and np.array_equal(off, exp_off) and np.array_equal(items, exp_items)
            abi.lists = made.lists
            rec, stats = abi.owners(True, g["hits"], g["cam"])
            assert same(rec, g["scan"][0]) and np.array_equal(stats, g["scan"][1]), to
            assert same(rec, r["expect"])
    finally:
        abi.lists = own


@pytest.mark.parametrize("cs", cl.SMALL_CS)
def test_lists_over_half_the_world(cs):
    """The lists' box ends at x = 0, the object records are all of them: a record whose voxel lies inside the box is the scan's
    -- also where its owner's box leaves the lists' box -- and one outside is an orphan, counted."""
    c, r = cl.records_reach(cs)
    g = asked(cs)
    b = twins(cs)[1]
    abi = g["abi"]
    origin, dims = cl.half_box(cs)
    exp_off, exp_items = chunk_object_lists(c["boxes"], origin, dims, cs)
    made = Build(b._objects_dev, abi.n_obj, origin, dims, cs, len(exp_items))
    off, items = made.numpy()
    assert made.rc == 0 and np.array_equal(off, exp_off) and np.array_equal(items, exp_items)
    scan_rec, scan_stats = g["scan"]
    owned = scan_rec["object"] >= 0
    lost = owned & ~cl.in_box(r["hits"]["cell"].astype(np.int64), origin, dims, cs)
    assert 100 < lost.sum() < owned.sum() - 500
    expect = scan_rec.copy()
    expect[lost] = np.zeros((), expect.dtype)
    expect["object"][lost] = -2
    own = abi.lists
    try:
        abi.lists = made.lists
        rec, stats = abi.owners(True, g["hits"], g["cam"])
    finally:
        abi.lists = own
    assert same(rec, expect)
    check_owner_stats(stats, r["examined"], r["resolved"] - int(lost.sum()), r["orphans"] + int(lost.sum()))
    bx = c["boxes"]
    across = np.flatnonzero((bx[:, 0, 0] < 0) & (bx[:, 1, 0] > 0))
    assert len(across) >= 1 and np.isin(rec["object"][rec["object"] >= 0], across).any()
