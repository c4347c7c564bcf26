"""Inputs and references for the limits of the per-chunk object lists and of both voxelisers (tests/test_chunk_lists_limits_host.py
on the CPU, tests/test_gpu_chunk_lists_limits.py on the GPU).  Nothing here touches a device: every expected value is computed
exactly on the host, from world.chunk_object_lists and world.build_world, and every REACH CONDITION -- the property of an input
that makes its case the case it is meant to be -- is a function of the inputs alone, so the CPU suite evaluates all of them and a
GPU run cannot lose a case silently.

A. BUILD_CASES: raw box records for vrt_chunk_lists_build, by chunk count around the scan's four-per-thread, one-wave and
   4096-per-iteration edges, by object count around the 64-object ballot word, and at the +-2^30 limits of the chunk box.
B. small_world / big_world: worlds for both voxelisers at every chunk size from 8 to 256.
C. owner_records: hit records made on the host -- every filled voxel, the lower chunk faces, empty cells, records that are no
   hits -- with the owner records the pass must return for them."""
import numpy as np

from python_raytracer_amd import _native as nat
from python_raytracer_amd.world import _rotate_index, build_world, chunk_object_lists

SCAN_SPAN = 4096   # counts lists_scan_kernel sums per iteration: 1024 threads x 4
TILE = 128         # object records voxelize_lists_kernel stages in LDS at a time

OBJECT_DTYPE = np.dtype([("mins", "<i4", 3), ("maxs", "<i4", 3), ("size", "<i4", 3), ("turns", "<i4", 3), ("model", "<i8"),
                         ("remap", "<i4"), ("pad", "<i4")])
assert OBJECT_DTYPE.itemsize == 64


# ---- A. raw boxes for the build ----------------------------------------------------------------------------------------------
# name: (origin, dims, chunk size, objects).  Non-cubic dims, negative origins; the chunk counts and why:
BUILD_CASES = {
    "c1": ((-8, 0, 8), (1, 1, 1), 8, 200),
    "c4": ((0, -16, 0), (4, 1, 1), 8, 200),                   # one thread's four counts, exactly ...
    "c5": ((-40, 0, 0), (5, 1, 1), 8, 200),                   # ... and one into the next thread
    "c255": ((-8, 8, -40), (3, 5, 17), 8, 200),               # one wave of the scan: 64 threads x 4 = 256 counts
    "c256": ((0, 0, -64), (2, 8, 16), 8, 200),
    "c257": ((16, -800, 0), (1, 257, 1), 8, 200),
    "c4095": ((-64, 0, 0), (15, 13, 21), 8, 200),             # the first iteration of the scan, exactly and one over
    "c4096": ((-64, -64, -64), (16, 16, 16), 8, 200),
    "c4097": ((-72, 8, -1000), (17, 1, 241), 8, 200),
    "c8191": ((0, 0, -32000), (1, 1, 8191), 8, 200),          # the second iteration
    "c8192": ((-8, -128, 0), (16, 32, 16), 8, 200),
    "c8193": ((-16, 0, -8000), (3, 1, 2731), 8, 200),
    "c12293": ((-80, 8, -2400), (19, 1, 647), 8, 200),        # above 3 x 4096, no multiple of 4: three carries
    # +-2^30: the lowest origin and the highest top lists_view accepts, at the largest chunk size
    "lo30": ((-(1 << 30), 0, -256), (3, 2, 2), 256, 200),
    "hi30": (((1 << 30) - 3 * 256, -512, (1 << 30) - 2 * 256), (3, 2, 2), 256, 200),
}
# object counts around the 64-lane ballot word (an exact multiple of 64 is where `k < n_objects` decides), over the 4097-chunk box
for _n in (0, 1, 63, 64, 65, 127, 128, 192, 1000):
    BUILD_CASES["n%d" % _n] = BUILD_CASES["c4097"][:3] + (_n,)
OVERFLOW_CASE = "c8193"
# one chunk further out than lo30 / hi30: refused before any HIP call
REFUSED_BOXES = {"below": ((-(1 << 30) - 256, 0, -256), (3, 2, 2), 256), "above": (((1 << 30) - 3 * 256, -512, (1 << 30) - 2 * 256), (4, 2, 2), 256)}

_PATTERN = ["small", "span", "straddle", "outside", "small", "touch", "empty", "span", "inverted", "straddle", "small", "outside", "touch"]


def make_boxes(origin, dims, cs, n, seed):
    """int64 [n, 2, 3] (mins, maxs): three boxes that cover the whole chunk box (first, middle, last: every chunk's count is
    non-zero whatever n >= 1 is), one box at the int32 extremes, and a repeating mix of small boxes, boxes over many chunks, boxes
    across the edge of the chunk box, boxes outside it, boxes that touch its outermost faces from inside and from outside, empty
    boxes (mins == maxs on an axis) and inverted ones (mins > maxs) that lie inside the chunk box."""
    rng = np.random.default_rng(seed)
    lo = np.asarray(origin, np.int64)
    hi = lo + np.asarray(dims, np.int64) * cs
    wholes = sorted({0, n // 2, n - 1})
    out, touches = [], 0
    for i in range(n):
        if i in wholes:
            pad = (0, 1, cs + 3)[wholes.index(i)]
            out.append([lo - pad, hi + pad])
            continue
        if i == 1:
            out.append([np.full(3, -(1 << 31)), np.full(3, (1 << 31) - 1)])
            continue
        kind = _PATTERN[i % len(_PATTERN)]
        mn = rng.integers(lo, hi)
        mx = mn + rng.integers(1, cs + 1, 3)
        a = int(rng.integers(0, 3))
        low = bool(rng.integers(0, 2))
        if kind == "span":
            mx = mn + rng.integers(1, np.maximum((hi - lo) // 2, 2) + 1)
        elif kind == "straddle":
            if low:
                mn[a], mx[a] = lo[a] - rng.integers(1, cs), lo[a] + rng.integers(1, 2 * cs)
            else:
                mn[a], mx[a] = hi[a] - rng.integers(1, 2 * cs), hi[a] + rng.integers(1, cs)
        elif kind == "outside":
            if low:
                mx[a] = lo[a] - rng.integers(0, 20)
                mn[a] = mx[a] - rng.integers(1, cs)
            else:
                mn[a] = hi[a] + rng.integers(0, 20)
                mx[a] = mn[a] + rng.integers(1, cs)
        elif kind == "touch":
            a = (touches // 4) % 3
            mn[a], mx[a] = [(hi[a] - 1, hi[a]), (hi[a], hi[a] + 1), (lo[a], lo[a] + 1), (lo[a] - 1, lo[a])][touches % 4]
            touches += 1
        elif kind == "empty":
            mx[a] = mn[a]
        elif kind == "inverted":   # (both ends inside the chunk box: only the emptiness test keeps it out of the lists)
            mn[a], mx[a] = mx[a], mn[a]
        out.append([mn, mx])
    boxes = np.asarray(out, np.int64).reshape(-1, 2, 3)
    assert (boxes >= -(1 << 31)).all() and (boxes < (1 << 31)).all()
    return boxes


def object_records(boxes):
    """uint8 array of 64-byte vrt_object records with these boxes.  The build reads mins and maxs only: every other field holds
    a pattern that is no valid size, turn or offset."""
    rec = np.zeros(len(boxes), OBJECT_DTYPE)
    rec["mins"], rec["maxs"] = boxes[:, 0], boxes[:, 1]
    rec["size"], rec["turns"], rec["model"], rec["remap"], rec["pad"] = -0x01010102, 0x7e7e7e7e, -1, -7, 0x55555555
    return rec.view(np.uint8).reshape(-1)


_build = {}


def build_case(name):
    """dict(origin, dims, cs, n_chunks, boxes, offsets, items) of BUILD_CASES[name]: the boxes and the host's lists, made once."""
    if name not in _build:
        origin, dims, cs, n = BUILD_CASES[name]
        boxes = make_boxes(origin, dims, cs, n, seed=sorted(BUILD_CASES).index(name))
        off, items = chunk_object_lists(boxes, origin, dims, cs)
        for a in (boxes, off, items):
            a.setflags(write=False)
        _build[name] = dict(origin=origin, dims=dims, cs=cs, n_chunks=int(np.prod(np.asarray(dims, np.int64))), boxes=boxes, offsets=off, items=items)
    return _build[name]


def build_reach(name):
    """The reach conditions of a build case, asserted: the chunk count the name states, a non-empty list in every block of 4096
    chunks (every iteration of the scan carries something) and a non-empty LAST list (offsets[n_chunks] differs from the offset
    before it: it is the scan's own word)."""
    c = build_case(name)
    n, off = c["n_chunks"], c["offsets"].astype(np.int64)
    if name[0] == "c":
        assert n == int(name[1:])
    if name == "c12293":
        assert n > 3 * SCAN_SPAN and n % 4
    if name[0] == "n":
        assert len(c["boxes"]) == int(name[1:]) and n == 4097
    assert len(off) == n + 1 and off[-1] == len(c["items"])
    if len(c["boxes"]) == 0:
        assert not off.any()
        return
    counts = np.diff(off)
    for base in range(0, n, SCAN_SPAN):
        assert counts[base:base + SCAN_SPAN].any()
    assert counts[-1] > 0 and (counts > 0).all()
    if len(c["boxes"]) >= 100:   # the mix is there: lists differ from chunk to chunk unless the box is a single chunk
        assert n == 1 or len(set(counts.tolist())) > 1
        b = c["boxes"]
        assert ((b[:, 1] == b[:, 0]).any(1)).any() and ((b[:, 1] < b[:, 0]).any(1)).any()
        assert (b[:, 0] == -(1 << 31)).all(1).any() and (b[:, 1] == (1 << 31) - 1).all(1).any()


# ---- B. worlds for both voxelisers ---------------------------------------------------------------------------------------------
SMALL_CS = (8, 16, 32, 64)
BIG_CS = (128, 256)


def slab(pos, rot, rng, size):
    """A non-cubic visible object: only the quarter turns between its two equal extents apply."""
    from python_raytracer_amd.lib import vec3
    from python_raytracer_amd.world import Object, Sprite
    from test_gpu_chunk_lists import mats
    spr = Sprite(size=vec3(*size), frames=1, lod=0)
    vox = {p: mats()[int(rng.integers(0, 4))] for p in np.ndindex(*size) if rng.random() < 0.7}
    vox[(0, 0, 0)] = mats()[1]
    spr.get_frame(0).set_voxels(vox, True)
    ob = Object(pos=vec3(*[int(v) for v in pos]), rot=vec3(*rot), sprite=spr)
    ob.visible = True
    return ob


def small_world(cs):
    """151 objects of edge 2 to 6 over the chunk box [-2 cs, 2 cs) x [-cs, cs) x [0, 2 cs) -- 4 x 2 x 2 chunks:
    132 inside the one chunk [-cs, 0) x [-cs, 0) x [0, cs), 100 of them crowded into 8^3 voxels around its centre (across its brick
    faces from chunk size 16 on) and 32 anywhere in it; 14 anywhere in the box; one cube in the lowest and one in the highest
    corner, first and last of the array; one cube around the chunk corner (0, 0, cs), which meets eight chunks and lies across
    x = 0, where the half box of the owner tests ends; two non-cubic models with turns that apply and turns that do not."""
    from test_gpu_chunk_lists import tiny
    rng = np.random.default_rng(40 + cs)
    lo, hi = np.array([-2 * cs, -cs, 0]), np.array([2 * cs, cs, 2 * cs])
    k0 = np.array([-cs, -cs, 0])
    b = cs // 2 - 4

    def within(rl, rh):
        e = int(rng.choice([2, 4, 6]))
        return tiny(rng.integers(rl + e // 2, rh - e // 2 + 1), rng, e)

    crowd = [within(k0 + b, k0 + b + 8) for _ in range(100)] + [within(k0, k0 + cs) for _ in range(32)]
    spread = [within(lo, hi - 1) for _ in range(14)]
    first, last = tiny(lo + 1, rng, 2), tiny(hi - 2, rng, 2)
    corner = tiny((0, 0, cs), rng, 4)
    slabs = [slab((-cs - 3, -5, cs + 3), (0, 0, 90), rng, (4, 4, 2)), slab((cs + 5, 3, 5), (90, 270, 180), rng, (2, 4, 4))]
    return [first] + spread[:7] + [corner, slabs[0]] + crowd + [slabs[1]] + spread[7:] + [last]


BIG_BRICKS = {"slab": (5, 6, 1), "b123": (1, 2, 3)}   # (and the last brick, (nb - 1,) * 3)


def big_world(cs):
    """Five objects in 2 x 1 x 1 chunks from x = -cs on: a cube across the shared face x = 0; a cube in the LAST brick of the
    lower chunk (local coordinates cs - 6 .. cs - 3 on every axis); a slab with a turn in its brick (5, 6, 1); a cube inside
    brick (1, 2, 3) of the upper chunk, and a larger one over it.  The three brick positions differ from each other on every
    axis: no swap of two axes in a brick decode maps the set onto itself."""
    from test_gpu_chunk_lists import tiny
    rng = np.random.default_rng(90 + cs)
    return [tiny((0, 20, 20), rng, 4), tiny((-4, cs - 4, cs - 4), rng, 4), slab((-cs + 44, 52, 12), (0, 0, 90), rng, (4, 4, 2)),
            tiny((12, 20, 28), rng, 4), tiny((14, 22, 28), rng, 6)]


_worlds = {}


def boxes_of(objs):
    return np.array([[[int(o.mins.x), int(o.mins.y), int(o.mins.z)], [int(o.maxs.x), int(o.maxs.y), int(o.maxs.z)]] for o in objs], np.int64)


def world_case(cs, owners=True):
    """dict(objs, boxes, w, offsets, items) for chunk size cs: the objects, the host world (with its owner grid if `owners`) and
    the host lists over its chunk box.  Made once, never changed."""
    key = (cs, owners)
    if key not in _worlds:
        objs = small_world(cs) if cs in SMALL_CS else big_world(cs)
        w = build_world(objs, cs, owners=owners)
        boxes = boxes_of(objs)
        off, items = chunk_object_lists(boxes, w.origin, w.dims, cs)
        for a in (w.grid, w.owner, w.present, boxes, off, items):
            if a is not None:
                a.setflags(write=False)
        _worlds[key] = dict(objs=objs, boxes=boxes, w=w, offsets=off, items=items)
    return _worlds[key]


def local_bricks(w):
    """Set of (bx, by, bz): the bricks, by their position INSIDE their chunk, in which the world holds a voxel."""
    at = np.argwhere(w.grid != 0)
    return {tuple(v) for v in np.unique((at % w.chunk_size) // 8, axis=0).tolist()}


def world_bricks(w):
    """... by their position in the whole chunk box."""
    return {tuple(v) for v in np.unique(np.argwhere(w.grid != 0) // 8, axis=0).tolist()}


def three_apart(bricks):
    """Three of `bricks` that differ from each other on every axis, or None."""
    bricks = sorted(bricks)
    for i, p in enumerate(bricks):
        for j in range(i + 1, len(bricks)):
            q = bricks[j]
            if any(x == y for x, y in zip(p, q)):
                continue
            for r in bricks[j + 1:]:
                if all(x != z and y != z for x, y, z in zip(p, q, r)):
                    return p, q, r
    return None


def world_reach(cs):
    """The reach conditions of a world of section B, asserted; returns the case."""
    c = world_case(cs)
    w, objs, nb = c["w"], c["objs"], cs // 8
    counts = np.diff(c["offsets"].astype(np.int64))
    assert nb == {8: 1, 16: 2, 32: 4, 64: 8, 128: 16, 256: 32}[cs]
    if cs in SMALL_CS:
        assert len(objs) == 151 and w.origin.tolist() == [-2 * cs, -cs, 0] and w.dims.tolist() == [4, 2, 2]
        assert counts.max() > TILE                                           # two LDS tiles of the voxeliser
        assert int(np.argmax(counts)) == (1 * 2 + 0) * 2 + 0                 # ... in the chunk [-cs, 0) x [-cs, 0) x [0, cs)
        corner = 8
        assert objs[corner].mins.tuple() == (-2, -2, cs - 2) and (c["items"] == corner).sum() == 8                            # the cube around a chunk corner meets eight chunks
        sizes = [(int(o.sprite.size.x), int(o.sprite.size.y), int(o.sprite.size.z)) for o in objs]
        turned = [s for s, o in zip(sizes, objs) if len(set(s)) > 1 and (o.rot.x or o.rot.y or o.rot.z)]
        assert len(turned) == 2
        bricks = np.array(sorted(world_bricks(w)))
        assert len(bricks) >= 3 and all(len(set(bricks[:, a].tolist())) >= 2 for a in range(3))
        if nb >= 4:   # (fewer bricks per axis cannot hold three that differ pairwise)
            assert three_apart(local_bricks(w)) is not None
    else:
        assert len(objs) == 5 and w.origin.tolist() == [-cs, 0, 0] and w.dims.tolist() == [2, 1, 1]
        assert counts.tolist() == [3, 3]                                     # the cube across the shared face is in both lists
        got = local_bricks(w)
        want = {BIG_BRICKS["slab"], BIG_BRICKS["b123"], (nb - 1, nb - 1, nb - 1)}
        assert want <= got and three_apart(want) is not None
        last = w.grid[cs - 8:cs, cs - 8:, cs - 8:]                           # the last brick of the lower chunk
        assert last.any()
    assert w.present.all() or w.present.sum() >= 2
    return c


# ---- C. hit records for the owner pass -----------------------------------------------------------------------------------------
HIT_DTYPE = np.dtype(nat.HIT_FIELDS)
OWNER_DTYPE = np.dtype(nat.OWNER_FIELDS)
MAX_VOXEL_RECORDS = 20000
_records = {}


def owner_records(cs):
    """dict(hits, expect, kind, face, examined, resolved, orphans) for the small world of chunk size cs under a camera scene that
    lists every chunk at resolution 1.
    hits: vrt_hit records -- one per filled voxel (at most 20000, drawn by a seeded generator) standing in the voxel's middle;
    every filled voxel on a lower chunk face once per such axis with pos EXACTLY the integer cell there, and once more with all
    of its face axes exact (the lower candidate chunks are then tried; at resolution 1 the voxel lies outside each of them, so
    none counts); 500 empty cells with material 1, inside and outside the chunk box (orphans); 100 records with material 0 and
    100 with -1 or -2 standing in filled voxels (not examined).  In random order: the lanes of a wave are in different chunks.
    expect: the vrt_owner records, from World.owner and _rotate_index; object indexes the visible objects in build order.
    kind: 0 voxel, 1 face, 2 empty, 3 no hit; face: bit a = pos exact on axis a."""
    if cs in _records:
        return _records[cs]
    c = world_case(cs)
    w, objs = c["w"], c["objs"]
    rng = np.random.default_rng(1000 + cs)
    org = np.asarray(w.origin, np.int64)
    shape = np.array(w.grid.shape, np.int64)
    filled = np.argwhere(w.grid != 0)
    pick = filled
    if len(filled) > MAX_VOXEL_RECORDS:
        pick = filled[np.sort(rng.choice(len(filled), MAX_VOXEL_RECORDS, replace=False))]
    cells, poss, mats_, kinds, faces = [], [], [], [], []

    def add(at, exact, material, kind):
        """Records at grid positions `at` [n, 3]; exact [n, 3] bool: pos is the integer cell on that axis, else the middle."""
        cell = at + org
        exact = np.broadcast_to(exact, cell.shape)
        cells.append(cell)
        poss.append(np.where(exact, cell.astype(np.float64), cell + 0.5))
        mats_.append(np.broadcast_to(np.asarray(material, np.int32), (len(at),)).copy())
        kinds.append(np.full(len(at), kind, np.int8))
        faces.append((exact * np.array([1, 2, 4])).sum(1).astype(np.int8))

    value = lambda at: w.grid[at[:, 0], at[:, 1], at[:, 2]].astype(np.int32)
    none = np.zeros((1, 3), bool)
    add(pick, none, value(pick), 0)
    on = filled % cs == 0
    for a in range(3):
        sel = filled[on[:, a]]
        add(sel, np.arange(3)[None, :] == a, value(sel), 1)
    many = on.sum(1) >= 2
    add(filled[many], on[many], value(filled[many]), 1)
    empty = np.argwhere(w.grid == 0)
    add(empty[rng.choice(len(empty), 400, replace=False)], none, 1, 2)
    out = rng.integers(-cs, shape + cs, (4000, 3))
    out = out[((out < 0) | (out >= shape)).any(1)][:100]
    assert len(out) == 100
    add(out, none, 1, 2)
    nohit = filled[rng.choice(len(filled), 200, replace=False)]
    add(nohit[:100], none, 0, 3)
    add(nohit[100:], none, np.where(np.arange(100) % 2 == 0, -1, -2), 3)
    order = rng.permutation(sum(len(x) for x in cells))
    cell, pos, material = np.concatenate(cells)[order], np.concatenate(poss)[order], np.concatenate(mats_)[order]
    kind, face = np.concatenate(kinds)[order], np.concatenate(faces)[order]
    hits = np.zeros(len(cell), HIT_DTYPE)
    hits["pos"], hits["cell"], hits["material"] = pos, cell, material
    expect = np.zeros(len(cell), OWNER_DTYPE)
    expect["object"] = np.where(material > 0, -2, -1)
    own = kind <= 1
    g = cell[own] - org
    owner = w.owner[g[:, 0], g[:, 1], g[:, 2]]
    assert (owner >= 0).all()
    local = np.zeros((len(owner), 3), np.int64)
    for k in np.unique(owner):
        ob, sel = objs[int(k)], owner == k
        d = cell[own][sel] - np.array([int(ob.mins.x), int(ob.mins.y), int(ob.mins.z)])
        local[sel] = np.stack(_rotate_index(d[:, 0], d[:, 1], d[:, 2], ob.sprite.size, ob.rot), 1)
    expect["object"][own], expect["resolution"][own], expect["voxel"][own], expect["local"][own] = owner, 1, cell[own], local
    for a in (hits, expect, kind, face):
        a.setflags(write=False)
    _records[cs] = dict(hits=hits, expect=expect, kind=kind, face=face, examined=int((material > 0).sum()), resolved=int(own.sum()),
                        orphans=int((kind == 2).sum()))
    return _records[cs]


def model_materials(objs, materials, owner, local):
    """World material ids (1 + index in `materials`) of the model voxels `local` [n, 3] of the objects `owner` [n]: each sprite's
    dense model read at `local`, through its remap."""
    out = np.zeros(len(owner), np.int32)
    ids = [id(m) for m in materials]
    for k in np.unique(owner):
        dense, smats = objs[int(k)].sprite.dense()
        remap = np.array([0] + [1 + ids.index(id(m)) for m in smats], np.int32)
        sel = owner == k
        at = local[sel]
        out[sel] = remap[dense[at[:, 0], at[:, 1], at[:, 2]]]
    return out


def overlap_counts(cs):
    """(later, earlier) over the voxel records of owner_records(cs): records whose voxel lies in the boxes of two or more objects
    and is owned by the LAST of them, and records owned by an earlier one -- every later object is empty there."""
    c, r = world_case(cs), owner_records(cs)
    sel = r["kind"] == 0
    v, own = r["hits"]["cell"][sel].astype(np.int64), r["expect"]["object"][sel]
    b = c["boxes"]
    inside = ((v[:, None, :] >= b[None, :, 0, :]) & (v[:, None, :] < b[None, :, 1, :])).all(2)          # [records, objects]
    last = inside.shape[1] - 1 - np.argmax(inside[:, ::-1], 1)
    assert inside.any(1).all() and inside[np.arange(len(v)), own].all()
    many = inside.sum(1) >= 2
    return int((many & (own == last)).sum()), int((many & (own < last)).sum())


def records_reach(cs):
    """The reach conditions of section C, asserted; returns (world case, records)."""
    c, r = world_case(cs), owner_records(cs)
    n = len(c["objs"])
    own = r["expect"]["object"]
    assert 0 in own and n - 1 in own                                         # owners at both ends of the object array
    later, earlier = overlap_counts(cs)
    assert later >= 50 and earlier >= 50, (later, earlier)
    for a in range(3):
        assert ((r["kind"] == 1) & (r["face"] == 1 << a)).any()
    assert ((r["kind"] == 1) & (np.isin(r["face"], [3, 5, 6, 7]))).any()      # ... and voxels on chunk edges, several axes at once
    assert (r["kind"] == 0).sum() == min(int((c["w"].grid != 0).sum()), MAX_VOXEL_RECORDS) > 1000
    assert (r["kind"] == 2).sum() == 500 and (r["kind"] == 3).sum() == 200
    assert r["examined"] == r["resolved"] + r["orphans"] == len(own) - 200
    return c, r


def half_box(cs):
    """(origin, dims) of the lower half, on x, of the small world's chunk box: it ends at x = 0."""
    w = world_case(cs)["w"]
    return [int(v) for v in w.origin], [int(w.dims[0]) // 2, int(w.dims[1]), int(w.dims[2])]


def in_box(cells, origin, dims, cs):
    lo = np.asarray(origin, np.int64)
    return ((cells >= lo) & (cells < lo + np.asarray(dims, np.int64) * cs)).all(1)


def rounded_box(cs, to):
    """The small world's chunk box rounded outward to multiples of `to` voxels: (origin, top)."""
    w = world_case(cs)["w"]
    lo = np.asarray(w.origin, np.int64)
    hi = lo + np.asarray(w.dims, np.int64) * cs
    return (lo // to) * to, -((-hi) // to) * to
