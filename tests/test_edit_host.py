"""Sprite edits on the host (python_raytracer_amd/world.py: Sprite.set_voxel, set_voxels_area, mix, clear and their journal,
edit_world_box) against tests/golden/world_edit.npz -- the real reference's Sprite methods and Window.chunk_update, tick by
tick (tests/golden/make_world_edit.py) -- and the declarations of the two device entry points.  No GPU needed."""
import ctypes
import itertools
import json
import os
import re
import warnings

import numpy as np
import pytest

import oracle_lib as ol
from python_raytracer_amd import Material
from python_raytracer_amd.lib import vec3, rgb, material
from python_raytracer_amd.world import Sprite, Object, build_world, _rotate_index

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ASSETS = os.path.join(ol.GOLDEN, "assets")
N_TICKS = 6


class EditWorld:
    """The world of world_edit.npz on this package's host classes, and its ticks (also used by tests/test_gpu_edit.py)."""

    def __init__(self):
        wb = np.load(os.path.join(ol.GOLDEN, "world_build.npz"))
        self.z = np.load(os.path.join(ol.GOLDEN, "world_edit.npz"))
        self.mats = [Material(function=material, albedo=rgb(*[int(v) for v in row[:3]]), roughness=row[3], absorption=row[4],
                              ior=row[5], energy=row[6]) for row in wb["materials"]]
        colours = [str(c) for c in wb["colours"]]
        cmap, cmap_src = dict(zip(colours, self.mats)), dict(zip(colours, self.mats[1:] + self.mats[:1]))
        self.cs = int(self.z["chunk_size"])

        def sprite(fn, size, cm):
            spr = Sprite(size=vec3(*size), frames=1, lod=0)
            spr.load([os.path.join(ASSETS, fn)], cm)
            return spr

        self.sprites = {"cube": sprite("cube.txt.gz", (12, 12, 12), cmap), "src": sprite("cube.txt.gz", (12, 12, 12), cmap_src),
                        "slab": sprite("slab.txt", (10, 6, 8), cmap)}
        self.objs = []
        for name, pos, rot in zip(self.z["spec_sprite"], self.z["spec_pos"], self.z["spec_rot"]):
            ob = Object(pos=vec3(*[int(v) for v in pos]), rot=vec3(*[int(v) for v in rot]), sprite=self.sprites[str(name)])
            ob.visible = True
            self.objs.append(ob)
        self.ops = json.loads(bytes(self.z["ops"]).decode())

    def run(self, k):
        """Tick k's edits through Sprite's own methods; the calls the reference answered with a warning warn here."""
        mat = lambda i: None if i is None else self.mats[i]  # noqa: E731
        n_warned = 0
        for op in self.ops[k]:
            spr = self.sprites[op[0]]
            with warnings.catch_warnings(record=True) as w:
                warnings.simplefilter("always")
                if op[1] == "set_voxel":
                    spr.set_voxel(0, vec3(*op[2]), mat(op[3]), op[4])
                elif op[1] == "set_voxels_area":
                    spr.set_voxels_area(0, vec3(*op[2]), vec3(*op[3]), mat(op[4]), op[5])
                elif op[1] == "mix":
                    spr.mix(self.sprites[op[2]], op[3])
                elif op[1] == "clear":
                    spr.clear(op[2])
                else:
                    raise AssertionError(op)
            n_warned += bool(w)
        return n_warned

    def model(self, name="cube"):
        """The sprite's dense model in the fixture's numbering (material index + 1)."""
        dense, smats = self.sprites[name].dense()
        return self.fixture_ids(dense, smats)

    def fixture_ids(self, ids, mats):
        lut = np.zeros(256, np.uint8)
        for k, m in enumerate(mats):
            lut[k + 1] = 1 + self.mats.index(m)
        return lut[np.asarray(ids)]

    def same_world(self, origin, grid, k):
        """`grid` at `origin` (fixture numbering) holds the voxels of the fixture's tick k."""
        oa, ga = np.asarray(origin, np.int64), grid
        ob, gb = self.z["origin_%d" % k].astype(np.int64), self.z["grid_%d" % k]
        lo = np.minimum(oa, ob)
        hi = np.maximum(oa + ga.shape, ob + gb.shape)
        a, b = np.zeros(tuple(hi - lo), np.uint8), np.zeros(tuple(hi - lo), np.uint8)
        o = oa - lo
        a[o[0]:o[0] + ga.shape[0], o[1]:o[1] + ga.shape[1], o[2]:o[2] + ga.shape[2]] = ga
        o = ob - lo
        b[o[0]:o[0] + gb.shape[0], o[1]:o[1] + gb.shape[1], o[2]:o[2] + gb.shape[2]] = gb
        return np.array_equal(a, b)


def test_sprite_edits_reproduce_the_reference_models_tick_by_tick():
    w = EditWorld()
    n_noop = {1: 2, 2: 1, 3: 1}   # calls per tick that leave the model (two positions, an area) or are a mix of unequal sizes
    for k in range(N_TICKS):
        journal = len(w.sprites["cube"].edits)
        warned = w.run(k)
        assert np.array_equal(w.model(), w.z["model_%d" % k]), k
        # the no-ops warn and leave no record; every other call of the cube's leaves exactly one
        cube_ops = [op for op in w.ops[k] if op[0] == "cube"]
        assert warned >= n_noop.get(k, 0)
        assert len(w.sprites["cube"].edits) - journal == len(cube_ops) - n_noop.get(k, 0), k
        if k == 0:
            assert np.array_equal(w.model("src"), w.z["src_model"])
    serials = [e.serial for e in w.sprites["cube"].edits]
    assert serials == sorted(set(serials))
    # the records say what was done: a point is a box of one voxel, clear is the whole model with None and force, a mix names
    # its source
    e = [e for e in w.sprites["cube"].edits if e.lo is not None]
    assert e[0].lo == e[0].hi == tuple(w.ops[1][0][2]) and e[0].mat is None and e[0].force
    assert e[-1].lo == (0, 0, 0) and e[-1].hi == (11, 11, 11) and e[-1].mat is None and e[-1].force and e[-1].source is None
    mixes = [x for x in e if x.source]
    assert [(x.source[0] is w.sprites["src"], x.source[1], x.force) for x in mixes] == [(True, 0, False), (True, 0, True)]


def test_edit_rules_outside_the_fixture():
    m1, m2 = [Material(function=material, albedo=rgb(10 * i, 0, 0), roughness=0, absorption=1, ior=0, energy=0) for i in (1, 2)]
    spr = Sprite(size=vec3(4, 6, 4), frames=2, lod=0)
    with pytest.warns(UserWarning):
        spr.set_voxel(None, vec3(0, 6, 0), m1, True)
    with pytest.warns(UserWarning):
        spr.set_voxels_area(None, vec3(0, 0, 0), vec3(3, 5, 4), m1, True)
    assert not spr.edits and not spr.dense()[0].any()
    spr.set_voxel(None, vec3(1, 2, 3), None, True)          # clearing an empty voxel: a no-op (the reference: KeyError)
    assert not spr.dense()[0].any()
    spr.set_voxels_area(1, vec3(0.5, 1, 1), vec3(2.5, 1, 2), m1, True)   # bounds truncated as the reference's range() does
    d = spr.dense(1)[0]
    assert d[0:3, 1, 1:3].all() and d.sum() == 6 and not spr.dense(0)[0].any()
    spr.set_voxel(1, vec3(0, 1, 1), m2, False)              # force = False: only where the voxel is empty
    spr.set_voxel(1, vec3(3, 1, 1), m2, False)
    d, mats = spr.dense(1)
    assert mats[d[0, 1, 1] - 1] is m1 and mats[d[3, 1, 1] - 1] is m2
    assert [e.frame for e in spr.edits] == [0, 1, 1, 1]
    other = Sprite(size=vec3(4, 4, 4), frames=1, lod=0)
    with pytest.warns(UserWarning):
        spr.mix(other, True)
    # mix walks the frames both have; lod > 0 sprites change on the host but journal no operation
    a, b = Sprite(size=vec3(4, 6, 4), frames=1, lod=0), Sprite(size=vec3(4, 4, 4), frames=1, lod=1)
    a.set_voxel(0, vec3(2, 2, 2), m2, True)
    n = len(spr.edits)
    spr.mix(a, True)
    assert len(spr.edits) == n + 1 and spr.edits[-1].frame == 0 and spr.dense(0)[0][2, 2, 2] and (spr.dense(1)[0] != 0).sum() == 7
    b.set_voxels_area(0, vec3(0, 0, 0), vec3(3, 3, 3), m1, True)
    assert b.dense()[0].all() and [e.lo for e in b.edits] == [None]
    assert not hasattr(Sprite, "set_voxels")


def test_host_world_reproduces_the_reference_grids_in_its_merge_orders():
    w = EditWorld()
    for k in range(N_TICKS):
        w.run(k)
        order = [w.objs[i] for i in w.z["order_%d" % k]]
        if k == N_TICKS - 1:
            assert not w.model().any()      # (the cleared cube left the reference's dict: only the slab is listed)
        world = build_world(order, w.cs)
        assert w.same_world(world.origin, w.fixture_ids(world.grid, world.materials), k), k
    # the order matters: the slab and the first cube overlap, and tick 1's world is not the one the first order gives
    assert w.z["order_0"].tolist() != w.z["order_1"].tolist()


def _brute_force_box(spr, ob, lo, hi):
    ext = [int(ob.maxs.x - ob.mins.x), int(ob.maxs.y - ob.mins.y), int(ob.maxs.z - ob.mins.z)]
    seen = []
    for x, y, z in itertools.product(*[range(n) for n in ext]):
        m = _rotate_index(x, y, z, spr.size, ob.rot)
        if all(lo[a] <= m[a] <= hi[a] for a in range(3)):
            seen.append((x + int(ob.mins.x), y + int(ob.mins.y), z + int(ob.mins.z)))
    if not seen:
        return None, 0
    a = np.array(seen)
    return (tuple(a.min(0).tolist()), tuple((a.max(0) + 1).tolist())), len(seen)


@pytest.mark.parametrize("size,pos", [((4, 4, 4), (3, -2, 7)), ((4, 6, 4), (3, -2, 7)), ((4, 4, 4), (2.5, 0, -1.25))],
                         ids=["cube", "4x6x4", "fractional"])
def test_edit_world_box_against_brute_force_for_every_turn(size, pos):
    from python_raytracer_amd.world import edit_world_box
    spr = Sprite(size=vec3(*size), frames=1, lod=0)
    boxes = [((0, 0, 0), (0, 0, 0)), ((3, size[1] - 1, 3), (3, size[1] - 1, 3)), ((1, 0, 2), (2, 1, 3)), ((0, 2, 0), (3, 2, 1)),
             ((0, 0, 0), (3, size[1] - 1, 3)), ((3, 0, 0), (3, 0, 3))]
    n_none = 0
    for turns in itertools.product(range(4), repeat=3):
        ob = Object(pos=vec3(*pos), rot=vec3(*[90 * t for t in turns]), sprite=spr)
        for lo, hi in boxes:
            want, count = _brute_force_box(spr, ob, lo, hi)
            got = edit_world_box(spr.size, ob.rot, ob.mins, ob.maxs, lo, hi)
            assert got == want, (turns, lo, hi)
            if want is None:
                n_none += 1
            else:   # the image of a box under a signed permutation is a box: nothing in it is spared
                assert count == np.prod(np.array(want[1]) - np.array(want[0]))
    if any(p % 1 for p in pos):
        assert n_none > 0   # (an object at a fractional position is one voxel short on that axis: some edits do not show)


def test_header_and_exports_declare_the_edit_entry_points():
    from python_raytracer_amd import _native as nat
    h = open(os.path.join(ROOT, "include", "vrt.h")).read()
    assert re.search(r"#define VRT_ABI_VERSION 9\b", h) and nat.ABI_VERSION == 9     # the change only adds symbols
    assert re.search(r"int vrt_edit_models\(uint8_t\* d_models, int64_t models_bytes, const vrt_edit\* d_edits, int32_t n_edits,\s+"
                     r"uint64_t\* d_stats, void\* stream\);", h)
    assert re.search(r"int vrt_stamp_model\(uint8_t\* d_models, int64_t models_bytes, int64_t dst, int64_t src, const int32_t\* size,\s+"
                     r"const uint8_t\* d_idmap, int32_t force, void\* stream\);", h)
    assert "vrt_edit_models" in nat.EXPORTS and "vrt_stamp_model" in nat.EXPORTS
    src = open(os.path.join(ROOT, "python_raytracer_amd", "csrc", "vrt_kernels.hip")).read()
    for name in ("vrt_edit_models", "vrt_stamp_model"):
        assert re.search(r"^int %s\(" % name, src, re.M)


def test_edit_record_is_64_bytes():
    from python_raytracer_amd import _native as nat
    assert ctypes.sizeof(nat.VrtEdit) == 64 == nat.EDIT_BYTES
    assert [(f[0], getattr(nat.VrtEdit, f[0]).offset) for f in nat.VrtEdit._fields_] == [
        ("model", 0), ("size", 8), ("lo", 20), ("hi", 32), ("value", 44), ("force", 48), ("pad", 52)]
