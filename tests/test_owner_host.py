"""The owner pass without a GPU: build_world(owners=True) against the real reference's own record of which object every world
voxel came from (tests/golden/world_owners.npz, made by tests/golden/make_world_owners.py), the C ABI's new record and symbol,
what vrt_hit_owners refuses before any HIP call, and the rule "which voxel a hit record means" (tests/owner_ref.py) against a
march that knows the truth."""
import ctypes as C
import os
import re

import numpy as np

import cast_ref as cr
import oracle_lib as ol
import owner_ref as orf
from python_raytracer_amd import _native as nat
from python_raytracer_amd.lib import vec3
from python_raytracer_amd.world import DeviceWorld, build_world
from test_world import _redraw_sequence, build_from_fixture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vrt.h")


def _fixture():
    z = np.load(os.path.join(ol.GOLDEN, "world_build.npz"))
    seq = np.load(os.path.join(ol.GOLDEN, "world_update.npz"))
    own = np.load(os.path.join(ol.GOLDEN, "world_owners.npz"))
    mats, st, objs = build_from_fixture(z)
    return z, seq, own, mats, st, objs


def spec_owner(w, order, objs):
    """World.owner with its indices into `order` replaced by indices into the fixture's spec list."""
    to_spec = np.array([objs.index(o) for o in order] + [-1], np.int32)   # (-1 stays -1)
    return to_spec[w.owner]


def same_cells(origin_a, a, origin_b, b, fill):
    """Two dense grids over (possibly different) chunk-aligned boxes hold the same values (`fill` outside them)."""
    origin_a, origin_b = np.asarray(origin_a, np.int64), np.asarray(origin_b, np.int64)
    lo = np.minimum(origin_a, origin_b)
    hi = np.maximum(origin_a + a.shape, origin_b + b.shape)
    x, y = np.full(tuple(hi - lo), fill, np.int32), np.full(tuple(hi - lo), fill, np.int32)
    o = origin_a - lo
    x[o[0]:o[0] + a.shape[0], o[1]:o[1] + a.shape[1], o[2]:o[2] + a.shape[2]] = a
    o = origin_b - lo
    y[o[0]:o[0] + b.shape[0], o[1]:o[1] + b.shape[1], o[2]:o[2] + b.shape[2]] = b
    return np.array_equal(x, y)


# ---- 1. the reference's owners ---------------------------------------------------------------------------------------------
def test_owner_grid_matches_the_reference():
    """Tick 0: the first build.  Ticks 1 and 2: the redraws of world_update.npz replayed through DeviceWorld.merge_order, the
    host owner grid built in that order.  The fixture is only worth something where two objects hold one position: the slab
    and the cube share voxels, and the winner there differs between tick 0 and tick 1 -- both asserted."""
    z, seq, own, mats, st, objs = _fixture()
    cam_pos = vec3(*[float(v) for v in z["cam_pos"]])
    vis = [o for o in objs if o.visible]
    order = list(vis)
    w = build_world(order, 16, owners=True)
    assert w.owner.dtype == np.int32 and w.owner.shape == w.grid.shape
    assert same_cells(w.origin, spec_owner(w, order, objs), seq["origin_0"], own["owner_0"], -1)
    # where the slab (spec 0) and the cube (spec 1) both have a voxel
    slab, cube = build_world([objs[0]], 16), build_world([objs[1]], 16)
    lo = np.minimum(slab.origin, cube.origin)
    hi = np.maximum(slab.origin + slab.grid.shape, cube.origin + cube.grid.shape)
    both = np.ones(tuple(hi - lo), bool)
    for part in (slab, cube):
        g = np.zeros(tuple(hi - lo), bool)
        o = part.origin - lo
        g[o[0]:o[0] + part.grid.shape[0], o[1]:o[1] + part.grid.shape[1], o[2]:o[2] + part.grid.shape[2]] = part.grid != 0
        both &= g
    shared = np.argwhere(both) + lo
    assert len(shared) > 0 and len(shared) == int(own["shared_0"])
    ref0 = own["owner_0"][tuple((shared - seq["origin_0"]).T)]
    ref1 = own["owner_1"][tuple((shared - seq["origin_1"]).T)]
    assert set(ref0.tolist()) | set(ref1.tolist()) == {0, 1} and (ref0 != ref1).any()
    winners = [spec_owner(w, order, objs)[tuple((shared - w.origin).T)]]
    for tag, changed in _redraw_sequence(objs, st, cam_pos, seq):
        stay, moved = DeviceWorld.merge_order(order, vis, changed)
        order = stay + moved
        w = build_world(order, 16, owners=True)
        assert same_cells(w.origin, spec_owner(w, order, objs), seq["origin_" + tag], own["owner_" + tag], -1), tag
        winners.append(spec_owner(w, order, objs)[tuple((shared - w.origin).T)])
    assert (winners[0] != winners[1]).any()


# ---- 2. owner and material agree -------------------------------------------------------------------------------------------
def test_owner_and_material_agree():
    """owner >= 0 exactly where the world has a voxel, and the owner's own sprite, asked voxel by voxel through the
    single-position API (Sprite.get_voxel under the object's rotation at p - mins), holds the material the grid holds."""
    z, seq, own, mats, st, objs = _fixture()
    for world_objs in ([o for o in objs if o.visible], orf.lod_world()["objs"]):
        w = build_world(world_objs, 16, owners=True)
        assert np.array_equal(w.owner >= 0, w.grid != 0) and (w.owner >= 0).sum() > 500
        assert w.owner.max() == len(world_objs) - 1 and len(set(np.unique(w.owner).tolist())) >= 4
        filled = np.argwhere(w.grid != 0)
        for p in filled[:: max(1, len(filled) // 3000)]:
            ob = world_objs[int(w.owner[tuple(p)])]
            q = p + w.origin
            m = ob.sprite.get_voxel(None, vec3(int(q[0]) - int(ob.mins.x), int(q[1]) - int(ob.mins.y), int(q[2]) - int(ob.mins.z)),
                                    ob.rot)
            assert m is w.materials[int(w.grid[tuple(p)]) - 1], (p, ob)
    assert build_world(world_objs, 16).owner is None          # (only on request)
    assert (build_world([], 16, owners=True).owner == -1).all()


# ---- 3. the C ABI ----------------------------------------------------------------------------------------------------------
def test_symbols_and_layout():
    text = open(HEADER).read()
    assert re.search(r"typedef struct vrt_owner \{[^}]*int32_t object;[^}]*int32_t resolution;[^}]*int32_t voxel\[3\];[^}]*"
                     r"int32_t local\[3\];[^}]*\} vrt_owner;", text, re.S)
    assert re.search(r"int vrt_hit_owners\(const vrt_scene\* scene, const vrt_hit\* d_hits, int64_t n_hits,\s+"
                     r"const vrt_object\* d_objects, int32_t n_objects, const uint8_t\* d_models, const uint8_t\* d_remap,\s+"
                     r"vrt_owner\* d_owners, uint64_t\* d_stats, void\* stream\);", text)
    for name, word in (("EXAMINED", 8), ("RESOLVED", 4), ("ORPHANS", 9), ("AMBIGUOUS", 10)):
        assert re.search(r"VRT_S_OWNER_%s = %d\b" % (name, word), text), name
    assert "#define VRT_ABI_VERSION 9" in text and "two chunks explain this record; the first was" in text
    L = nat.lib()
    assert L.vrt_abi_version() == 9 and nat.ABI_VERSION == 9      # the change only adds a symbol
    assert L.vrt_hit_owners is not None and "vrt_hit_owners" in nat.EXPORTS
    assert C.sizeof(nat.VrtOwner) == 32 == nat.OWNER_BYTES == np.dtype(nat.OWNER_FIELDS).itemsize
    assert [getattr(nat.VrtOwner, f).offset for f in ("object", "resolution", "voxel", "local")] == [0, 4, 8, 20]
    assert (nat.S_OWNER_EXAMINED, nat.S_OWNER_RESOLVED, nat.S_OWNER_ORPHANS, nat.S_OWNER_AMBIGUOUS) == (8, 4, 9, 10)


def test_hit_owners_rejects_bad_arguments_without_a_device():
    """Everything the entry point can refuse is refused before its first HIP call: these calls carry made-up device
    pointers, which nothing reads."""
    L = nat.lib()
    fake = 0x1000
    sc = nat.VrtScene()
    sc.origin[:] = [-32, -32, -32]
    sc.dims[:] = [4, 4, 4]
    sc.chunk_size, sc.n_slots, sc.n_materials, sc.max_resolution = 16, 64, 4, 3
    sc.d_chunk_table = sc.d_voxels = sc.d_materials = fake

    def call(scene=sc, hits=fake, n=100, objects=fake, n_objects=5, models=fake, remap=fake, owners=fake, stats=fake):
        return L.vrt_hit_owners(C.byref(scene) if scene is not None else None, hits, n, objects, n_objects, models, remap, owners,
                                stats, None)

    assert call(scene=None) == -1 and call(hits=None) == -1 and call(owners=None) == -1 and call(stats=None) == -1
    assert call(objects=None) == -1 and call(models=None) == -1 and call(remap=None) == -1
    assert call(n=-1) == -1 and call(n_objects=-1) == -1 and call(n=1 << 32) == -1 and call(n=(1 << 32) + 5) == -1
    assert call(hits=fake + 4) == -1 and call(owners=fake + 8) == -1        # 8- and 16-byte aligned arrays
    bad = nat.VrtScene.from_buffer_copy(sc)
    bad.chunk_size = 12
    assert call(scene=bad) == -1                                            # the chunk size is a power of two
    bad = nat.VrtScene.from_buffer_copy(sc)
    bad.d_chunk_table = None
    assert call(scene=bad) == -1
    bad = nat.VrtScene.from_buffer_copy(sc)
    bad.origin[0] = -30
    assert call(scene=bad) == -1                                            # the origin is a multiple of it
    bad = nat.VrtScene.from_buffer_copy(sc)
    bad.dims[1] = 0
    assert call(scene=bad) == -1


# ---- 4. which voxel a record means -----------------------------------------------------------------------------------------
def test_march_true_is_the_pinned_restatement():
    """owner_ref.march_true returns cast_ref.march's (step, pos, material) -- which test_cast_host pins to the oracle -- and a
    (chunk, r, c) that holds that material."""
    for name in ("hand", "default"):
        sc, origins, vels, lives, exp = cr.ray_set(name)
        for o, v, l in zip(origins[:200], vels[:200], lives[:200]):
            a = cr.march(sc, round(sc.chunk_size / 2), o, v, l)
            b = orf.march_true(sc, round(sc.chunk_size / 2), o, v, l)
            assert a == b[:3]
            if b[2]:
                assert orf._voxel_in(sc, b[3], [int(np.floor(p)) for p in b[1]]) == (b[4], b[5], b[2])


def _check_rule(sc, truth):
    """The candidate rule recovers the true (chunk, r, c) of every hit.  Returns (hits, face cases among them, records two
    chunks explain)."""
    hits = faces = ambiguous = 0
    for step, pos, mat, cell, r, c in truth:
        if not mat:
            continue
        hits += 1
        got = orf.counting(sc, pos, mat)
        ambiguous += len(got) > 1
        assert got and got[0] == (cell, r, c), (pos, mat, got, (cell, r, c))
        faces += orf.is_face_case(sc, pos, cell)
    return hits, faces, ambiguous


def test_candidate_rule_recovers_the_voxel_on_the_oracle_sets():
    for name in ("hand", "default"):
        sc, origins, vels, lives, exp = cr.ray_set(name)
        truth = [orf.march_true(sc, round(sc.chunk_size / 2), o, v, l) for o, v, l in zip(origins, vels, lives)]
        hits, faces, ambiguous = _check_rule(sc, truth)
        assert hits == int((exp["material"] > 0).sum()) and hits > 50


def test_candidate_rule_recovers_the_voxel_on_integer_rays():
    """About 500 axis-aligned rays from integer points into the LOD world: every position is an integer, so rays stand exactly
    on chunk faces.  The face case -- pos[a] == chunk_max[a], the voxel snapped back into the lower chunk -- is asserted to
    occur; the one constructed record that two chunks explain (the last ray) is the only one the rule is allowed to miss."""
    lw = orf.lod_world()
    sc, truth = lw["scene"], lw["truth"]
    assert 450 <= len(truth) <= 550
    hits, faces, ambiguous = _check_rule(sc, truth[:-1])
    assert hits > 100 and faces >= 5 and ambiguous == 0, (hits, faces, ambiguous)
    assert {t[4] for t in truth if t[2]} == {1, 2, 3}          # all three resolutions occur among the hits
    # the constructed record: the march read A's voxel (30, 21, 6) in the chunk at resolution 3, standing at pos.x == 32.0 after
    # an empty first cell; the chunk above, at resolution 1, holds B's voxel of the same material at floor(pos)
    step, pos, mat, cell, r, c = truth[-1]
    assert (step, pos, cell, r, c) == (3.0, [32.0, 21.0, 6.0], (1, 1, 0), 3, (30, 21, 6)) and mat
    got = orf.counting(sc, pos, mat)
    assert got == [((2, 1, 0), 1, (32, 21, 6)), ((1, 1, 0), 3, (30, 21, 6))]
    w = lw["world"]
    assert orf.host_owner_at(w, (30, 21, 6)) == len(lw["objs"]) - 2 and orf.host_owner_at(w, (32, 21, 6)) == len(lw["objs"]) - 1
