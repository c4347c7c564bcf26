#!/usr/bin/env python3
"""Generate tests/golden/world_owners.npz: WHICH OBJECT every world voxel came from, observed on the real reference.

Needs the reference checkout make_golden.py needs; the test-suite only reads the committed output.  Nothing of the reference
is copied: its modules are imported in place (make_golden.load_reference) and its Window.chunk_update is driven and observed.

The world is the one of world_build.npz, rebuilt from that file's own spec_* arrays and settings, and the ticks are the three
of world_update.npz: the first build, the slab redrawing alone, then the slab and the cube redrawing together after the cube
moved by one voxel.  Before anything is written the script asserts that it reproduces grid_lod0 and grid_0 / grid_1 / grid_2
bit for bit.  For every tick it then walks the reference's `chunks_objects` dict in its own order -- the order in which
chunk_update unions the objects' voxels (init.py:437-439), so the LAST object holding a position wins -- and records

    owner_<k>   int8 grid aligned with world_update.npz's grid_<k> (origin_<k>, dims_<k>): the index into the spec list of the
                object each voxel came from, -1 where the world is empty

which pins "who wins an overlap" by identity -- including the re-insert-at-end order after redraws -- not only through
materials that happen to differ.

Usage:  python tests/golden/make_world_owners.py
"""
import json
import os

import numpy as np

from make_golden import flatten_chunks, frame_points, load_reference, set_config  # noqa: F401  (frame_points: via flatten_chunks)

OUT = os.path.dirname(os.path.abspath(__file__))


def _num(v):
    return float(v) if v % 1 else int(v)


def main():
    z = np.load(os.path.join(OUT, "world_build.npz"))
    seq = np.load(os.path.join(OUT, "world_update.npz"))
    cfg = json.loads(bytes(z["settings"]).decode())
    data, lib, mod = load_reference()
    data.objects.clear()
    set_config(data, **cfg)
    s = data.settings
    s.culling = False
    cs = s.chunk_size
    wm = [data.Material(function=lib.material, albedo=lib.rgb(*[int(v) for v in row[:3]]), roughness=row[3], absorption=row[4],
                        ior=row[5], energy=row[6], solidity=1, weight=0.001, friction=0.1, elasticity=0.5)
          for row in z["materials"]]
    cmap = {str(c): m for c, m in zip(z["colours"], wm)}
    wids = {id(m): i + 1 for i, m in enumerate(wm)}
    assets = os.path.join(OUT, "assets")
    objs = []
    for fn, size, lod, pos, rot in zip(z["spec_files"], z["spec_size"], z["spec_lod"], z["spec_pos"], z["spec_rot"]):
        spr = data.Sprite(size=lib.vec3(*[_num(v) for v in size]), frames=1, lod=int(lod))
        spr.load([os.path.join(assets, str(fn))], cmap)
        ob = data.Object(pos=lib.vec3(*[_num(v) for v in pos]), rot=lib.vec3(*[_num(v) for v in rot]), vel=lib.vec3(0, 0, 0),
                         physics=False)
        ob.set_sprite(spr)
        objs.append(ob)
    cam = mod.Camera()
    cam.pos = lib.vec3(*[float(v) for v in z["cam_pos"]])
    cam.rot = lib.quaternion(0, 0, 0, 1)
    for ob in objs:
        ob.update(cam.pos)
    assert [bool(o.visible) for o in objs] == z["obj_visible"].tolist()
    win = lib.store(timer=0, traversed=[[]], chunks={}, chunks_objects={}, cam=cam)
    index = {o.id: k for k, o in enumerate(objs)}
    out = {}

    def snap(tag):
        lo, dims, _, _, grid = flatten_chunks({p: f[0] for p, f in win.chunks.items() if f}, cs, wids)
        assert np.array_equal(lo, seq["origin_" + tag]) and np.array_equal(dims, seq["dims_" + tag])
        assert np.array_equal(grid, seq["grid_" + tag]), "tick %s: the reference's voxels are not world_update.npz's" % tag
        order = [index[k] for k in win.chunks_objects.keys()]
        assert order == seq["order_" + tag].tolist(), (tag, order)
        owner = np.full(grid.shape, -1, np.int8)
        count = np.zeros(grid.shape, np.int8)                 # how many objects hold each position
        for obj_id, frames in win.chunks_objects.items():     # dict order: the union's order, the last wins
            for frame in frames.values():
                for p in frame.get_voxels():
                    q = tuple(np.array(p) - lo)
                    owner[q] = index[obj_id]
                    count[q] += 1
        assert np.array_equal(owner >= 0, grid != 0)
        out["owner_" + tag] = owner
        out["shared_" + tag] = np.int64((count > 1).sum())
        return owner, count

    mod.Window.chunk_update(win, 1.0)
    lo0, dims0, _, _, grid0 = flatten_chunks({p: f[0] for p, f in win.chunks.items()}, cs, wids)
    assert np.array_equal(lo0, z["origin"]) and np.array_equal(dims0, z["dims"]) and np.array_equal(grid0, z["grid_lod0"])
    own0, cnt0 = snap("0")
    objs[0].redraw = True                                     # tick 1: the slab redraws alone
    mod.Window.chunk_update(win, 1.0)
    own1, cnt1 = snap("1")
    objs[0].redraw = True                                     # tick 2: both redraw, the cube moved by one voxel
    objs[1].move(lib.vec3(*[_num(v) for v in seq["cube_pos_2"]]))
    objs[1].update(cam.pos)
    mod.Window.chunk_update(win, 1.0)
    snap("2")
    # the fixture's whole point: the slab and the cube share voxels, and the winner there flips between ticks 0 and 1
    assert np.array_equal(seq["origin_0"], seq["origin_1"]) and own0.shape == own1.shape
    shared = (cnt0 > 1) & (cnt1 > 1)
    assert shared.sum() > 0 and (own0[shared] != own1[shared]).any(), int(shared.sum())
    assert set(np.unique(own0[shared]).tolist()) | set(np.unique(own1[shared]).tolist()) == {0, 1}
    np.savez_compressed(os.path.join(OUT, "world_owners.npz"), **out)
    print("world_owners: shared voxels per tick", [int(out["shared_%d" % k]) for k in range(3)],
          "winner flips at", int((own0[shared] != own1[shared]).sum()), "of", int(shared.sum()))


if __name__ == "__main__":
    main()
