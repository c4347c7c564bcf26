#!/usr/bin/env python3
"""Generate tests/golden/world_random.npz: a world of 64 objects, one per quarter-turn triple, voxelised by the real
reference -- its voxels, its object boxes and WHICH OBJECT every voxel came from.

Needs the reference checkout make_golden.py needs; the test-suite only reads the committed output.  Nothing of the reference
is copied: its modules are imported in place (make_golden.load_reference) and its Sprite / Object / Window.chunk_update are
driven and observed.  world_build.npz pins six objects with three distinct rotation triples; this one pins the rotation
rule itself (data.py:338-371): every combination of quarter turns, on models whose extents let a turn take effect and on
models whose extents make the reference ignore it, with angles that only banker's rounding of rot / 90 maps to their turn.

The world (seeded, deterministic):
  * 64 objects; object k has the turns of a shuffled list of all (x, y, z) in {0..3}^3;
  * sizes cycle through 8^3, 6^3, 6 x 8 x 8, 8 x 6 x 8, 8 x 8 x 6 (two equal extents: turns about one axis apply) and
    6 x 8 x 10 (none applies);
  * sprite LOD 0, every fourth object 1 (Frame resolution 2: only even model positions are kept);
  * positions inside a box of 56 x 40 x 56 with fractions .0, .25 and .5;
  * every angle is 90 * turn, moved on some axes by +360, -360, +10, -20 and, for even turns, +45 and -45 (45 -> 0, 135 -> 2,
    -45 -> 0, 225 -> 2: round-half-even decides);
  * a few objects sit almost on top of their predecessor with dense models (deliberate overlaps);
  * one object lies beyond dist_max: invisible, it leaves no voxel.

Written:
    spec_size, spec_lod, spec_pos, spec_rot     the objects as given to Sprite(...) and Object(...)
    vox, vox_start                              int16 [n, 4] (x, y, z, material index into `materials`) of every model in
                                                set_voxels order, object k = vox[vox_start[k]:vox_start[k + 1]]
    materials                                   [5, 7] r, g, b, roughness, absorption, ior, energy
    sprite_size, obj_mins, obj_maxs, obj_visible  what the reference made of them
    origin, dims, present, grid_lod0            its lod-0 world grid (make_golden.flatten_chunks; 1 + material index)
    owner                                       int8 grid like grid_lod0: the spec index of the object each voxel came from,
                                                -1 where empty -- `chunks_objects` walked in dict order, the last holder
                                                wins (init.py:437-439), as make_world_owners.py walks it
    contested                                   how many voxels two or more objects hold
    turns_effective, turns_ignored              how many visible objects have a turn that applies / that the size rule ignores
    cam_pos, settings

The file is only written if at least 40 objects have a turn that takes effect, at least 10 one that is ignored and at least
20 voxels are contested.

Usage:  python tests/golden/make_world_random.py
"""
import json
import os
import time

import numpy as np

from make_golden import flatten_chunks, load_reference, set_config, settings_dict

OUT = os.path.dirname(os.path.abspath(__file__))
SIZES = [(8, 8, 8), (6, 6, 6), (6, 8, 8), (8, 6, 8), (8, 8, 6), (6, 8, 10)]
MATERIALS = np.array([[255, 0, 0, 0.5, 1.0, 1.0, 0.0], [0, 255, 0, 0.0, 0.5, 0.5, 0.0], [0, 0, 255, 0.25, 1.5, 1.0, 2.0],
                      [127, 127, 127, 0.1, 0.25, 0.0, 0.0], [255, 255, 0, 1.0, 2.0, 0.75, 0.5]])
CAM_POS = (2.0, 3.0, -40.0)
ON_TOP = (5, 17, 29, 41, 53)       # these sit on their predecessor
INVISIBLE = 37


def _num(v):
    return float(v) if v % 1 else int(v)


def angle(rng, turn):
    """An angle in degrees that round(angle / 90) % 4 -- with Python's round-half-even -- maps to `turn`."""
    moves = [0, 0, 360, -360, 10, -20] + ([45, -45] if turn % 2 == 0 else [])
    a = 90 * turn + int(rng.choice(moves))
    assert round(a / 90) % 4 == turn
    return a


def make_spec():
    rng = np.random.default_rng(6464)
    triples = [tuple(int(v) for v in t) for t in rng.permutation(np.array(list(np.ndindex(4, 4, 4))))]
    spec = []
    for k, turns in enumerate(triples):
        size = SIZES[k % len(SIZES)]
        lod = 1 if k % 4 == 3 else 0
        dense = k in ON_TOP or k + 1 in ON_TOP
        vox = {}
        for p in np.ndindex(*size):
            if rng.random() < (0.6 if dense else 0.15):
                vox[p] = int(rng.integers(0, len(MATERIALS)))
        if k in ON_TOP:
            pos = tuple(float(np.floor(p)) + d for p, d in zip(spec[-1]["pos"], (1, 0.5, -2)))
        else:
            pos = tuple(int(rng.integers(-h, h)) + float(rng.choice([0.0, 0.0, 0.25, 0.5])) for h in (28, 20, 28))
        if k == INVISIBLE:
            pos = (400.0, 0.25, -3.0)
        spec.append(dict(size=size, lod=lod, pos=pos, rot=tuple(angle(rng, t) for t in turns), turns=turns, vox=vox))
    moved = sorted({r - 90 * t for s in spec for r, t in zip(s["rot"], s["turns"])})
    assert moved == [-360, -45, -20, 0, 10, 45, 360], moved
    assert any(r == 135 for s in spec for r in s["rot"]) and any(r == 45 for s in spec for r in s["rot"])
    assert {f for s in spec for f in (p % 1 for p in s["pos"])} == {0.0, 0.25, 0.5}
    return spec


def turn_use(spec_k, sprite_size):
    """(a turn applies, a turn is ignored) under the size rule of data.py:345, 354, 363."""
    sx, sy, sz = sprite_size
    ok = (sy == sz, sx == sz, sx == sy)
    return (any(t and e for t, e in zip(spec_k["turns"], ok)), any(t and not e for t, e in zip(spec_k["turns"], ok)))


def main():
    t0 = time.time()
    spec = make_spec()
    data, lib, mod = load_reference()
    data.objects.clear()
    set_config(data, width=48, height=36, samples=2, max_bounces=4, threads=1, dist_max=192, dist_min=0, chunk_size=16,
               chunk_lod=0)
    s = data.settings
    s.culling = False
    cs = s.chunk_size
    wm = [data.Material(function=lib.material, albedo=lib.rgb(*[int(v) for v in row[:3]]), roughness=float(row[3]),
                        absorption=float(row[4]), ior=float(row[5]), energy=float(row[6]), solidity=1, weight=0.001, friction=0.1,
                        elasticity=0.5) for row in MATERIALS]
    wids = {id(m): i + 1 for i, m in enumerate(wm)}
    cam = mod.Camera()
    cam.pos = lib.vec3(*CAM_POS)
    cam.rot = lib.quaternion(0, 0, 0, 1)
    objs = []
    for sp in spec:
        spr = data.Sprite(size=lib.vec3(*sp["size"]), frames=1, lod=sp["lod"])
        spr.get_frame(0).set_voxels({p: wm[m] for p, m in sp["vox"].items()}, True)
        ob = data.Object(pos=lib.vec3(*[_num(v) for v in sp["pos"]]), rot=lib.vec3(*sp["rot"]), vel=lib.vec3(0, 0, 0), physics=False)
        ob.set_sprite(spr)
        ob.update(cam.pos)
        objs.append(ob)
    assert [bool(o.visible) for o in objs] == [k != INVISIBLE for k in range(len(objs))]
    win = lib.store(timer=0, traversed=[[]], chunks={}, chunks_objects={}, cam=cam)
    mod.Window.chunk_update(win, 1.0)
    lo, dims, present, _, grid = flatten_chunks({p: f[0] for p, f in win.chunks.items()}, cs, wids)
    index = {o.id: k for k, o in enumerate(objs)}
    assert [index[k] for k in win.chunks_objects.keys()] == [k for k in range(len(objs)) if k != INVISIBLE]
    owner = np.full(grid.shape, -1, np.int8)
    count = np.zeros(grid.shape, np.int8)
    for obj_id, frames in win.chunks_objects.items():     # dict order: the union's order, the last wins
        for frame in frames.values():
            for p in frame.get_voxels():
                q = tuple(np.array(p) - lo)
                owner[q] = index[obj_id]
                count[q] += 1
    assert np.array_equal(owner >= 0, grid != 0)
    sizes = [(o.sprite.size.x, o.sprite.size.y, o.sprite.size.z) for o in objs]
    use = [turn_use(sp, sz) for k, (sp, sz) in enumerate(zip(spec, sizes)) if k != INVISIBLE]
    effective, ignored, contested = sum(u[0] for u in use), sum(u[1] for u in use), int((count > 1).sum())
    print("world_random: %d voxels, %d chunks, %d objects with a turn that applies, %d with one that is ignored, %d contested "
          "voxels, %d owners, %.1f s" % (int((grid != 0).sum()), int(present.sum()), effective, ignored, contested,
                                        len(np.unique(owner[owner >= 0])), time.time() - t0))
    assert effective >= 40 and ignored >= 10 and contested >= 20
    assert len({sp["turns"] for sp in spec}) == 64
    vox = [np.array([p + (m,) for p, m in sp["vox"].items()], np.int16).reshape(-1, 4) for sp in spec]
    np.savez_compressed(
        os.path.join(OUT, "world_random.npz"),
        spec_size=np.array([sp["size"] for sp in spec], np.float64), spec_lod=np.array([sp["lod"] for sp in spec], np.int64),
        spec_pos=np.array([sp["pos"] for sp in spec], np.float64), spec_rot=np.array([sp["rot"] for sp in spec], np.float64),
        vox=np.concatenate(vox), vox_start=np.cumsum([0] + [len(v) for v in vox]).astype(np.int64), materials=MATERIALS,
        sprite_size=np.array(sizes, np.int64),
        obj_mins=np.array([[o.mins.x, o.mins.y, o.mins.z] for o in objs], np.float64),
        obj_maxs=np.array([[o.maxs.x, o.maxs.y, o.maxs.z] for o in objs], np.float64),
        obj_visible=np.array([bool(o.visible) for o in objs]),
        origin=lo.astype(np.int64), dims=dims.astype(np.int64), present=present, grid_lod0=grid, owner=owner,
        contested=np.int64(contested), turns_effective=np.int64(effective), turns_ignored=np.int64(ignored),
        cam_pos=np.array(CAM_POS, np.float64), settings=np.frombuffer(json.dumps(settings_dict(data)).encode(), np.uint8))
    print("  -> world_random.npz (%d bytes)" % os.path.getsize(os.path.join(OUT, "world_random.npz")))


if __name__ == "__main__":
    main()
