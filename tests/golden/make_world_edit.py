#!/usr/bin/env python3
"""Generate tests/golden/world_edit.npz: sprite edits (Sprite.set_voxel, set_voxels_area, mix, clear) observed on the real
reference, model and world after every tick.

Needs the reference checkout make_golden.py needs; the test-suite only reads the committed output.  Nothing of the reference
is copied: its modules are imported in place (make_golden.load_reference), its Sprite methods are called and its
Window.chunk_update is driven and observed.

The world (chunk size 8, the synthetic assets of tests/golden/assets, the materials and settings of world_build.npz):

    object 0   the 12^3 cube, turned a quarter about y, overlapping the slab
    object 1   THE SAME SPRITE at another place, turned about x and z
    object 2   the slab

A second 12^3 sprite (`src`: the cube's file under a rotated colour map, with a solid column added) is what the cube is
mixed with.  Every tick edits the cube sprite, sets `redraw` on objects 0 and 1 -- the reference's flow -- and runs chunk_update.  The
edits are chosen by scanning the model in a fixed order for voxels in the state each case needs (the reference raises
KeyError when it clears an empty voxel, so every clear is of filled voxels only) and written into the file as `ops`, JSON:
one list per tick of [sprite, method, arguments...] with materials as indices into world_build.npz's table (null = None).
Tick 0 holds the set-up of `src`.  The calls that must change nothing (a position or an area outside the model, a mix with a
sprite of another size) are part of the ticks.

    origin_<k>, dims_<k>, grid_<k>   the LOD-0 world after tick k (material = index + 1)
    order_<k>                        the reference's merge order (dict order of chunks_objects), object indices
    model_<k>                        the cube sprite's frame as a dense [12, 12, 12] array (material = index + 1, 0 = empty)
    src_model                        the same of `src`, after its set-up

Usage:  python tests/golden/make_world_edit.py
"""
import itertools
import json
import os

import numpy as np

from make_golden import flatten_chunks, frame_points, load_reference, set_config  # noqa: F401  (frame_points: via flatten_chunks)

OUT = os.path.dirname(os.path.abspath(__file__))
CHUNK = 8


def main():
    z = np.load(os.path.join(OUT, "world_build.npz"))
    cfg = json.loads(bytes(z["settings"]).decode())
    data, lib, mod = load_reference()
    data.objects.clear()
    cfg["chunk_size"] = CHUNK
    set_config(data, **cfg)
    s = data.settings
    s.culling = False
    wm = [data.Material(function=lib.material, albedo=lib.rgb(*[int(v) for v in row[:3]]), roughness=row[3], absorption=row[4],
                        ior=row[5], energy=row[6], solidity=1, weight=0.001, friction=0.1, elasticity=0.5)
          for row in z["materials"]]
    colours = [str(c) for c in z["colours"]]
    cmap = dict(zip(colours, wm))
    cmap_src = dict(zip(colours, wm[1:] + wm[:1]))
    wids = {id(m): i + 1 for i, m in enumerate(wm)}
    assets = os.path.join(OUT, "assets")

    def sprite(fn, size, cm):
        spr = data.Sprite(size=lib.vec3(*size), frames=1, lod=0)
        spr.load([os.path.join(assets, fn)], cm)
        return spr

    sprites = {"cube": sprite("cube.txt.gz", (12, 12, 12), cmap), "src": sprite("cube.txt.gz", (12, 12, 12), cmap_src),
               "slab": sprite("slab.txt", (10, 6, 8), cmap)}
    cube, src = sprites["cube"], sprites["src"]
    specs = [("cube", (9, 2, -3), (0, 90, 0)), ("cube", (-20, 5, 14), (90, 0, 180)), ("slab", (0, 0, 0), (0, 0, 0))]
    objs = []
    for name, pos, rot in specs:
        ob = data.Object(pos=lib.vec3(*pos), rot=lib.vec3(*rot), vel=lib.vec3(0, 0, 0), physics=False)
        ob.set_sprite(sprites[name])
        objs.append(ob)
    cam = mod.Camera()
    cam.pos = lib.vec3(*[float(v) for v in z["cam_pos"]])
    cam.rot = lib.quaternion(0, 0, 0, 1)
    for ob in objs:
        ob.update(cam.pos)
    assert all(o.visible for o in objs)
    win = lib.store(timer=0, traversed=[[]], chunks={}, chunks_objects={}, cam=cam)
    index = {o.id: k for k, o in enumerate(objs)}
    out, ops = {}, []

    def dense(spr):
        a = np.zeros((12, 12, 12), np.uint8)
        for p, m in spr.get_voxels(0).items():
            if all(0 <= c < 12 for c in p):
                a[p] = wids[id(m)]
        return a

    def find(spr, shape, want):
        """First box of `shape`, in x-major order of its corner, whose filled mask satisfies want(mask)."""
        full = dense(spr) != 0
        for c in itertools.product(*[range(12 - n + 1) for n in shape]):
            m = full[c[0]:c[0] + shape[0], c[1]:c[1] + shape[1], c[2]:c[2] + shape[2]]
            if want(m):
                return list(c), [c[a] + shape[a] - 1 for a in range(3)]
        raise AssertionError("no box of shape %r in the state asked for" % (shape,))

    def mat(i):
        return None if i is None else wm[i]

    def run(tick):
        """Apply one tick's ops through the reference's own methods."""
        for op in tick:
            spr = sprites[op[0]]
            if op[1] == "set_voxel":
                spr.set_voxel(0, lib.vec3(*op[2]), mat(op[3]), op[4])
            elif op[1] == "set_voxels_area":
                spr.set_voxels_area(0, lib.vec3(*op[2]), lib.vec3(*op[3]), mat(op[4]), op[5])
            elif op[1] == "mix":
                spr.mix(sprites[op[2]], op[3])
            elif op[1] == "clear":
                spr.clear(0 if op[2] is None else op[2])
            else:
                raise AssertionError(op)
        ops.append(tick)

    def snap(k):
        lo, dims, _, _, grid = flatten_chunks({p: f[0] for p, f in win.chunks.items() if f}, CHUNK, wids)
        out["origin_%d" % k], out["dims_%d" % k], out["grid_%d" % k] = lo.astype(np.int64), dims.astype(np.int64), grid
        out["order_%d" % k] = np.array([index[i] for i in win.chunks_objects.keys()], np.int64)
        out["model_%d" % k] = dense(cube)

    def tick(k, edits):
        before = dense(cube)
        run(edits)
        objs[0].redraw = objs[1].redraw = True
        mod.Window.chunk_update(win, 1.0)
        snap(k)
        return before, out["model_%d" % k]

    # tick 0: src gets a solid 4 x 4 x 12 column next to its scattered voxels, then the first build
    run([["src", "set_voxels_area", [4, 4, 0], [7, 7, 11], 3, True]])
    out["src_model"] = dense(src)
    assert (out["src_model"] == 0).any() and (out["src_model"] != 0).any()
    mod.Window.chunk_update(win, 1.0)
    snap(0)
    # tick 1: set_voxel -- dig one filled voxel, place one (force = False) into an empty one; a position outside changes nothing
    dig, _ = find(cube, (1, 1, 1), lambda m: m.all())
    put, _ = find(cube, (1, 1, 1), lambda m: not m.any())
    a, b = tick(1, [["cube", "set_voxel", dig, None, True], ["cube", "set_voxel", put, 2, False],
                    ["cube", "set_voxel", [12, 0, 0], 1, True], ["cube", "set_voxel", [3, -1, 3], 1, True]])
    assert a[tuple(dig)] != 0 and b[tuple(dig)] == 0 and a[tuple(put)] == 0 and b[tuple(put)] == 3 and (a != b).sum() == 2
    # tick 2: set_voxels_area -- a 3 x 2 x 4 box with force over a partly filled region, the same without force over another
    # partly filled region, then a 2^3 of the box just filled -- fully filled -- cleared; an area that leaves the model changes
    # nothing
    part = lambda m: m.any() and not m.all()  # noqa: E731
    f_lo, f_hi = find(cube, (3, 2, 4), part)
    taken = np.zeros((12, 12, 12), bool)
    taken[f_lo[0]:f_hi[0] + 1, f_lo[1]:f_hi[1] + 1, f_lo[2]:f_hi[2] + 1] = True

    def elsewhere(lo_hi_shape, want):
        full = dense(cube) != 0
        for c in itertools.product(*[range(12 - n + 1) for n in lo_hi_shape]):
            sl = tuple(slice(c[a], c[a] + lo_hi_shape[a]) for a in range(3))
            if not taken[sl].any() and want(full[sl]):
                taken[sl] = True
                return list(c), [c[a] + lo_hi_shape[a] - 1 for a in range(3)]
        raise AssertionError("no free box of shape %r" % (lo_hi_shape,))

    n_lo, n_hi = elsewhere((3, 2, 4), part)
    c_lo, c_hi = [f_lo[0] + 1, f_lo[1], f_lo[2] + 1], [f_lo[0] + 2, f_lo[1] + 1, f_lo[2] + 2]
    a, b = tick(2, [["cube", "set_voxels_area", f_lo, f_hi, 0, True], ["cube", "set_voxels_area", n_lo, n_hi, 1, False],
                    ["cube", "set_voxels_area", c_lo, c_hi, None, True],
                    ["cube", "set_voxels_area", [10, 10, 10], [12, 11, 11], 0, True]])
    sl = lambda lo, hi: tuple(slice(lo[i], hi[i] + 1) for i in range(3))  # noqa: E731
    filled = b[sl(f_lo, f_hi)].copy()
    assert (b[sl(c_lo, c_hi)] == 0).all() and (filled == 1).sum() == 24 - 8 and (filled == 0).sum() == 8
    assert np.array_equal(b[sl(n_lo, n_hi)], np.where(a[sl(n_lo, n_hi)] != 0, a[sl(n_lo, n_hi)], 2))
    assert (a[sl(n_lo, n_hi)] != 0).any() and (a[sl(n_lo, n_hi)] == 0).any()
    # tick 3: mix without force (only the cube's gaps take src's voxels); a mix with a sprite of another size changes nothing
    a, b = tick(3, [["cube", "mix", "src", False], ["cube", "mix", "slab", True]])
    assert np.array_equal(b, np.where((a == 0) & (out["src_model"] != 0), out["src_model"], a)) and (a != b).any()
    # tick 4: mix with force
    a, b = tick(4, [["cube", "mix", "src", True]])
    assert np.array_equal(b, np.where(out["src_model"] != 0, out["src_model"], a)) and (a != b).any()
    # tick 5: clear
    a, b = tick(5, [["cube", "clear", None]])
    assert a.any() and not b.any() and out["order_5"].tolist() == [2]
    out["ops"] = np.frombuffer(json.dumps(ops).encode(), np.uint8)
    out["spec_sprite"] = np.array([sp[0] for sp in specs])
    out["spec_pos"] = np.array([sp[1] for sp in specs], np.float64)
    out["spec_rot"] = np.array([sp[2] for sp in specs], np.float64)
    out["chunk_size"] = np.int64(CHUNK)
    np.savez_compressed(os.path.join(OUT, "world_edit.npz"), **out)
    print("world_edit: merge orders", [out["order_%d" % k].tolist() for k in range(6)],
          "model voxels", [int((out["model_%d" % k] != 0).sum()) for k in range(6)])


if __name__ == "__main__":
    main()
