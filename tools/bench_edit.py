#!/usr/bin/env python3
"""Time one dug voxel of the default world's castle, end to end, by the two routes there are, in one process:

    (i)  Sprite.set_voxel + DeviceWorld.update   the edit goes to the device as one 64-byte record (vrt_edit_models) and the
                                                 one chunk it can change is recombined (vrt_voxelize with a chunk list)
    (ii) Sprite.set_voxel + DeviceWorld.invalidate + build   the only route before: every model is re-densified on the host
                                                 (Sprite.dense walks the castle's ~207 000 cells in Python), uploaded, and the
                                                 whole chunk box is voxelised

The world is the reference's default mod (tests/golden/mod_default/voxels: the castle, six material cubes, the player, placed as
the mod places them), chunk size 16.  Every iteration digs another filled voxel of the castle and is timed by the wall clock
from before set_voxel until the device has finished (torch.cuda.synchronize), host work included -- most of route (ii) IS host
work.  After warm-up, the median of the repetitions and their spread; route (i) must report one rebuilt chunk every time.
The kernels alone, bracketed by HIP events in windows of `--inner` launches: vrt_edit_models with one point record, vrt_voxelize
of one chunk, vrt_voxelize of the whole box.  One JSON object goes to stdout and, with --out, to that file.

    python tools/bench_edit.py --out profiles/edit_bench.json
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
VOXELS = os.path.join(ROOT, "tests", "golden", "mod_default", "voxels")


def default_world():
    from python_raytracer_amd import Material
    from python_raytracer_amd.lib import vec3, rgb, material
    from python_raytracer_amd.world import Sprite, Object

    def mat(i):
        return Material(function=material, albedo=rgb(20 * i, 120, 250 - 20 * i), roughness=0.1, absorption=1, ior=0, energy=0)

    castle = {c: mat(k) for k, c in enumerate(("000000", "3f3f3f", "7f7f7f", "bfbfbf", "ffffff"))}
    base, player = mat(5), mat(6)
    spec = [("castle.txt.gz", (128, 64, 128), castle, (0, 0, 0))]
    for k, pos in enumerate(((-56, -16, 56), (12, -24, 24), (48, -24, -48), (-4, 18, 16), (-56, 18, 16), (-36, 18, -36))):
        spec.append(("material.txt.gz", (12, 12, 12), {"7f7f7f": base, "ffffff": mat(7 + k)}, pos))
    spec.append(("player.txt.gz", (12, 16, 12), {"7f7f7f": player}, (-12, 0, -8)))
    objs = []
    for fn, size, cmap, pos in spec:
        spr = Sprite(size=vec3(*size), frames=1, lod=0)
        spr.load([os.path.join(VOXELS, fn)], cmap)
        ob = Object(pos=vec3(*pos), rot=vec3(0, 0, 0), sprite=spr)
        ob.visible = True
        objs.append(ob)
    return objs


def series(v):
    med = statistics.median(v)
    q = statistics.quantiles(v, n=4)
    return dict(median_ms=round(med, 4), min_ms=round(min(v), 4), max_ms=round(max(v), 4),
                iqr_over_median=round((q[2] - q[0]) / med, 4), repetitions=len(v))


def window(torch, fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=10, help="untimed iterations of route (i) and kernel windows")
    ap.add_argument("--reps", type=int, default=50, help="timed iterations of route (i)")
    ap.add_argument("--rebuild-warmup", type=int, default=1)
    ap.add_argument("--rebuild-reps", type=int, default=7, help="timed iterations of route (ii)")
    ap.add_argument("--rounds", type=int, default=20, help="kernel windows")
    ap.add_argument("--inner", type=int, default=20, help="launches per kernel window")
    ap.add_argument("--out", default="", help="write the JSON object to this file")
    args = ap.parse_args()
    import torch
    from python_raytracer_amd import _native as nat
    from python_raytracer_amd.lib import vec3
    from python_raytracer_amd.world import DeviceWorld, build_world
    objs = default_world()
    castle = objs[0].sprite
    dense = castle.dense()[0]
    filled = np.argwhere(dense != 0)
    np.random.default_rng(1).shuffle(filled)
    digs = iter(filled.tolist())
    cs = 16
    dw, old = DeviceWorld(cs), DeviceWorld(cs)
    dw.build(objs)
    old.build(objs)
    torch.cuda.synchronize()

    def edit_update():
        p = next(digs)
        t0 = time.perf_counter()
        castle.set_voxel(None, vec3(*p), None, True)
        _, rebuilt = dw.update(objs)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        assert rebuilt == 1, rebuilt
        return (t1 - t0) * 1e3

    def edit_rebuild():
        p = next(digs)
        t0 = time.perf_counter()
        castle.set_voxel(None, vec3(*p), None, True)
        old.invalidate()
        old.build(objs)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    for _ in range(args.warmup):
        edit_update()
    leg_update = [edit_update() for _ in range(args.reps)]
    for _ in range(args.rebuild_warmup):
        edit_rebuild()
    leg_rebuild = [edit_rebuild() for _ in range(args.rebuild_reps)]
    # both routes end in the same world: the host's
    dw.update(objs)
    torch.cuda.synchronize()

    def same_world():   # (each world numbers the materials in the order it met them)
        lut = torch.tensor([0] + [1 + [id(x) for x in old.materials].index(id(m)) for m in dw.materials], dtype=torch.uint8,
                           device="cuda")
        return torch.equal(lut[dw._voxels.long()], old._voxels) and torch.equal(dw._table, old._table)

    assert same_world()
    host = build_world(objs, cs)
    assert int((host.grid != 0).sum()) == int((dw._voxels != 0).sum().item())

    # the kernels alone
    off, shape, _ = dw._models[(id(castle), 0)]
    p = filled[0].tolist()                                     # (dug already: the record changes nothing, launch after launch)
    rec = nat.VrtEdit()
    rec.model, rec.value, rec.force = off, 0, 1
    rec.size[:], rec.lo[:], rec.hi[:] = list(shape), p, p
    d_rec = torch.from_numpy(np.frombuffer((nat.VrtEdit * 1)(rec), np.uint8).copy()).cuda()
    stats = torch.empty(nat.NSTATS, dtype=torch.int64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    o64 = (C.c_int64 * 3)(*[int(v) for v in dw.origin])
    d32 = (C.c_int32 * 3)(*[int(v) for v in dw.dims])
    w = np.array(p) + np.array([objs[0].mins.x, objs[0].mins.y, objs[0].mins.z]) - np.asarray(dw.origin)
    cell = int(((w[0] // cs) * int(dw.dims[1]) + w[1] // cs) * int(dw.dims[2]) + w[2] // cs)
    d_list = torch.tensor([cell], dtype=torch.int32, device="cuda")
    n_obj = len(dw.order)

    def k_edit():
        nat.check(nat.lib().vrt_edit_models(dw._model_dev.data_ptr(), dw._model_dev.numel(), d_rec.data_ptr(), 1, stats.data_ptr(),
                                            stream), "vrt_edit_models")

    def k_voxelize(lst, n):
        def call():
            nat.check(nat.lib().vrt_voxelize(dw._objects_dev.data_ptr(), n_obj, dw._model_dev.data_ptr(), dw._remap_dev.data_ptr(),
                                             o64, d32, cs, lst, n, dw._table.data_ptr(), dw._voxels.data_ptr(), stream), "vrt_voxelize")
        return call

    kernels = {"vrt_edit_models_one_record": k_edit, "vrt_voxelize_one_chunk": k_voxelize(d_list.data_ptr(), 1),
               "vrt_voxelize_whole_box": k_voxelize(None, 0)}
    for fn in kernels.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in kernels}
    for _ in range(args.rounds):
        for k, fn in kernels.items():
            ms[k].append(window(torch, fn, args.inner))
    assert same_world() and int(stats[nat.S_EDIT_INVALID].item()) == 0
    out = dict(world="default mod: castle 128x64x128 (%d voxels), 6 material cubes, player; chunk size %d, %d world chunks"
                     % (len(filled), cs, int(np.prod(np.asarray(dw.dims, np.int64)))),
               device=torch.cuda.get_device_name(0), timing="wall clock per iteration incl. host work and device completion",
               edit_update=series(leg_update), invalidate_build=series(leg_rebuild),
               kernels_hip_events={k: dict(series(v), launches_per_window=args.inner) for k, v in ms.items()},
               chunks_rebuilt_per_edit=1, edit_calls=dw.edit_calls)
    text = json.dumps(out, indent=1)
    print(text, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
