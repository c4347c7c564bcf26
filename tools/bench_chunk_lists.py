#!/usr/bin/env python3
"""Time the per-chunk object lists (vrt_chunk_lists_build) and the two passes that read them against the scans they replace, in
one process, on the worlds of tools/bench_owners.py (its `cubes`) at 8, 32, 64, 128, 256, 1024 and 4096 objects.

Per world, alternating within every round (a round = one timed window of `--inner` calls of each leg), bracketed by HIP events
after warm-up:
  lists_build                       vrt_chunk_lists_build over the world's chunk box
  voxelize / voxelize_lists         vrt_voxelize against vrt_voxelize_lists over the whole box, into scratch buffers
  owners_scan / owners_lists        DeviceWorld.owners() of a world without and with lists, on the 1920 x 1080 first-hit records
  update_scan / update_lists        DeviceWorld.update() after one object moved by a voxel, under both settings
Before anything is timed the voxel bytes, the table and the owner records with their statistics are asserted equal.
Then one large sparse box -- eight small cubes at the corners of a box of more than 10^5 chunks -- for what the build costs
where chunks, not objects, are many.  Medians over the rounds, each series' interquartile range, and `lists_min`: the smallest
benchmarked count from which on, at every larger count too, build + lists voxelise and the lists owner pass are both faster
than their scans by more than the sum of the series' interquartile ranges (None if the largest world does not win).
The windows time calls through the Python layer, so the update legs measure the host's work on the object list as well.
One JSON object goes to stdout and, with --out, to that file.

    python tools/bench_chunk_lists.py --out profiles/chunk_lists_bench.json
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_owners import HEIGHT, WIDTH, cubes, window  # noqa: E402

COUNTS = (8, 32, 64, 128, 256, 1024, 4096)


def summarise(ms):
    out = {}
    for k, v in ms.items():
        med = statistics.median(v)
        q = statistics.quantiles(v, n=4)
        out[k + "_ms"] = round(med, 4)
        out[k + "_min_ms"] = round(min(v), 4)
        out[k + "_max_ms"] = round(max(v), 4)
        out[k + "_iqr_ms"] = round(q[2] - q[0], 4)
    return out


def measure(torch, legs, warmup, rounds, inner):
    for fn in legs.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in legs}
    for _ in range(rounds):
        for k, fn in legs.items():
            ms[k].append(window(torch, fn, inner))
    return summarise(ms)


def abi_voxelize(torch, nat, dw, lists):
    """A call of vrt_voxelize (lists None) or vrt_voxelize_lists over dw's records and whole box into scratch buffers."""
    n_obj = dw._objects_dev.numel() // C.sizeof(nat.VrtObject)
    o64 = (C.c_int64 * 3)(*[int(v) for v in dw.origin])
    d32 = (C.c_int32 * 3)(*[int(v) for v in dw.dims])
    table, voxels = torch.zeros_like(dw._table), torch.zeros_like(dw._voxels)
    args = (dw._objects_dev.data_ptr(), n_obj, dw._model_dev.data_ptr(), dw._remap_dev.data_ptr(), o64, d32, dw.chunk_size, None, 0,
            table.data_ptr(), voxels.data_ptr())
    struct = lists.c_struct() if lists is not None else None
    # the arguments are raw device addresses: the tensors behind them are held here for as long as the call can be made
    # (a DeviceWorld.update() replaces the world's record tensors, so no world timed here is ever updated)
    held = (dw._objects_dev, dw._model_dev, dw._remap_dev, dw._table, dw._voxels, lists)

    def call(held=held):
        stream = torch.cuda.current_stream().cuda_stream
        if struct is None:
            nat.check(nat.lib().vrt_voxelize(*args, stream), "vrt_voxelize")
        else:
            nat.check(nat.lib().vrt_voxelize_lists(*args, C.byref(struct), stream), "vrt_voxelize_lists")
    return call, table, voxels


def run_world(n_objects, warmup, rounds, inner):
    import torch
    from python_raytracer_amd import Camera, make_settings, _native as nat
    from python_raytracer_amd.lib import quaternion, vec3
    from python_raytracer_amd.world import DeviceWorld
    st = make_settings(width=WIDTH, height=HEIGHT, samples=1)
    st.culling = False
    cs = int(st.chunk_size)
    worlds = {}
    # the same world four times, each DeviceWorld with objects of its own: two that stay as built (their device records are
    # read through raw addresses), two that the update legs move an object of
    for key, on in (("scan", False), ("lists", True), ("scan_moving", False), ("lists_moving", True)):
        objs = cubes(n_objects, 1000 + n_objects)
        dw = DeviceWorld(cs, lists=on)
        worlds[key] = (dw, objs, dw.build(objs))
    scan, lists = worlds["scan"][0], worlds["lists"][0]
    assert torch.equal(scan._table, lists._table) and torch.equal(scan._voxels, lists._voxels), "the two voxelisations disagree"
    cam = Camera(settings=st)
    cam.pos, cam.rot = vec3(0.0, 0.0, 0.0), quaternion(0.0, 0.0, 0.0, 1.0)
    cam.set_world_scene(worlds["scan"][2])
    cam.chunk_update(None)
    dp = cam.upload_pixels(np.concatenate([p.array for p in st.pixels]))
    hits = cam.first_hit(0, pixels=dp)
    a, b = scan.owners(hits, cam), lists.owners(hits, cam)
    assert a.numpy().tobytes() == b.numpy().tobytes() and np.array_equal(a.stats, b.stats), "the two owner passes disagree"
    assert int(a.stats[nat.S_OWNER_ORPHANS]) == 0 and lists.list_calls["owners"] == 1 and scan.list_calls["owners"] == 0
    the_lists = lists.chunk_lists()
    vox_scan, t0, v0 = abi_voxelize(torch, nat, scan, None)
    vox_lists, t1, v1 = abi_voxelize(torch, nat, lists, the_lists)
    vox_scan()
    vox_lists()
    torch.cuda.synchronize()
    assert torch.equal(t0, t1) and torch.equal(v0, v1) and torch.equal(v1, scan._voxels)

    def update(key):
        dw, objs, _ = worlds[key]
        state = {"step": 1}

        def call():
            o = objs[len(objs) // 2]
            o.move(vec3(o.pos.x + state["step"], o.pos.y, o.pos.z))
            state["step"] = -state["step"]
            rebuilt = dw.update(objs)[1]
            assert rebuilt > 0
        return call

    legs = {"lists_build": lambda: lists._build_lists(lists.origin, lists.dims), "voxelize": vox_scan, "voxelize_lists": vox_lists,
            "owners_scan": lambda: scan.owners(hits, cam), "owners_lists": lambda: lists.owners(hits, cam),
            "update_scan": update("scan_moving"), "update_lists": update("lists_moving")}
    out = dict(objects=n_objects, world_chunks=int(np.prod(np.asarray(scan.dims, np.int64))), list_items=the_lists.n_items,
               longest_list=int(np.diff(the_lists.numpy()[0].astype(np.int64)).max()),
               records=int(hits.records.numel() // nat.HIT_BYTES), records_that_hit=int(hits.stats[4]))
    out.update(measure(torch, legs, warmup, rounds, inner))
    assert torch.equal(worlds["scan_moving"][0]._voxels, worlds["lists_moving"][0]._voxels)   # (after the same moves each)
    assert torch.equal(scan._voxels, lists._voxels)
    out["build_plus_voxelize_lists_ms"] = round(out["lists_build_ms"] + out["voxelize_lists_ms"], 4)
    out["voxelize_speedup_with_build"] = round(out["voxelize_ms"] / out["build_plus_voxelize_lists_ms"], 3)
    out["voxelize_speedup"] = round(out["voxelize_ms"] / out["voxelize_lists_ms"], 3)
    out["owners_speedup"] = round(out["owners_scan_ms"] / out["owners_lists_ms"], 3)
    out["update_speedup"] = round(out["update_scan_ms"] / out["update_lists_ms"], 3)
    out["voxelize_wins"] = bool(out["voxelize_ms"] - out["build_plus_voxelize_lists_ms"] >
                                out["voxelize_iqr_ms"] + out["lists_build_iqr_ms"] + out["voxelize_lists_iqr_ms"])
    out["owners_wins"] = bool(out["owners_scan_ms"] - out["owners_lists_ms"] > out["owners_scan_iqr_ms"] + out["owners_lists_iqr_ms"])
    return out


def run_sparse(warmup, rounds, inner):
    """Eight cubes at the corners of a box of 64 x 40 x 40 chunks: the build walks 102400 chunks for eight objects."""
    import torch
    from python_raytracer_amd import _native as nat
    from python_raytracer_amd.lib import vec3
    from python_raytracer_amd.world import DeviceWorld
    cs = 16
    src = cubes(8, 77)
    ext = (64 * cs - 16, 40 * cs - 16, 40 * cs - 16)
    for k, o in enumerate(src):
        o.move(vec3(8 + ((k >> 2) & 1) * ext[0], 8 + ((k >> 1) & 1) * ext[1], 8 + (k & 1) * ext[2]))
    dw = DeviceWorld(cs, lists=True)
    dw.build(src)
    n = int(np.prod(np.asarray(dw.dims, np.int64)))
    assert n >= 100000, dw.dims
    the_lists = dw.chunk_lists()
    vox_scan, t0, v0 = abi_voxelize(torch, nat, dw, None)
    vox_lists, t1, v1 = abi_voxelize(torch, nat, dw, the_lists)
    vox_scan()
    vox_lists()
    torch.cuda.synchronize()
    assert torch.equal(t0, t1) and torch.equal(v0, v1)
    legs = {"lists_build": lambda: dw._build_lists(dw.origin, dw.dims), "voxelize": vox_scan, "voxelize_lists": vox_lists}
    out = dict(objects=len(src), world_chunks=n, dims=[int(d) for d in dw.dims], list_items=the_lists.n_items)
    out.update(measure(torch, legs, warmup, rounds, inner))
    return out


def lists_min(worlds):
    """The smallest count from which on every benchmarked world wins both comparisons; None if the largest does not."""
    best = None
    for w in sorted(worlds, key=lambda w: -w["objects"]):
        if not (w["voxelize_wins"] and w["owners_wins"]):
            break
        best = w["objects"]
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--inner", type=int, default=10, help="calls per timed window")
    ap.add_argument("--counts", type=int, nargs="*", default=list(COUNTS), help="objects per world")
    ap.add_argument("--no-sparse", action="store_true", help="leave out the large sparse box")
    ap.add_argument("--out", default="", help="write the JSON object to this file")
    args = ap.parse_args()
    import torch
    worlds = [run_world(n, args.warmup, args.rounds, args.inner) for n in args.counts]
    sparse = None if args.no_sparse else run_sparse(args.warmup, args.rounds, args.inner)
    out = dict(shape="%dx%dx1, first sample per pixel" % (WIDTH, HEIGHT), warmup=args.warmup, rounds=args.rounds,
               calls_per_window=args.inner, device=torch.cuda.get_device_name(0), worlds=worlds, sparse_box=sparse, lists_min=lists_min(worlds))
    text = json.dumps(out, indent=1)
    print(text, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
