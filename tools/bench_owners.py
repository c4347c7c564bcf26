#!/usr/bin/env python3
"""Time the owner pass (DeviceWorld.owners -> vrt_hit_owners) against the first-hit pass that produced its records, on a
1920 x 1080 frame over worlds of 8, 256 and 4096 objects, in one process.

Each world is random small cubes (edge 4, 8 or 12, 60 % full, eight materials, every quarter turn) scattered through the view
volume of a camera with the reference's defaults (dist_max 192, chunk_lod 2: the far chunks are rendered at resolution 3).
Before anything is timed the owner records of the two stagings of the object list -- uniform loads from memory, tiles in LDS
(VRT_OWNER_LDS=0 / 1) -- are asserted equal, and no record may be an orphan.

Per world, alternating within every round (a round = one timed window of `--inner` calls of each), bracketed by HIP events after
warm-up: first_hit (one record per pixel), the owner pass with each staging and with the library's own choice, and vrt_voxelize
of the same world (the whole chunk box).  Medians over the rounds, each series' spread, and the ratios owner pass / first_hit.
The windows time calls through the Python layer, so the smallest worlds measure launch and allocation as much as the kernel.
One JSON object goes to stdout and, with --out, to that file.

    python tools/bench_owners.py --out profiles/owners_bench.json
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

WIDTH, HEIGHT = 1920, 1080
COUNTS = (8, 256, 4096)


def window(torch, fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def cubes(n, seed):
    from python_raytracer_amd import Material
    from python_raytracer_amd.lib import vec3, rgb, material
    from python_raytracer_amd.world import Sprite, Object
    rng = np.random.default_rng(seed)
    mats = [Material(function=material, albedo=rgb(30 * i, 90, 200 - 20 * i), roughness=0.1, absorption=1, ior=0, energy=0)
            for i in range(1, 9)]
    sprites = []
    for e in (4, 8, 12):
        for _ in range(8):
            spr = Sprite(size=vec3(e, e, e), frames=1, lod=0)
            keep = rng.random((e, e, e)) < 0.6
            spr.get_frame(0).set_voxels({tuple(int(v) for v in p): mats[int(rng.integers(0, 8))] for p in np.argwhere(keep)}, True)
            sprites.append(spr)
    objs = []
    for _ in range(n):
        # inside the camera's view volume: the camera stands at the origin and looks along +z with a 90-degree lens
        z = float(rng.uniform(12, 180))
        pos = [int(rng.uniform(-0.8, 0.8) * z), int(rng.uniform(-0.45, 0.45) * z), int(z)]
        ob = Object(pos=vec3(*pos), rot=vec3(*[int(rng.choice([0, 90, 180, 270])) for _ in range(3)]),
                    sprite=sprites[int(rng.integers(0, len(sprites)))])
        ob.visible = True
        objs.append(ob)
    return objs


def run_world(n_objects, warmup, rounds, inner):
    import torch
    from python_raytracer_amd import Camera, make_settings, _native as nat
    from python_raytracer_amd.lib import quaternion, vec3
    from python_raytracer_amd.world import DeviceWorld
    st = make_settings(width=WIDTH, height=HEIGHT, samples=1)
    st.culling = False
    dw = DeviceWorld(int(st.chunk_size))
    ps = dw.build(cubes(n_objects, 1000 + n_objects))
    cam = Camera(settings=st)
    cam.pos, cam.rot = vec3(0.0, 0.0, 0.0), quaternion(0.0, 0.0, 0.0, 1.0)
    cam.set_world_scene(ps)
    table = cam.chunk_update(None).cpu().numpy().view(np.uint32)
    dp = cam.upload_pixels(np.concatenate([p.array for p in st.pixels]))
    hits = cam.first_hit(0, pixels=dp)

    def owners(staging):
        def call():
            if staging is None:
                os.environ.pop("VRT_OWNER_LDS", None)
            else:
                os.environ["VRT_OWNER_LDS"] = staging
            return dw.owners(hits, cam)
        return call

    # the stagings must agree before anything is timed
    a, b, c = owners("0")(), owners("1")(), owners(None)()
    assert a.numpy().tobytes() == b.numpy().tobytes() == c.numpy().tobytes(), "the two stagings disagree"
    assert np.array_equal(a.stats, b.stats) and int(a.stats[nat.S_OWNER_ORPHANS]) == 0, a.stats
    assert int(a.stats[nat.S_OWNER_EXAMINED]) == int(hits.stats[4])

    n_cells = int(np.prod(np.asarray(dw.dims, np.int64)))
    o64 = (C.c_int64 * 3)(*[int(v) for v in dw.origin])
    d32 = (C.c_int32 * 3)(*[int(v) for v in dw.dims])
    scratch_table, scratch_voxels = torch.zeros_like(dw._table), torch.zeros_like(dw._voxels)

    def voxelize():
        nat.check(nat.lib().vrt_voxelize(dw._objects_dev.data_ptr(), n_objects, dw._model_dev.data_ptr(), dw._remap_dev.data_ptr(),
                                         o64, d32, int(st.chunk_size), None, 0, scratch_table.data_ptr(), scratch_voxels.data_ptr(),
                                         torch.cuda.current_stream().cuda_stream), "vrt_voxelize")

    voxelize()
    torch.cuda.synchronize()
    assert torch.equal(scratch_voxels, dw._voxels)
    legs = {"first_hit": lambda: cam.first_hit(0, pixels=dp), "owners_uniform": owners("0"), "owners_lds": owners("1"),
            "owners": owners(None), "voxelize": voxelize}
    for fn in legs.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in legs}
    for _ in range(rounds):
        for k, fn in legs.items():
            ms[k].append(window(torch, fn, inner))
    os.environ.pop("VRT_OWNER_LDS", None)
    med = {k: statistics.median(v) for k, v in ms.items()}
    res = (table >> 24)[table != 0]
    out = dict(objects=n_objects, world_chunks=n_cells, chunks_listed=int((table != 0).sum()),
               chunks_at_resolution={str(r): int((res == r).sum()) for r in (1, 2, 3)},
               records=int(hits.records.numel() // nat.HIT_BYTES), records_that_hit=int(hits.stats[4]),
               ambiguous=int(a.stats[nat.S_OWNER_AMBIGUOUS]),
               resolved_at_resolution={str(r): int(((a.numpy()["resolution"] == r) & (a.numpy()["object"] >= 0)).sum()) for r in (1, 2, 3)})
    for k, v in ms.items():
        out[k + "_ms"] = round(med[k], 4)
        out[k + "_min_ms"] = round(min(v), 4)
        out[k + "_max_ms"] = round(max(v), 4)
        q = statistics.quantiles(v, n=4)
        out[k + "_iqr_over_median"] = round((q[2] - q[0]) / med[k], 4)
    for k in ("owners_uniform", "owners_lds", "owners"):
        out[k + "_over_first_hit"] = round(med[k] / med["first_hit"], 4)
    out["owners_lds_over_uniform"] = round(med["owners_lds"] / med["owners_uniform"], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--inner", type=int, default=10, help="calls per timed window")
    ap.add_argument("--counts", type=int, nargs="*", default=list(COUNTS), help="objects per world")
    ap.add_argument("--out", default="", help="write the JSON object to this file")
    args = ap.parse_args()
    import torch
    worlds = [run_world(n, args.warmup, args.rounds, args.inner) for n in args.counts]
    out = dict(shape="%dx%dx1, first sample per pixel" % (WIDTH, HEIGHT), warmup=args.warmup, rounds=args.rounds,
               calls_per_window=args.inner, device=torch.cuda.get_device_name(0), worlds=worlds)
    text = json.dumps(out, indent=1)
    print(text, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
