#!/usr/bin/env python3
"""Generate tests/golden/edges/*.npz: the edge scenes and the boundary-camera scene of tests/edge_scenes.py rendered by the
*real* reference.

Needs the reference checkout make_golden.py needs and runs only where that is; the test-suite reads the committed output and
never imports this script.  Nothing of the reference is copied: its modules are imported in place
(make_golden.load_reference), its Camera.tile is driven under make_golden's instrumentation and observed.

For every camera of every EDGE_CASES entry, for `no_background` (data.background = None, restored afterwards) and for the 14
boundary renders the script builds reference Materials and Frames from the scene -- one unpacked Frame of the chunk's
resolution r per present chunk, data3[p // r] for every voxel p of the scene's camera grid --, sets data.settings through
set_config, asserts that the reference's `proportions` and `chunk_radius` are ours, runs Camera.tile(0, 0) and writes

    settings        the settings JSON (make_golden.settings_dict)
    has_background  1 | 0
    cam_pos, cam_rot (x, y, z, w), cam_lens
    scene_sha256    edge_scenes.scene_sha256 over origin, dims, present, res, camera grid, materials: the scene itself is not
                    stored, the tests rebuild it from tests/edge_scenes.py and fail on another hash
    pix_mean        [height, width, 4] float64, as handed to Surface.set_at
    traversed_t0    the tile's traversed list, in order
    counters_total, counter_names, n_rays
    rays, ray_fields                        the FULL cases: every field of every ray (make_golden.RAY_F)
    ray_rgba, ray_energy, ray_counters      the others: x, y, s, r, g, b, alpha (int32), energy, the eight event counters (int32)
    ray_extra, ray_extra_fields             ... and, for the three of them whose proof of reaching the edge reads a field more
                                            (edge_scenes.edge_proof: EXTRA), those columns as float64

Every file stays below the largest fixture committed before these (MAX_FILE) and all of them together below MAX_TOTAL; the
script refuses to finish otherwise (demote cases from the end of FULL).  A second run reproduces every array bit for bit
(--check compares a fresh run with the committed files instead of writing).

Usage:  python tests/golden/make_golden_edges.py [--only NAME ...] [--check]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "edges")
sys.path.insert(0, os.path.dirname(HERE))     # tests/: edge_scenes, oracle_lib (its pure-numpy parts only)

from make_golden import RAY_F, Counters, instrument, load_reference, set_config, settings_dict  # noqa: E402

# the cases whose edge lives in double fields keep every field of every ray (first camera); in order of preference
FULL = ["far_pos", "far_neg", "limit_28_pos", "limit_28_neg", "res9", "fov179", "bounces16", "dof10", "rough25_abs7", "cs64"]
# compact cases whose edge_proof reads fields the compact form does not have
EXTRA = {"bounces_half": ["bounces"], "lod_full": ["life", "detail"], "near4": ["life", "detail"]}
MAX_FILE = 842566          # bytes: the largest fixture committed before these (render_c3_96.npz)
MAX_TOTAL = 3 * 1000 * 1000


def reference_chunks(data, sc, mats):
    """{chunk position: Frame} as Camera.chunks holds them, from a dense oracle_lib.Scene."""
    cs = sc.chunk_size
    chunks = {}
    for c in np.argwhere(sc.present != 0):
        r = int(sc.res[tuple(c)])
        lo = sc.origin + c * cs
        fr = data.Frame(packed=False, resolution=r)
        block = sc.grid[c[0] * cs:(c[0] + 1) * cs, c[1] * cs:(c[1] + 1) * cs, c[2] * cs:(c[2] + 1) * cs]
        for q in np.argwhere(block != 0):
            p = lo + q
            assert not (p % r).any()            # the camera grid keeps multiples of the resolution only
            fr.data3[tuple(int(v) // r for v in p)] = mats[int(block[tuple(q)]) - 1]
        chunks[tuple(int(v) for v in lo)] = fr
    return chunks


def record(data, cam, rays, sc_hash, has_background, full, extra=()):
    """One Camera.tile(0, 0) under the instrumentation, in make_golden.render()'s record layout."""
    s = data.settings
    W, H = s.width, s.height
    rays.clear()
    t0 = time.time()
    surf, traversed, th = cam.tile(0, 0)
    dt = time.time() - t0
    pix = np.full((H, W, 4), np.nan, np.float64)
    for (x, y), c in surf.px.items():
        pix[y, x] = c
    assert not np.isnan(pix).any()
    rec = np.zeros((len(rays), len(RAY_F)), np.float64)
    last, sidx = None, 0
    for i, (dx, dy, detail, ray, cv) in enumerate(rays):
        x = round((dx + 1) / 2 * W)
        y = round((dy + 1) / 2 * H)
        assert -1 + (x / W) * 2 == dx and -1 + (y / H) * 2 == dy
        sidx = sidx + 1 if last == (x, y) else 0
        last = (x, y)
        alpha = round(min(1, ray.energy + s.shutter) * 255)
        rec[i] = [x, y, sidx, detail, ray.color.r, ray.color.g, ray.color.b, alpha, ray.energy, ray.step, ray.life,
                  ray.bounces, ray.pos.x, ray.pos.y, ray.pos.z, ray.vel.x, ray.vel.y, ray.vel.z, len(ray.traversed)] + cv
    nc = len(Counters.FIELDS)
    out = dict(
        settings=np.frombuffer(json.dumps(settings_dict(data)).encode(), np.uint8),
        has_background=np.array([1 if has_background else 0], np.int64),
        cam_pos=np.array([cam.pos.x, cam.pos.y, cam.pos.z], np.float64),
        cam_rot=np.array([cam.rot.x, cam.rot.y, cam.rot.z, cam.rot.w], np.float64),
        cam_lens=np.array([cam.lens], np.float64),
        scene_sha256=np.array(sc_hash),
        pix_mean=pix,
        traversed_t0=np.array([[float(v) for v in p] for p in traversed], np.float64).reshape(-1, 3),
        counters_total=rec[:, -nc:].sum(0).astype(np.int64),
        counter_names=np.array(Counters.FIELDS),
        n_rays=np.array([len(rays)], np.int64),
    )
    if full:
        out["rays"] = rec
        out["ray_fields"] = np.array(RAY_F)
    else:
        out["ray_rgba"] = rec[:, [0, 1, 2, 4, 5, 6, 7]].astype(np.int32)
        out["ray_energy"] = rec[:, 8].copy()
        out["ray_counters"] = rec[:, -nc:].astype(np.int32)
        if extra:
            out["ray_extra"] = rec[:, [RAY_F.index(f) for f in extra]].copy()
            out["ray_extra_fields"] = np.array(list(extra))
    return out, rec, dt


def main():
    ap = argparse.ArgumentParser()                  # (before load_reference(): it overwrites sys.argv and changes directory)
    ap.add_argument("--only", nargs="*", default=None)
    ap.add_argument("--check", action="store_true", help="compare with the committed fixtures instead of writing")
    args = ap.parse_args()
    import edge_scenes as es
    renders = es.reference_renders()
    assert len(renders) == sum(len(es.edge_scene(n)[2]) for n in es.EDGE_CASES) + 1 + 14
    if args.only is not None:
        renders = [r for r in renders if r[0] in args.only]

    t_start = time.time()
    data, lib, mod = load_reference()
    data.objects.clear()
    cnt, rays = Counters(), []
    wrap_material = instrument(data, lib, mod, cnt, rays)
    background = data.background
    os.makedirs(OUT, exist_ok=True)
    built = {}                  # id(scene) -> (chunks, hash): the cameras of a case share their Frames
    sizes, t_render = {}, {}
    for name, sc, st, pos, q, lens, has_bg in renders:
        if id(sc) not in built:
            mats = [data.Material(function=lib.material, albedo=lib.rgb(int(m[0]), int(m[1]), int(m[2])), roughness=float(m[3]),
                                  absorption=float(m[4]), ior=float(m[5]), energy=float(m[6]), solidity=1, weight=0.001,
                                  friction=0.1, elasticity=0.5) for m in sc.materials]
            assert all((m[:3] == np.floor(m[:3])).all() for m in sc.materials)
            for m in mats:
                wrap_material(m)
            built[id(sc)] = (sc, reference_chunks(data, sc, mats), es.scene_sha256(sc))
        _, chunks, sc_hash = built[id(sc)]
        set_config(data, **{k: v for k, v in st.items() if k not in ("proportions", "chunk_radius")})
        s = data.settings
        assert s.proportions == st["proportions"] and s.chunk_radius == st["chunk_radius"], name
        assert s.threads == 1 and s.chunk_size == sc.chunk_size
        cam = mod.Camera()
        cam.chunks = chunks
        cam.pos = lib.vec3(*[float(v) for v in pos])
        cam.rot = lib.quaternion(*[float(v) for v in q])
        cam.lens = float(lens)
        data.background = background if has_bg else None
        try:
            out, rec, dt = record(data, cam, rays, sc_hash, has_bg, name in FULL, EXTRA.get(name, ()))
        finally:
            data.background = background
        F = {k: i for i, k in enumerate(RAY_F)}
        if not has_bg:      # from the reference's output alone: rays did end without a hit, so the missing background shows
            no_hit = int((rec[:, F["c_broke"]] == 0).sum())
            assert no_hit > 0 and int((rec[:, F["c_hit"]] == 0).sum()) > 0, name
            print("  %-18s %d of %d rays ended without a hit" % (name, no_hit, len(rec)))
        path = os.path.join(OUT, "%s.npz" % name)
        if args.check:
            z = np.load(path)
            assert sorted(z.files) == sorted(out), (name, sorted(z.files))
            for k, v in out.items():
                assert z[k].dtype == np.asarray(v).dtype and z[k].tobytes() == np.asarray(v).tobytes(), (name, k)
        else:
            np.savez_compressed(path, **out)
        sizes[name], t_render[name] = os.path.getsize(path), dt
        print("  %-18s %6d rays  %5.2fs  %-7s %7d bytes" % (name, len(rec), dt, "full" if name in FULL else "compact", sizes[name]),
              flush=True)
    total = sum(sizes.values())
    print("%d fixtures%s, %d bytes together, largest %d; reference %.2f..%.2f s per render, %.1f s in all (%.1f s with set-up)"
          % (len(sizes), " checked" if args.check else "", total, max(sizes.values()), min(t_render.values()),
             max(t_render.values()), sum(t_render.values()), time.time() - t_start))
    assert max(sizes.values()) < MAX_FILE, "a fixture is larger than the largest committed before: demote from the end of FULL"
    assert args.only is not None or total < MAX_TOTAL, "the fixtures together exceed the budget: demote from the end of FULL"


if __name__ == "__main__":
    main()
