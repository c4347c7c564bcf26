#!/usr/bin/env python3
"""Generate tests/golden/select_edges.npz: the real reference's chunk selection where one ulp of the distance is a whole LOD.

Needs the reference checkout make_golden.py needs; the test-suite only reads the committed output.  Nothing of the reference
is copied: its modules are imported in place (make_golden.load_reference), small worlds are built from its own Sprite and
Object (one voxel per chunk, next to the chunk's centre), its own Window.chunk_update (init.py:389-452) runs, and what the
camera was given (Camera.chunk_set) is recorded.

Why: the LOD is min(trunc(dist / (dist_max / (1 + chunk_lod))), chunk_lod) with dist = math.dist(chunk centre, camera)
(init.py:448-449, lib.py:297-298).  math.dist is not sqrt(dx*dx + dy*dy + dz*dz); the two differ by an ulp on about one
input in six, and where dist / step lands on an integer that ulp is a LOD.  Random cameras never land there; these do.

Cases (every one: chunk_size, dist_max, chunk_lod, culling; the camera as float64; the traversed list; the world's chunk
positions; per chunk whether the camera got it and at which LOD):
  tie_*       the centres of a row of chunks are exactly 0, 1, .. chunk_lod steps from the camera along one axis (and one
              chunk beyond the last step, which min() caps), for eight settings with chunk sizes 8, 16, 32 and 64, two of
              them 2^24 cells out: with the camera on the tie (LOD k), one ulp nearer (k - 1) and one ulp farther (k).
              Every square and sum is exact here: the naive formula agrees.
  quad_*      exact ties off the axes: differences that are multiples of (1, 2, 2), (3, 4, 0) and (12, 15, 16).
  lod0_*      chunk_lod = 0, a chunk at exactly dist_max among others: trunc() gives 1, min() gives 0.
  flip_*      constructed flips, found by a seeded search: the camera's x is moved by up to +-6 ulps around
              cx - sqrt((k step)^2 - dy^2 - dz^2) for random chunk centres and random float camera y, z, and a pair is
              kept where the naive formula's LOD differs from math.dist's.  SEARCH lists the (chunk_size, dist_max,
              chunk_lod) settings and how many pairs each contributes; (1000, 5) has a step no double holds.  The world of
              a flip case is the chunk and its neighbour.  The search takes what it finds: of its 32 pairs math.dist gives
              the higher LOD in 19 and the lower in 13 (`flip_dir`, +1 / -1); no direction is forced.
  cull_*      culling on: tie and flip worlds again with a traversed list that holds some of the boundary chunks, leaves
              others out and names positions outside the world.

The generator asserts its own coverage: at least 24 flips over at least three settings with (1000, 5) among them, each one
confirmed by the reference itself (its LOD is math.dist's, not the naive one); kept and dropped chunks under culling; every
LOD from 0 to chunk_lod in the tie worlds.

Usage:  python tests/golden/make_select_edges.py
"""
import math
import os
import platform
import random

import numpy as np

from make_golden import load_reference, set_config

OUT = os.path.dirname(os.path.abspath(__file__))
SEED = 4849
# chunk_size, dist_max, chunk_lod, pairs wanted, draws allowed
SEARCH = [(8, 16, 1, 4, 4000), (8, 48, 2, 8, 4000), (16, 64, 3, 6, 4000), (32, 192, 5, 6, 4000), (8, 1000, 5, 8, 8000)]
# chunk_size, dist_max, chunk_lod, axis, base coordinate of the camera on that axis (a multiple of 64)
TIES = [(8, 48, 2, 0, -4096), (8, 64, 3, 1, 4096), (16, 192, 5, 2, -4096), (8, 16, 1, 0, 4096), (8, 1000, 4, 1, -4096),
        (64, 256, 3, 2, 4096), (32, 192, 5, 0, 1 << 24), (16, 48, 2, 1, -(1 << 24))]


def ulps(x, n):
    for _ in range(abs(n)):
        x = math.nextafter(x, math.inf if n > 0 else -math.inf)
    return x


def lod_of(dist, dist_max, chunk_lod):
    return min(math.trunc(dist / (dist_max / (1 + chunk_lod))), chunk_lod)


def naive_dist(c, p):
    dx, dy, dz = c[0] - p[0], c[1] - p[1], c[2] - p[2]
    return math.sqrt(dx * dx + dy * dy + dz * dz)


def post_of(centre, cs):
    assert all((int(v) - cs // 2) % cs == 0 for v in centre), (centre, cs)
    return tuple(int(v) - cs // 2 for v in centre)


def search_flips():
    """[(cs, dist_max, chunk_lod, centre, camera, direction)]: pairs whose naive LOD is not math.dist's."""
    rng = random.Random(SEED)
    found = []
    for cs, dist_max, chunk_lod, want, draws in SEARCH:
        step = dist_max / (1 + chunk_lod)
        got = 0
        for _ in range(draws):
            if got == want:
                break
            r = rng.randrange(1, chunk_lod + 1) * step
            # the camera's x is as large as the distance, so that an ulp of it moves the distance by about an ulp
            c = [(rng.randrange(int(2 * r), int(8 * r)) // cs * cs + cs // 2) * rng.choice([-1, 1]),
                 rng.randrange(-256, 256) // cs * cs + cs // 2, rng.randrange(-256, 256) // cs * cs + cs // 2]
            py, pz = c[1] + rng.uniform(-0.6, 0.6) * r, c[2] + rng.uniform(-0.6, 0.6) * r
            rest = r * r - (c[1] - py) ** 2 - (c[2] - pz) ** 2
            if rest <= 0:
                continue
            x0 = c[0] - math.sqrt(rest) * rng.choice([-1, 1])
            for n in range(-6, 7):
                p = [ulps(x0, n), py, pz]
                a, b = lod_of(math.dist(c, p), dist_max, chunk_lod), lod_of(naive_dist(c, p), dist_max, chunk_lod)
                if a != b:
                    found.append((cs, dist_max, chunk_lod, c, p, 1 if a > b else -1))
                    got += 1
                    break
        assert got == want, ("search budget", cs, dist_max, chunk_lod, got)
    return found


def main():
    data, lib, mod = load_reference()
    s = data.settings
    mat = data.Material(function=lib.material, albedo=lib.rgb(255, 0, 0), roughness=0.5, absorption=1.0, ior=1.0, energy=0.0,
                        solidity=1, weight=0.001, friction=0.1, elasticity=0.5)
    cases = []

    def run(name, cs, dist_max, chunk_lod, culling, cam_pos, chunks, traversed=()):
        """Build the world `chunks` (chunk positions) in the reference, select for the camera, record."""
        data.objects.clear()
        set_config(data, width=8, height=8, samples=1, threads=1, dist_max=dist_max, dist_min=0, chunk_size=cs, chunk_lod=chunk_lod)
        s.culling = culling
        cam = mod.Camera()
        cam.pos = lib.vec3(*[float(v) for v in cam_pos])
        cam.rot = lib.quaternion(0, 0, 0, 1)
        for post in chunks:
            spr = data.Sprite(size=lib.vec3(2, 2, 2), frames=1, lod=0)
            spr.get_frame(0).set_voxels({(0, 0, 0): mat}, True)
            ob = data.Object(pos=lib.vec3(*[int(v) + cs // 2 for v in post]), rot=lib.vec3(0, 0, 0), vel=lib.vec3(0, 0, 0), physics=False)
            ob.set_sprite(spr)
            ob.update(cam.pos)
            assert ob.visible, (name, post)
        win = lib.store(timer=0, traversed=[[tuple(int(v) for v in t) for t in traversed]], chunks={}, chunks_objects={}, cam=cam)
        mod.Window.chunk_update(win, 1.0)
        assert set(win.chunks) == {tuple(int(v) for v in p) for p in chunks}, (name, sorted(win.chunks), chunks)
        kept = [tuple(p) in cam.chunks for p in chunks]
        lod = [cam.chunks[tuple(p)].resolution - 1 if k else 0 for p, k in zip(chunks, kept)]
        assert (cam.pos.x, cam.pos.y, cam.pos.z) == tuple(float(v) for v in cam_pos)
        cases.append(dict(name=name, settings=(cs, dist_max, chunk_lod, int(culling)), cam=[float(v) for v in cam_pos],
                          chunks=[tuple(int(v) for v in p) for p in chunks], kept=kept, lod=lod,
                          trav=[tuple(int(v) for v in t) for t in traversed]))
        return cases[-1]

    # ---- exact ties on an axis, one ulp nearer, one ulp farther ------------------------------------------------------
    tie_worlds = []
    for cs, dist_max, chunk_lod, axis, base in TIES:
        step = dist_max / (1 + chunk_lod)
        assert step == int(step) and int(step) % cs == 0
        cam0 = [cs // 2 + 64, cs // 2 - 128, cs // 2]
        cam0[axis] = base + cs // 2
        offs = [k * int(step) for k in range(chunk_lod + 1)]
        if offs[-1] + cs <= dist_max:
            offs.append(offs[-1] + cs)          # beyond the last step: min() caps it
        chunks = []
        for o in offs:
            c = list(cam0)
            c[axis] += o
            chunks.append(post_of(c, cs))
        tie_worlds.append((cs, dist_max, chunk_lod, axis, cam0, chunks))
        for tag, n in (("on", 0), ("near", 1), ("far", -1)):   # the chunks lie towards +axis: +1 ulp is nearer
            cam = list(cam0)
            cam[axis] = ulps(float(cam[axis]), n)
            rec = run("tie_%s_cs%d_%d_%d" % (tag, cs, dist_max, chunk_lod), cs, dist_max, chunk_lod, False, cam, chunks)
            ks = list(range(chunk_lod + 1)) + [chunk_lod] * (len(offs) - chunk_lod - 1)
            want = [max(k - 1, 0) if n == 1 and k * step == o else k for k, o in zip(ks, offs)]
            assert all(rec["kept"]) and rec["lod"] == want, (rec["name"], rec["lod"], want)
            assert set(rec["lod"]) == set(range(chunk_lod + (0 if n == 1 and len(offs) == chunk_lod + 1 else 1))), rec
            for c, l in zip(chunks, rec["lod"]):     # exact sums: the naive formula agrees
                assert lod_of(naive_dist([v + cs // 2 for v in c], cam), dist_max, chunk_lod) == l

    # ---- exact ties off the axes ----------------------------------------------------------------------------------------
    for cs, dist_max, chunk_lod, k, d in [(8, 64, 3, 3, (16, 32, 32)), (16, 192, 5, 3, (-64, 32, 64)), (16, 192, 5, 5, (96, 0, -128)),
                                          (8, 1000, 4, 1, (96, -120, 128)), (8, 1000, 4, 2, (-240, 320, 0)), (8, 1000, 4, 3, (400, 400, -200)),
                                          (8, 1000, 4, 4, (384, 480, 512))]:
        assert math.isqrt(sum(v * v for v in d)) ** 2 == sum(v * v for v in d) and math.isqrt(sum(v * v for v in d)) * (1 + chunk_lod) == k * dist_max
        cam = [cs // 2 - 40 * cs, cs // 2 + 24 * cs, cs // 2]
        c = [a + b for a, b in zip(cam, d)]
        chunks = [post_of(c, cs), post_of([c[0] + cs, c[1], c[2]], cs)]
        rec = run("quad_cs%d_%d_%d_k%d" % (cs, dist_max, chunk_lod, k), cs, dist_max, chunk_lod, False, cam, chunks)
        assert rec["kept"][0] and rec["lod"][0] == k, rec

    # ---- chunk_lod = 0 -----------------------------------------------------------------------------------------------
    cam = [4.0, 4.0, 4.0]
    chunks = [post_of(c, 8) for c in ([4, 4, 4], [52, 4, 4], [4, -28, 4], [36, 36, 4], [-44, 4, 4])]
    rec = run("lod0_cs8_48", 8, 48, 0, False, cam, chunks)
    assert all(rec["kept"]) and rec["lod"] == [0] * 5
    rec = run("lod0_off_cs8_48", 8, 48, 0, False, [4.25, 3.5, 4.0 + 2.0 ** -40], chunks)
    assert all(rec["kept"]) and rec["lod"] == [0] * 5

    # ---- constructed flips ---------------------------------------------------------------------------------------------
    flips = search_flips()
    flip_case, flip_dir = [], []
    for i, (cs, dist_max, chunk_lod, c, p, direction) in enumerate(flips):
        chunks = [post_of(c, cs), post_of([c[0] + (cs if c[0] > p[0] else -cs), c[1], c[2]], cs)]   # neighbour: away from the camera
        rec = run("flip%02d_cs%d_%d_%d" % (i, cs, dist_max, chunk_lod), cs, dist_max, chunk_lod, False, p, chunks)
        ref, naive = rec["lod"][0], lod_of(naive_dist(c, p), dist_max, chunk_lod)
        assert rec["kept"][0] and ref == lod_of(math.dist(c, p), dist_max, chunk_lod) and ref - naive == direction, (rec, naive)
        flip_case.append(len(cases) - 1)
        flip_dir.append(direction)
    settings = {f[:3] for f in flips}
    assert len(flips) >= 24 and len(settings) >= 3 and (8, 1000, 5) in settings
    up, down = flip_dir.count(1), flip_dir.count(-1)

    # ---- culling on ---------------------------------------------------------------------------------------------------
    for j, (cs, dist_max, chunk_lod, axis, cam0, chunks) in enumerate(tie_worlds[:4] + tie_worlds[6:7]):
        for tag, n in (("on", 0), ("near", 1)):
            cam = list(cam0)
            cam[axis] = ulps(float(cam[axis]), n)
            trav = [c for k, c in enumerate(chunks) if (k + j) % 2] + [(chunks[0][0] - cs, chunks[0][1], chunks[0][2]),
                                                                       (chunks[0][0], chunks[0][1] + 40 * cs, chunks[0][2])]
            rec = run("cull_tie_%s_cs%d_%d_%d" % (tag, cs, dist_max, chunk_lod), cs, dist_max, chunk_lod, True, cam, chunks, trav)
            assert rec["kept"] == [bool((k + j) % 2) for k in range(len(chunks))]
    for i in (0, 5, 13, 19, 26, 31):
        cs, dist_max, chunk_lod, c, p, direction = flips[i]
        chunks = cases[flip_case[i]]["chunks"]
        for tag, trav in (("in", [chunks[0], (chunks[0][0], chunks[0][1] - cs, chunks[0][2])]), ("out", [chunks[1]])):
            rec = run("cull_flip%02d_%s" % (i, tag), cs, dist_max, chunk_lod, True, p, chunks, trav)
            assert rec["kept"] == [tag == "in", tag == "out"]
            if tag == "in":
                assert rec["lod"][0] == cases[flip_case[i]]["lod"][0]
                flip_case.append(len(cases) - 1)
                flip_dir.append(direction)
    culled = [c for c in cases if c["settings"][3]]
    assert any(k for c in culled for k in c["kept"]) and any(not k for c in culled for k in c["kept"])
    assert {l for c in cases for l, k in zip(c["lod"], c["kept"]) if k} == set(range(6))

    n_chunks = sum(len(c["chunks"]) for c in cases)
    print("select_edges: %d cases, %d chunks, %d flips found (%d up, %d down) over %d settings, %d flip pairs recorded"
          % (len(cases), n_chunks, len(flips), up, down, len(settings), len(flip_case)))
    assert (up, down) == (19, 13), "restate the docstring's flip directions"
    path = os.path.join(OUT, "select_edges.npz")
    np.savez_compressed(
        path, cpython=np.array(platform.python_version()), names=np.array([c["name"] for c in cases]),
        settings=np.array([c["settings"] for c in cases], np.int64), cam=np.array([c["cam"] for c in cases], np.float64),
        chunk_start=np.cumsum([0] + [len(c["chunks"]) for c in cases]).astype(np.int64),
        chunks=np.array([p for c in cases for p in c["chunks"]], np.int64).reshape(-1, 3),
        kept=np.array([k for c in cases for k in c["kept"]], np.uint8), lod=np.array([l for c in cases for l in c["lod"]], np.uint8),
        trav_start=np.cumsum([0] + [len(c["trav"]) for c in cases]).astype(np.int64),
        trav=np.array([t for c in cases for t in c["trav"]], np.int64).reshape(-1, 3),
        flip_case=np.array(flip_case, np.int64), flip_dir=np.array(flip_dir, np.int8), flips_up=np.int64(up), flips_down=np.int64(down))
    print("  -> select_edges.npz (%d bytes)" % os.path.getsize(path))


if __name__ == "__main__":
    main()
