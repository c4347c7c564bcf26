#!/usr/bin/env python3
"""Generate tests/golden/run_flags.npz: bodies whose distance to the camera is one of the limits of the run's flags, the double
below it or the double above it (the scene of tests/physics_flags_scene.py).

Own code, no reference needed: the reference's vec3.distance is math.dist (lib.py:297-298), Object.update compares it with
dist_max + max(size) for visibility and with dist_move for physics (data.py:564-585), and like make_kat_dist.py this file pins
what the generating interpreter's math.dist returns, so that the tests never ask the running one.

Body i: kind i % 3 (a 2^3 sprite, a 4 x 2 x 6 sprite, none), outcome (i // 3) % 3 (the distance IS the limit, is the double
below it, the double above it), and for a body with a sprite the limit (i // 9) % 2 (dist_move, or dist_max + max(half)); a body
without a sprite is never visible and stands at dist_move.  Every kind, outcome and limit so occurs on both sides of index 1024.
The body starts on the sphere of its limit about the camera, in a random direction whose x component is between 0.15 and 0.5;
then x is searched ulp by ulp for the positions at which math.dist(pos, cam) is exactly the wanted double.  Several are: an ulp
of x is a fraction of an ulp of the distance.  Among them the first is taken at which sqrt(dx^2 + dy^2 + dz^2) gives the other
flag, if there is one.

    pos        float64 [1100, 3]
    cam        float64 [3]
    visible    bool [1100]     bool(sprite) and math.dist(pos, cam) <= dist_max + max(half)
    awake      bool [1100]     math.dist(pos, cam) <= dist_move
    naive      bool [1100]     the plain square root gives another visible or another awake
    spec       JSON: n, dist_move, dist_max, cam, up (the followed body's attachment), kinds, half

The file is written only if the plain square root gives the other flag for at least 10 % of the bodies (the share
make_kat_dist.py demands), every outcome was found for every body, and (cam - up) + up is cam exactly.

Usage:  python tests/golden/make_run_flags.py
"""
import json
import math
import os
import platform
import random
import sys

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(OUT))
SEED = 20265
SEARCH = 400     # ulps of x searched on either side of the analytic root


def naive(p, c):
    dx, dy, dz = p[0] - c[0], p[1] - c[1], p[2] - c[2]
    return math.sqrt(dx * dx + dy * dy + dz * dz)


def flags(dist, kind, fs):
    return bool(kind) and dist <= fs.DIST_MAX + fs.HALF[kind], dist <= fs.DIST_MOVE


def main():
    import physics_flags_scene as fs
    import make_physics as mp
    rng = random.Random(SEED)
    cam = fs.CAM
    assert (cam[1] - fs.UP) + fs.UP == cam[1]
    pos, visible, awake, other = [], [], [], []
    per = {}
    for i in range(fs.N):
        kind, outcome = fs.KINDS[i % 3], (i // 3) % 3
        limit = float(fs.DIST_MAX + fs.HALF[kind]) if kind and (i // 9) % 2 else float(fs.DIST_MOVE)
        want = (limit, math.nextafter(limit, 0.0), math.nextafter(limit, math.inf))[outcome]
        while True:
            u = [rng.gauss(0, 1) for _ in range(3)]
            n = math.sqrt(sum(c * c for c in u))
            u = [c / n for c in u]
            if 0.15 <= abs(u[0]) <= 0.5:
                break
        y, z = cam[1] + limit * u[1], cam[2] + limit * u[2]
        x0 = cam[0] + math.copysign(math.sqrt(limit * limit - (y - cam[1]) ** 2 - (z - cam[2]) ** 2), u[0])
        found = []
        for step in (math.inf, -math.inf):
            x = x0
            for _ in range(SEARCH):
                if math.dist((x, y, z), cam) == want:
                    found.append(x)
                x = math.nextafter(x, step)
        assert found, "body %d: no x within %d ulps puts it at %r" % (i, SEARCH, want)
        true = flags(want, kind, fs)
        wrong = [x for x in found if flags(naive((x, y, z), cam), kind, fs) != true]
        x = (wrong or found)[0]
        p = (x, y, z)
        assert math.dist(p, cam) == want
        pos.append(p), visible.append(true[0]), awake.append(true[1]), other.append(bool(wrong))
        key = (kind, outcome, limit, i >= 1024)
        per[key] = per.get(key, 0) + 1
    # every kind at every outcome of every limit it has, on both sides of index 1024
    cases = {(k, o, float(l), side) for k in fs.KINDS for o in range(3) for side in (False, True)
             for l in ([fs.DIST_MOVE, fs.DIST_MAX + fs.HALF[k]] if k else [fs.DIST_MOVE])}
    assert set(per) == cases, sorted(cases - set(per), key=str)
    missed = sum(other)
    print("run_flags: %d bodies, the plain square root gives the other flag for %d; %d visible, %d awake (CPython %s)"
          % (fs.N, missed, sum(visible), sum(awake), platform.python_version()))
    assert missed >= fs.N // 10, (missed, fs.N)
    spec = dict(n=fs.N, dist_move=fs.DIST_MOVE, dist_max=fs.DIST_MAX, cam=cam, up=fs.UP, kinds=list(fs.KINDS), half=[fs.HALF[k] for k in fs.KINDS])
    out = dict(pos=np.array(pos, np.float64), cam=np.array(cam, np.float64), visible=np.array(visible, bool), awake=np.array(awake, bool),
               naive=np.array(other, bool), spec=np.frombuffer(json.dumps(spec).encode(), np.uint8))
    if mp.unchanged(fs.PATH, out):
        print(os.path.relpath(fs.PATH, OUT), "unchanged")
        return
    np.savez_compressed(fs.PATH, **out)
    print(os.path.relpath(fs.PATH, OUT), os.path.getsize(fs.PATH), "bytes")


if __name__ == "__main__":
    main()
