#!/usr/bin/env python3
"""Generate tests/golden/kat_dist.json.gz: known answers of CPython's math.dist on chunk-centre / camera pairs.

Own code, no reference needed: the reference's vec3.distance is math.dist (lib.py:297-298), and the chunk LOD is trunc() of
a multiple of it (init.py:448-449).  math.dist is not sqrt(dx*dx + dy*dy + dz*dz): it scales, accumulates the squares in
extended precision and corrects the root.  The file pins what the generating interpreter returns, so that the tests never
ask the running interpreter (another CPython may compute another math.dist).

Each vector is [cx, cy, cz, px, py, pz, value] as hex floats (the style of kat_math.json): a chunk centre, a camera position
and math.dist(centre, camera).  Families (the keys of "vectors"):
  integer     integer chunk centres (chunk size 8: 8 k + 4) against random float cameras
  far         worlds 2^24 .. 2^28 cells out with mixed signs: large coordinates cancel in the differences
  exact       cameras on integers and on .5: every square and every sum is exact
  pythagorean integer differences whose distance is an integer
  boundary    cameras within +-6 ulps of the x at which the distance is k * step for the steps 16 (= 48 / 3 = 64 / 4),
              192 / 6 and 1000 / 6: where an ulp of the distance is a whole LOD
  tiny        a camera inside its chunk's centre cell: differences below 1, zero components, the camera on the centre,
              one ulp off it, and -- about a centre at 0, which no chunk of size >= 8 has: for the CPU only -- 1e-300-sized
              and subnormal differences
Every centre but those of the last kind is the centre of a chunk of size 8 inside the +-2^28 box vrt_select_chunks accepts,
so the GPU test can put the question to the kernel itself.

The generator asserts that the naive formula misses at least 10 % of the vectors.

The JSON is some 350 KB of hex digits on one line, which nobody reads and which swamps a diff, so it is stored gzipped (level 9,
no name, no time stamp: the same bytes on every run); gzip.open(path, "rt") gives json.load the text.

Usage:  python tests/golden/make_kat_dist.py
"""
import gzip
import json
import math
import os
import platform
import random

OUT = os.path.dirname(os.path.abspath(__file__))
SEED = 20261020
LIMIT = 1 << 28


def naive(c, p):
    dx, dy, dz = c[0] - p[0], c[1] - p[1], c[2] - p[2]
    return math.sqrt(dx * dx + dy * dy + dz * dz)


def centre(rng, lo, hi):
    """A chunk centre 8 k + 4 with lo <= |centre| < hi on a random sign."""
    c = rng.randrange(lo, hi)
    c = (c // 8) * 8 + 4
    c = min(c, LIMIT - 4)
    return float(c if rng.random() < 0.5 else -c)


def ulps(x, n):
    for _ in range(abs(n)):
        x = math.nextafter(x, math.inf if n > 0 else -math.inf)
    return x


def families():
    rng = random.Random(SEED)
    fam = {k: [] for k in ("integer", "far", "exact", "pythagorean", "boundary", "tiny")}

    for _ in range(500):
        c = [centre(rng, 0, 320) for _ in range(3)]
        fam["integer"].append((c, [rng.uniform(-320, 320) for _ in range(3)]))

    for _ in range(400):
        e = rng.choice([24, 25, 26, 27])
        c = [centre(rng, 1 << e, 1 << (e + 1)) for _ in range(3)]
        if rng.random() < 0.25:          # one axis near the origin: differences of very different sizes
            c[rng.randrange(3)] = centre(rng, 0, 64)
        fam["far"].append((c, [v + rng.uniform(-200, 200) for v in c]))

    for _ in range(250):
        c = [centre(rng, 0, 1 << rng.choice([6, 10, 24])) for _ in range(3)]
        fam["exact"].append((c, [v + rng.randrange(-400, 401) / 2 for v in c]))

    quads = [(3, 4, 0, 5), (1, 2, 2, 3), (2, 3, 6, 7), (1, 4, 8, 9), (4, 4, 7, 9), (2, 6, 9, 11), (6, 6, 7, 11), (3, 4, 12, 13),
             (2, 10, 11, 15), (8, 9, 12, 17), (1, 12, 12, 17), (12, 15, 16, 25)]
    for _ in range(150):
        q = rng.choice(quads)
        assert q[0] ** 2 + q[1] ** 2 + q[2] ** 2 == q[3] ** 2
        m = rng.choice([1, 2, 4, 8, 16, 3, 5, 0.5, 0.25])
        d = [v * m * rng.choice([-1, 1]) for v in q[:3]]
        rng.shuffle(d)
        c = [centre(rng, 0, 1 << rng.choice([6, 10, 20])) for _ in range(3)]
        fam["pythagorean"].append((c, [v - w for v, w in zip(c, d)]))

    while len(fam["boundary"]) < 40 * 13:
        step = rng.choice([16.0, 48 / 3, 64 / 4, 192 / 6, 1000 / 6])
        r = rng.randrange(1, 6) * step
        c = [centre(rng, 0, 1024) for _ in range(3)]
        py, pz = c[1] + rng.uniform(-0.6, 0.6) * r, c[2] + rng.uniform(-0.6, 0.6) * r
        rest = r * r - (c[1] - py) ** 2 - (c[2] - pz) ** 2
        if rest <= 0:
            continue
        x0 = c[0] - math.sqrt(rest)
        for n in range(-6, 7):
            fam["boundary"].append((c, [ulps(x0, n), py, pz]))

    for k in range(160):
        c = [centre(rng, 0, 1 << rng.choice([4, 8, 24])) for _ in range(3)]
        d = [rng.uniform(-1, 1) for _ in range(3)]
        if k % 4 == 1:
            d[rng.randrange(3)] = 0.0
        if k % 4 == 2:
            d = [0.0, 0.0, 0.0]
            d[rng.randrange(3)] = rng.uniform(-1, 1)
        p = [v + w for v, w in zip(c, d)]
        if k % 8 == 3:
            p = [ulps(v, rng.choice([-1, 0, 1])) for v in c]
        if k % 16 == 7:
            p = list(c)
        fam["tiny"].append((c, p))
    for _ in range(40):                 # about 0: only here can a difference be smaller than an ulp of a chunk centre
        size = rng.choice([1e-300, 1e-300, 1e-160, 3e-308, 1e-310, 5e-324 * 1000])
        p = [rng.uniform(-1, 1) * size for _ in range(3)]
        if rng.random() < 0.3:
            p[rng.randrange(3)] = 0.0
        fam["tiny"].append(([0.0, 0.0, 0.0], p))
    return fam


def main():
    fam = families()
    out, n, missed, per = {}, 0, 0, {}
    for name, pairs in fam.items():
        recs = []
        for c, p in pairs:
            want = math.dist(c, p)
            recs.append([float(v).hex() for v in c + p] + [want.hex()])
            missed += naive(c, p) != want
            per[name] = per.get(name, 0) + (naive(c, p) != want)
        n += len(recs)
        out[name] = recs
    print("kat_dist: %d vectors, the naive formula misses %d (%s)" % (n, missed, per))
    assert n >= 1900 and missed >= n // 10, (n, missed)
    assert any(v == (0.0).hex() for r in out["tiny"] for v in r[6:]), "no zero distance"
    text = json.dumps(dict(cpython=platform.python_version(), seed=SEED, naive_misses=missed, vectors=out))
    path = os.path.join(OUT, "kat_dist.json.gz")
    with open(path, "wb") as f, gzip.GzipFile(filename="", mode="wb", compresslevel=9, fileobj=f, mtime=0) as g:
        g.write(text.encode("ascii"))
    print("  -> kat_dist.json.gz (%d bytes of JSON, %d on disk)" % (len(text), os.path.getsize(path)))


if __name__ == "__main__":
    main()
