"""What tests/test_select_edges_host.py and tests/test_gpu_select_edges.py share: the cases of tests/golden/select_edges.npz
(the real reference's chunk selection where one ulp of the distance is a whole LOD; tests/golden/make_select_edges.py) as
dense worlds, the known answers of tests/golden/kat_dist.json.gz (CPython's math.dist; tests/golden/make_kat_dist.py), and the
bracket that reads a distance out of a selection: with chunk_lod = 1 and dist_max = 2 T the step is exactly T, so a chunk's
LOD is 1 exactly when its distance is >= T; the two thresholds T = want and T = nextafter(want, inf) pin
want <= dist < nextafter(want, inf), that is dist == want.  Numpy and the oracle only: nothing here needs a GPU."""
import gzip
import json
import math
import os

import numpy as np

import oracle_lib as ol

KAT_CS = 8              # every KAT centre the device can be asked about is the centre of a chunk of this size
LIMIT = 1 << 28         # vrt_select_chunks accepts worlds inside +-2^28


class Case:
    """One case of select_edges.npz as a dense world box: origin, dims, present [dims]; want_present / want_res [dims] as
    ol.select_chunks returns them (res = LOD + 1 where kept, else 0)."""

    def __init__(self, z, i):
        self.name = str(z["names"][i])
        self.cs, self.dist_max, self.chunk_lod, culling = (int(v) for v in z["settings"][i])
        self.culling = bool(culling)
        self.cam = z["cam"][i].astype(np.float64)
        a, b = int(z["chunk_start"][i]), int(z["chunk_start"][i + 1])
        self.chunks, kept, lod = z["chunks"][a:b], z["kept"][a:b], z["lod"][a:b]
        self.trav = z["trav"][int(z["trav_start"][i]):int(z["trav_start"][i + 1])].astype(np.float64).reshape(-1, 3)
        self.origin = self.chunks.min(0)
        self.dims = (self.chunks.max(0) - self.origin) // self.cs + 1
        self.cells = (self.chunks - self.origin) // self.cs
        self.present = np.zeros(tuple(self.dims), np.uint8)
        self.want_present, self.want_res = np.zeros_like(self.present), np.zeros_like(self.present)
        for c, k, l in zip(self.cells, kept, lod):
            self.present[tuple(c)] = 1
            self.want_present[tuple(c)] = k
            self.want_res[tuple(c)] = (l + 1) if k else 0

    def naive_res(self):
        """want_res's counterpart under sqrt(dx*dx + dy*dy + dz*dz), separately rounded operations, in numpy."""
        d = (self.chunks + round(self.cs / 2)).astype(np.float64) - self.cam
        dist = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
        lod = np.minimum(np.trunc(dist / (self.dist_max / (1 + self.chunk_lod))), self.chunk_lod).astype(np.uint8)
        out = np.zeros_like(self.want_res)
        for c, l in zip(self.cells, lod):
            out[tuple(c)] = (l + 1) if self.want_present[tuple(c)] else 0
        return out

    def oracle(self):
        return ol.select_chunks(self.origin, self.dims, self.cs, self.present, self.cam, self.dist_max, self.chunk_lod,
                                self.culling, self.trav)


_fixture = {}


def edge_cases():
    """(cases, recorded flip pairs): loaded once, shared, never modified."""
    if not _fixture:
        z = np.load(os.path.join(ol.GOLDEN, "select_edges.npz"))
        _fixture["cases"] = [Case(z, i) for i in range(len(z["names"]))]
        _fixture["flips"] = (z["flip_case"].astype(int), z["flip_dir"].astype(int), int(z["flips_up"]), int(z["flips_down"]))
    return _fixture["cases"], _fixture["flips"]


def kat_dist():
    """{family: float64 [n, 7]} of kat_dist.json.gz: centre, camera, math.dist of the generating CPython."""
    if "kat" not in _fixture:
        with gzip.open(os.path.join(ol.GOLDEN, "kat_dist.json.gz"), "rt") as f:
            kat = json.load(f)
        _fixture["kat"] = {k: np.array([[float.fromhex(v) for v in r] for r in recs], np.float64) for k, recs in kat["vectors"].items()}
    return _fixture["kat"]


def on_chunk_grid(vec):
    """Whether a KAT vector's centre is the centre of a chunk of size KAT_CS inside the box vrt_select_chunks accepts."""
    c = vec[:3]
    return bool(np.all(c == np.floor(c)) and np.all((c - KAT_CS // 2) % KAT_CS == 0) and np.all(np.abs(c) + KAT_CS <= LIMIT))


def thresholds(want):
    """The bracket's thresholds T with the LOD each must give a chunk whose distance is `want`: (T, dist_max = 2 T, lod)."""
    up = math.nextafter(want, math.inf)
    return ([(want, 2.0 * want, 1)] if want > 0.0 else []) + [(up, 2.0 * up, 0)]


def bracket_by(select, vec):
    """Put vec's distance question to `select(origin, cam, dist_max) -> LOD of the one chunk at origin` (chunk size KAT_CS,
    chunk_lod 1, culling off).  Returns whether both thresholds answer that the distance is exactly vec[6]."""
    origin = [int(v) - KAT_CS // 2 for v in vec[:3]]
    return all(select(origin, vec[3:6], dist_max) == lod for _, dist_max, lod in thresholds(float(vec[6])))


def oracle_select_one(origin, cam, dist_max):
    pres, res = ol.select_chunks(origin, [1, 1, 1], KAT_CS, np.ones((1, 1, 1), np.uint8), cam, dist_max, 1, False, np.zeros((0, 3)))
    assert pres[0, 0, 0] == 1
    return int(res[0, 0, 0]) - 1
