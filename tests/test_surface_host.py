"""The surface pass without a GPU: the C ABI's new record and symbol, what vrt_hit_surfaces refuses before any HIP call, the
restated rule (tests/surface_ref.py) against shade_ref.trace -- which tests/test_shade_host.py pins to the oracle -- run to the
step after each ray's first hit, the normal's definition on hand-built walls, and the compiler's resource report of
python_raytracer_amd/csrc/vrt_surface.hip against the saved one (tests/surface_report.py)."""
import collections
import ctypes as C
import os
import re

import numpy as np
import pytest

import kernel_report
import oracle_lib as ol
import owner_ref as orf
import shade_ref as sr
import surface_ref as sf
import surface_report
from python_raytracer_amd import _native as nat

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vrt.h")


# ---- 1. the C ABI ----------------------------------------------------------------------------------------------------------
def test_symbols_and_layout():
    text = open(HEADER).read()
    assert re.search(r"typedef struct vrt_surface \{[^}]*double  vel\[3\];[^}]*double  next\[3\];[^}]*int8_t  normal\[3\];[^}]*"
                     r"int8_t  status;[^}]*uint8_t neighbour\[3\];[^}]*uint8_t resolution;[^}]*uint8_t reflect;[^}]*uint8_t side;[^}]*"
                     r"uint8_t fetched;[^}]*uint8_t open;[^}]*uint8_t pad\[4\];[^}]*\} vrt_surface;", text, re.S)
    assert re.search(r"int vrt_hit_surfaces\(const vrt_scene\* scene, const vrt_hit\* d_hits, const vrt_cast_ray\* d_rays, int64_t n,\s+"
                     r"vrt_surface\* d_surfaces, uint64_t\* d_stats, void\* stream\);", text)
    words = (("EXAMINED", 8), ("RESOLVED", 4), ("ORPHANS", 9), ("AMBIGUOUS", 10), ("INVALID", 11), ("ENCLOSED", 12))
    for name, word in words:
        assert re.search(r"VRT_S_SURFACE_%s = %d\b" % (name, word), text), name
        assert getattr(nat, "S_SURFACE_" + name) == word
    assert "#define VRT_ABI_VERSION 9" in text and "unjittered" in text.lower() and "own definition" in text
    L = nat.lib()
    assert L.vrt_abi_version() == 9 and nat.ABI_VERSION == 9      # the change only adds a symbol
    assert L.vrt_hit_surfaces is not None and "vrt_hit_surfaces" in nat.EXPORTS
    assert C.sizeof(nat.VrtSurface) == 64 == nat.SURFACE_BYTES == sf.SURFACE_DTYPE.itemsize
    fields = ("vel", "next", "normal", "status", "neighbour", "resolution", "reflect", "side", "fetched", "open", "pad")
    offsets = [0, 24, 48, 51, 52, 55, 56, 57, 58, 59, 60]
    assert [getattr(nat.VrtSurface, f).offset for f in fields] == offsets
    assert [sf.SURFACE_DTYPE.fields[f][1] for f in fields] == offsets
    assert (nat.SURFACE_OK, nat.SURFACE_NONE, nat.SURFACE_ORPHAN, nat.SURFACE_INVALID) == (0, -1, -2, -3)
    # the build: both translation units, the same flags, both counted by needs_build()
    units = [os.path.basename(u) for u in nat.UNITS]
    assert units == ["vrt_kernels.hip", "vrt_surface.hip"] and set(nat.UNITS) <= set(nat.SOURCES)
    assert "-ffp-contract=off" in nat.HIPCC_FLAGS
    assert "csrc/vrt_surface.hip" in open(os.path.join(ROOT, "tools", "build_variant.sh")).read()
    import python_raytracer_amd
    assert python_raytracer_amd.SurfaceResult is not None and "SurfaceResult" in python_raytracer_amd.__all__


def test_hit_surfaces_rejects_bad_arguments_without_a_device():
    """Everything the entry point can refuse is refused before its first HIP call: these calls carry made-up device
    pointers, which nothing reads."""
    L = nat.lib()
    fake = 0x1000
    sc = nat.VrtScene()
    sc.origin[:] = [-32, -32, -32]
    sc.dims[:] = [4, 4, 4]
    sc.chunk_size, sc.n_slots, sc.n_materials, sc.max_resolution = 16, 64, 4, 3
    sc.d_chunk_table = sc.d_voxels = sc.d_materials = fake

    def call(scene=sc, hits=fake, rays=fake, n=100, surfaces=fake, stats=fake):
        return L.vrt_hit_surfaces(C.byref(scene) if scene is not None else None, hits, rays, n, surfaces, stats, None)

    assert call(scene=None) == -1 and call(hits=None) == -1 and call(rays=None) == -1 and call(surfaces=None) == -1
    assert call(stats=None) == -1 and call(stats=None, n=0) == -1
    assert call(n=-1) == -1 and call(n=1 << 32) == -1 and call(n=(1 << 32) + 5) == -1
    assert call(hits=fake + 4) == -1 and call(rays=fake + 32) == -1 and call(surfaces=fake + 32) == -1 and call(surfaces=fake + 8) == -1
    for field, value in (("chunk_size", 12), ("d_chunk_table", None), ("d_voxels", None), ("d_materials", None), ("n_materials", 256),
                         ("n_materials", -1), ("n_slots", -1)):
        bad = nat.VrtScene.from_buffer_copy(sc)
        setattr(bad, field, value)
        assert call(scene=bad) == -1, field
    bad = nat.VrtScene.from_buffer_copy(sc)
    bad.origin[0] = -30
    assert call(scene=bad) == -1                                            # the origin is a multiple of the chunk size
    bad = nat.VrtScene.from_buffer_copy(sc)
    bad.dims[1] = 0
    assert call(scene=bad) == -1


# ---- 2. the restatement is the renderer's ------------------------------------------------------------------------------------
_checked = {}


def checked(name, kind="case"):
    """The case's reference records, each held to shade_ref.trace: dict(recs, stats, compared, skipped).
    kind: "case" (sf.case), "edge" (sf.edge_case) or "lattice" (sf.lattice_case)."""
    key, name = (kind, name), (name if kind == "case" else "%s:%s" % (kind, name))
    if key in _checked:
        return _checked[key]
    c = {"case": sf.case, "edge": sf.edge_case, "lattice": sf.lattice_case}[kind](key[1])
    sc = c["scene"]
    exp, stats, recs = sf.expect(sc, c["hits"], c["vels"])
    compared, skipped = 0, []
    for k, s in enumerate(recs):
        if int(c["hits"]["material"][k]) <= 0:
            assert s["status"] == nat.SURFACE_NONE
            continue
        assert s["status"] == 0, (name, k, s)
        step, pos, mat, chunk, r, voxel = c["truth"][k]
        if s["chunk"] != chunk:
            # the record does not say which chunk the ray stood in and the rule took the other one of two that explain it: what
            # include/vrt.h documents for such records.  Only a record with more than one counting candidate may be one
            assert len(orf.counting(sc, pos, mat)) > 1, (name, k)
            skipped.append(k)
            continue
        assert s["resolution"] == r
        rec, _ = sr.trace(sc, c["settings"], c["origins"][k], c["vels"][k], c["end_lives"][k], (), has_background=False)
        cnt = rec["counters"]
        # the loop found this voxel, went on to the reflection, advanced once more and ended
        assert int(cnt[sr.C_HIT]) == 1 and int(cnt[sr.C_BROKE]) == 0 and float(rec["step"]) == step + r, (name, k, cnt)
        assert np.array_equal(np.array(rec["vel"]).view(np.uint64), np.array(s["vel"]).view(np.uint64)), (name, k, rec["vel"], s["vel"])
        assert np.array_equal(np.array(rec["pos"]).view(np.uint64), np.array(s["next"]).view(np.uint64)), (name, k, rec["pos"], s["next"])
        assert (int(cnt[sr.C_NBR]), int(cnt[sr.C_CGET])) == (s["lookups"], s["fetches"]), (name, k, cnt, s)
        compared += 1
    _checked[key] = dict(case=c, exp=exp, recs=recs, stats=stats, compared=compared, skipped=skipped)
    return _checked[key]


@pytest.mark.parametrize("name", sf.CASES)
def test_restatement_is_the_renderers(name):
    """Each ray's first hit (cast_ref.march), then shade_ref.trace with the life that ends it with the step after that hit: the
    end record's vel and pos are surface_ref's vel and next bit for bit, its neighbour and chunk_get counters the ref's counts."""
    got = checked(name)
    hits = int((got["case"]["hits"]["material"] > 0).sum())
    assert hits >= 100 and got["compared"] + len(got["skipped"]) == hits
    assert len(got["skipped"]) <= int(got["stats"][nat.S_SURFACE_AMBIGUOUS])
    assert int(got["stats"][nat.S_SURFACE_RESOLVED]) == hits == int(got["stats"][nat.S_SURFACE_EXAMINED])


def test_cases_are_not_vacuous():
    """What the comparisons above and on the GPU rest on, from the reference alone."""
    reflect, res = collections.Counter(), collections.Counter()
    fetches = ior0 = enclosed = ambiguous = 0
    for name in sf.CASES:
        got = checked(name)
        c = got["case"]
        ok = [(k, s) for k, s in enumerate(got["recs"]) if s["status"] == 0]
        assert len(ok) >= 100, (name, len(ok))
        reflect.update(s["reflect"] for k, s in ok)
        res.update(s["resolution"] for k, s in ok)
        fetches += sum(s["fetches"] for k, s in ok)
        ior0 += sum(float(c["scene"].materials[int(c["hits"]["material"][k]) - 1][5]) == 0.0 for k, s in ok)
        enclosed += int(got["stats"][nat.S_SURFACE_ENCLOSED])
        ambiguous += int(got["stats"][nat.S_SURFACE_AMBIGUOUS])
    assert set(reflect) == set(range(8)), reflect
    assert fetches >= 20 and res[2] >= 20 and res[3] >= 20 and ior0 >= 10 and enclosed >= 5, (fetches, res, ior0, enclosed)
    # the constructed record of owner_ref.lod_world: the chunk above (resolution 1) is taken and finds no y neighbour, the
    # chunk the ray stood in (resolution 3) snaps that neighbour back onto the hit voxel
    lod = checked("lod")
    assert ambiguous >= 1 and lod["recs"][-1]["ambiguous"] and lod["skipped"] == [len(lod["recs"]) - 1]
    assert lod["recs"][-1]["chunk"] == (2, 1, 0) and lod["case"]["truth"][-1][3] == (1, 1, 0)


EDGE_SETS = [("edge", n) for n in sf.edge_names()] + [("lattice", n) for n in sf.LATTICE_CASES]


@pytest.mark.parametrize("kind,name", EDGE_SETS, ids=["%s-%s" % k for k in EDGE_SETS])
def test_restatement_is_the_renderers_at_the_edges(kind, name):
    """The same comparison over the edge scenes -- chunk sizes 8, 32 and 64, worlds 2^26 to 2^27 cells out, beside +-2^28,
    resolutions up to 9, dense and 0.5 % grids -- with the rays of tests/edge_rays.py and with lattice rays that end on chunk
    faces.  The explicit-ray calls' range rule rejects none of the rays, so the GPU tests can cast them."""
    import edge_rays as er
    got = checked(name, kind)
    c = got["case"]
    assert not er.rejected(c["scene"], c["origins"], c["vels"], c["lives"]).any()
    hits = int((c["hits"]["material"] > 0).sum())
    assert hits >= (20 if name in er.SMALL else 150) and got["compared"] + len(got["skipped"]) == hits, (hits, got["compared"])
    assert len(got["skipped"]) <= int(got["stats"][nat.S_SURFACE_AMBIGUOUS])
    assert int(got["stats"][nat.S_SURFACE_RESOLVED]) == hits == int(got["stats"][nat.S_SURFACE_EXAMINED])
    assert int(got["stats"][nat.S_SURFACE_ORPHANS]) == 0 == int(got["stats"][nat.S_SURFACE_INVALID])


def resolved(got):
    return [(k, s) for k, s in enumerate(got["recs"]) if s["status"] == 0]


def test_lattice_sets_reach_the_chunk_rules_low_candidates():
    """From the reference alone: what the lattice sets are for.  Measured: records with a non-zero `low` mask per scene 133, 117,
    143, 142, 143, 146, 124, 122, 177, 141 (in the order of sf.LATTICE_CASES); all three bits set 15; a candidate chunk at index
    -1 759; the containing chunk at index = dims 38 (res9: hits read from the upper face of the box's last chunks, whose
    resolution does not divide the face's coordinate); a neighbour probe at index = dims 9; records that a candidate m > 0
    decides -- the containing chunk does not count, the chunk below does -- 73 (res9's upper-face rays: with resolutions 1 and 2
    a chunk below can never count, its snapped voxel lies on the face itself)."""
    all_bits = below = base_at_dims = probe_at_dims = decided_below = 0
    for name in sf.LATTICE_CASES:
        got = checked(name, "lattice")
        c = got["case"]
        sc = c["scene"]
        cs, origin, dims = sc.chunk_size, [int(v) for v in sc.origin], [int(v) for v in sc.dims]
        low_records = 0
        for k, s in resolved(got):
            pos, cell = c["hits"]["pos"][k], c["hits"]["cell"][k]
            low = sf.low_mask(sc, pos, cell)
            base = [(int(cell[a]) - origin[a]) // cs for a in range(3)]
            low_records += low != 0
            all_bits += low == 7
            below += any((low >> a) & 1 and base[a] == 0 for a in range(3))            # the candidate one chunk below: index -1
            base_at_dims += any(base[a] == dims[a] for a in range(3))
            decided_below += tuple(s["chunk"]) != tuple(base)                           # a candidate m > 0 is the one that counts
            # a neighbour probe that left the current chunk (`fetched`) for the cell one past the box's last chunk
            probe = [np.floor(pos[a] + (1 if (s["side"] >> a) & 1 else -1)) for a in range(3)]
            probe_at_dims += any((s["fetched"] >> a) & 1 and (int(probe[a]) - origin[a]) // cs == dims[a] for a in range(3))
        print(name, "records with a low mask:", low_records)
        assert low_records >= 50, (name, low_records)
    print("all three bits", all_bits, "index -1", below, "containing chunk at dims", base_at_dims, "probe at dims", probe_at_dims,
          "decided by a candidate below", decided_below)
    assert decided_below >= 20
    assert all_bits >= 5 and below >= 5 and probe_at_dims >= 5 and base_at_dims >= 1, (all_bits, below, base_at_dims, probe_at_dims)


def test_edge_sets_reach_their_edges():
    """From the reference alone.  Measured over the 21 sets: every reflect value (193 records and more each); 727 fetched bits; 520 enclosed records (227
    of them fill_dense's); largest |pos| of a hit 67108991.9 (far_pos), 134217727.5 (far_neg), 268433372.5 and 268433371.2
    (limit_28_pos / _neg); resolutions 1, 3 and 5 to 9 in res9."""
    reflect = collections.Counter()
    fetched = enclosed = 0
    reach = {}
    for name in sf.edge_names():
        got = checked(name, "edge")
        ok = resolved(got)
        reflect.update(s["reflect"] for k, s in ok)
        fetched += sum(bin(s["fetched"]).count("1") for k, s in ok)
        enclosed += int(got["stats"][nat.S_SURFACE_ENCLOSED])
        pos = got["case"]["hits"]["pos"][[k for k, s in ok]]
        reach[name] = (float(pos.min()), float(pos.max()))
    print("reflect", sorted(reflect.items()), "fetched bits", fetched, "enclosed", enclosed, "reach", reach)
    assert set(reflect) == set(range(8)), reflect
    assert fetched >= 100 and enclosed >= 200, (fetched, enclosed)
    assert int(checked("fill_dense", "edge")["stats"][nat.S_SURFACE_ENCLOSED]) >= 200
    # far_neg's box is [-2^27, -2^27 + 128) on x and y: its hits lie within a chunk or two of -2^27, beyond -2^27 + 192
    assert reach["far_pos"][1] > 2.0 ** 26 and reach["far_neg"][0] < -(2.0 ** 27) + 192 and reach["far_neg"][0] < -(2.0 ** 26)
    assert reach["limit_28_pos"][1] > 2.0 ** 28 - 4096 > 2.0 ** 27 and reach["limit_28_neg"][0] < -(2.0 ** 28) + 4096
    assert {s["resolution"] for k, s in resolved(checked("res9", "edge"))} >= {1, 3, 5, 6, 7, 8, 9}
    assert {checked(n, "edge")["case"]["scene"].chunk_size for n in ("far_mixed", "res9", "cs64")} == {8, 32, 64}


# ---- 3. the normal -----------------------------------------------------------------------------------------------------------
def _hand_scene(filled):
    """2^3 chunks of 8 round the origin, all listed at resolution 1, one material (ior 0), the given cells filled."""
    dims = np.array([2, 2, 2])
    origin = np.array([-8, -8, -8], np.int64)
    grid = np.zeros((16, 16, 16), np.uint8)
    for c in filled:
        grid[c[0] + 8, c[1] + 8, c[2] + 8] = 1
    return ol.Scene(origin, dims, 8, np.ones((2, 2, 2), np.uint8), np.ones((2, 2, 2), np.uint8), grid,
                    np.array([[100.0, 100.0, 100.0, 0.0, 1.0, 0.0, 0.0]]))


def test_normal_of_an_axis_aligned_ray_into_a_solid_is_minus_its_direction():
    sc = _hand_scene([(x, y, z) for x in range(-2, 2) for y in range(-2, 2) for z in range(-2, 2)])
    for a in range(3):
        for sign in (1, -1):
            cell = [0, 0, 0]
            cell[a] = -2 if sign > 0 else 1                  # the face the ray meets
            vel = [0.0, 0.0, 0.0]
            vel[a] = float(sign)
            s = sf.surface(sc, [c + 0.5 for c in cell], cell, 1, vel)
            assert s["status"] == 0 and s["normal"] == [-int(v) for v in vel] and s["open"] == 1 << a, (a, sign, s)
    # from inside the solid nothing is open: enclosed
    s = sf.surface(sc, [0.5, 0.5, 0.5], [0, 0, 0], 1, [1.0, 0.0, 0.0])
    assert s["status"] == 0 and s["normal"] == [0, 0, 0] and s["open"] == 0


def test_normal_takes_the_open_side_not_the_fastest_axis():
    """v = (1, 0.5, 0) into a voxel whose x-side incoming neighbour is filled and whose y-side one is open: (0, -1, 0)."""
    sc = _hand_scene([(0, 0, 0), (-1, 0, 0)])
    s = sf.surface(sc, [0.25, 0.5, 0.5], [0, 0, 0], 1, [1.0, 0.5, 0.0])
    assert s["status"] == 0 and s["normal"] == [0, -1, 0] and s["open"] == 0b010
    # with both open the faster axis wins, and a tie goes to the lower axis
    sc = _hand_scene([(0, 0, 0)])
    assert sf.surface(sc, [0.25, 0.5, 0.5], [0, 0, 0], 1, [1.0, 0.5, 0.0])["normal"] == [-1, 0, 0]
    assert sf.surface(sc, [0.25, 0.5, 0.5], [0, 0, 0], 1, [-3.0, 0.5, 3.0])["normal"] == [1, 0, 0]


# ---- 4. the compiler's report of the new translation unit --------------------------------------------------------------------
def test_surface_report_is_the_saved_one():
    if not os.path.exists(kernel_report.HIPCC):
        pytest.skip("no hipcc")
    fresh = kernel_report.parse(surface_report.compile_report())
    saved = surface_report.saved()
    assert list(fresh) == list(saved) and fresh == saved
    names = [n for n in fresh if "surface_kernel" in n]
    assert len(names) == 1 and len(fresh) == 2
    for name, fig in fresh.items():
        assert fig["VGPRs Spill"] == 0 and fig["ScratchSize [bytes/lane]"] == 0 and fig["SGPRs Spill"] == 0, (name, fig)
    assert fresh[names[0]]["LDS Size [bytes/block]"] == 256 * 8 + 6 * 4       # the ior column and the workgroup's six counts
