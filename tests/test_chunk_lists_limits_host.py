"""The inputs and references of tests/chunk_lists_limits.py, held to brute force on the CPU: world.chunk_object_lists against the
triple loop on the 4097-chunk case and at the coordinate limits, the host-made hit records against owner_ref.record_voxel, and
every reach condition of the GPU tests (tests/test_gpu_chunk_lists_limits.py) for the chosen seeds."""
import numpy as np
import pytest

import chunk_lists_limits as cl
import oracle_lib as ol
import owner_ref as orf
from cast_ref import id_materials
from python_raytracer_amd.world import chunk_object_total
from test_chunk_lists_host import brute_lists


# ---- A. the boxes of the build -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["c4097", "lo30", "hi30", "n64", "c5"])
def test_host_lists_equal_the_triple_loop(name):
    """chunk_object_lists is the reference of every build case: here against the rule chunk by chunk and object by object, with
    the empty, the inverted and the int32-extreme boxes among the objects and the chunk box at +-2^30."""
    c = cl.build_case(name)
    exp_off, exp_items = brute_lists(c["boxes"].tolist(), list(c["origin"]), list(c["dims"]), c["cs"])
    assert np.array_equal(c["offsets"], exp_off) and np.array_equal(c["items"], exp_items)
    assert chunk_object_total(c["boxes"], c["origin"], c["dims"], c["cs"]) == len(exp_items)
    b = c["boxes"]
    dead = np.flatnonzero((b[:, 1] <= b[:, 0]).any(1))
    assert len(dead) > 0 and not np.isin(c["items"], dead).any()           # empty and inverted boxes are in no list
    if name in ("lo30", "hi30"):
        lo = np.asarray(c["origin"], np.int64)
        hi = lo + np.asarray(c["dims"], np.int64) * c["cs"]
        assert (lo == -(1 << 30)).any() or (hi == 1 << 30).any()
        # boxes that touch the outermost faces: one voxel thick from inside (listed), from outside (in no list)
        live = (b[:, 1] > b[:, 0]).all(1)
        outside = live & ((b[:, 0] >= hi) | (b[:, 1] <= lo)).any(1)
        touching = ((b[:, 0] == hi) | (b[:, 1] == lo)).any(1)
        assert (outside & touching).sum() >= 4 and not np.isin(c["items"], np.flatnonzero(outside)).any()
        inside = live & ((b[:, 1] == hi) & (b[:, 0] == hi - 1) | (b[:, 0] == lo) & (b[:, 1] == lo + 1)).any(1) & ~outside
        assert inside.sum() >= 4 and np.isin(np.flatnonzero(inside), c["items"]).all()


@pytest.mark.parametrize("name", list(cl.BUILD_CASES))
def test_build_cases_reach_what_they_are_for(name):
    cl.build_reach(name)
    c = cl.build_case(name)
    assert cl.object_records(c["boxes"]).nbytes == 64 * len(c["boxes"])
    rec = cl.object_records(c["boxes"]).view(cl.OBJECT_DTYPE)
    assert np.array_equal(rec["mins"], c["boxes"][:, 0]) and np.array_equal(rec["maxs"], c["boxes"][:, 1])


def test_the_build_cases_cover_the_edges_of_the_scan():
    counts = sorted(c["n_chunks"] for c in map(cl.build_case, cl.BUILD_CASES) if c["cs"] == 8 and len(c["boxes"]) == 200)
    assert counts == [1, 4, 5, 255, 256, 257, 4095, 4096, 4097, 8191, 8192, 8193, 12293]
    assert sorted(len(cl.build_case(n)["boxes"]) for n in cl.BUILD_CASES if n[0] == "n") == [0, 1, 63, 64, 65, 127, 128, 192, 1000]
    assert any(min(c["origin"]) < 0 for c in map(cl.build_case, cl.BUILD_CASES)) and len({tuple(cl.build_case(n)["dims"]) for n in cl.BUILD_CASES}) > 10
    ov = cl.build_case(cl.OVERFLOW_CASE)
    assert ov["n_chunks"] > 2 * cl.SCAN_SPAN and len(ov["items"]) > ov["n_chunks"]
    for origin, dims, cs in cl.REFUSED_BOXES.values():
        lo = np.asarray(origin, np.int64)
        assert (lo % cs == 0).all() and ((lo < -(1 << 30)) | (lo + np.asarray(dims) * cs > 1 << 30)).sum() == 1


# ---- B. the worlds -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cs", cl.SMALL_CS + cl.BIG_CS)
def test_worlds_reach_what_they_are_for_and_owners_are_listed(cs):
    """The reach conditions, and build_world against the host lists: the object every filled voxel came from is in the list of
    the voxel's chunk."""
    c = cl.world_reach(cs)
    w = c["w"]
    at = np.argwhere(w.owner >= 0)
    assert np.array_equal(w.owner >= 0, w.grid != 0) and len(at) > 100
    dims = [int(d) for d in w.dims]
    chunk = ((at[:, 0] // cs) * dims[1] + at[:, 1] // cs) * dims[2] + at[:, 2] // cs
    pairs = np.unique(np.stack([chunk, w.owner[at[:, 0], at[:, 1], at[:, 2]]], 1), axis=0)
    off, items = c["offsets"], c["items"]
    for ch, k in pairs.tolist():
        assert k in items[off[ch]:off[ch + 1]].tolist(), (ch, k)
    assert len(pairs) >= (60 if cs in cl.SMALL_CS else 6)                # (many of the crowd are buried: they own nothing)


# ---- C. the records ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cs", cl.SMALL_CS)
def test_records_reach_what_they_are_for(cs):
    c, r = cl.records_reach(cs)
    # the half box of the owner tests: records on both sides, and an object across the cut that owns a voxel inside
    origin, dims = cl.half_box(cs)
    top = origin[0] + dims[0] * cs
    assert top == 0
    own = r["expect"]["object"] >= 0
    inside = cl.in_box(r["hits"]["cell"].astype(np.int64), origin, dims, cs)
    assert (own & inside).sum() > 500 and (own & ~inside).sum() > 100
    b = c["boxes"]
    across = np.flatnonzero((b[:, 0, 0] < top) & (b[:, 1, 0] > top) & (b[:, 1] > b[:, 0]).all(1))
    assert len(across) >= 1 and np.isin(r["expect"]["object"][own & inside], across).any()
    # the longest list lies inside the half box: the walk over two LDS tiles' worth of items is part of that test
    counts = np.diff(c["offsets"].astype(np.int64))
    assert np.unravel_index(int(np.argmax(counts)), tuple(int(d) for d in c["w"].dims))[0] < dims[0]
    if cs == 16:
        for to in (8, 32):
            lo, hi = cl.rounded_box(cs, 32)
            assert (lo % 32 == 0).all() and (hi % 32 == 0).all() and ((hi - lo) // to >= 1).all()
            assert (lo <= c["w"].origin).all() and (lo < c["w"].origin).any()   # (not the scene's box)


@pytest.mark.parametrize("cs", cl.SMALL_CS)
def test_records_agree_with_the_restated_candidate_rule(cs):
    """2000 of the host-made records, the face records among them, through owner_ref.record_voxel over the camera scene that
    lists every chunk at resolution 1: the same voxel, one candidate that counts, the same owner; the model voxel at `local`
    holds the record's material."""
    c, r = cl.world_case(cs), cl.owner_records(cs)
    w = c["w"]
    res = np.ones_like(w.present)
    sc = ol.Scene(w.origin, w.dims, cs, w.present, res, ol.Scene.camera_grid(w.grid, w.origin, w.dims, cs, w.present, res),
                  id_materials(len(w.materials)))
    rng = np.random.default_rng(cs)
    face = np.flatnonzero(r["kind"] == 1)
    sample = np.concatenate([rng.choice(face, min(600, len(face)), replace=False), rng.choice(len(r["kind"]), 1400, replace=False)])
    seen = set()
    for k in sample.tolist():
        h, e = r["hits"][k], r["expect"][k]
        if h["material"] <= 0:
            assert e["object"] == -1 and not e["voxel"].any() and not e["local"].any() and e["resolution"] == 0
            seen.add("none")
            continue
        got = orf.counting(sc, h["pos"].tolist(), int(h["material"]))
        if not got:
            assert e["object"] == -2 and not e["voxel"].any() and not e["local"].any() and e["resolution"] == 0
            seen.add("orphan")
            continue
        assert len(got) == 1                                               # never ambiguous
        cell, res_, vox = orf.record_voxel(sc, h["pos"].tolist(), int(h["material"]))
        assert res_ == 1 == e["resolution"] and list(vox) == e["voxel"].tolist() == h["cell"].tolist()
        assert orf.host_owner_at(w, vox) == e["object"]
        seen.add("face" if r["face"][k] else "voxel")
    assert seen == {"none", "orphan", "face", "voxel"}
    own = r["expect"]["object"] >= 0
    got = cl.model_materials(c["objs"], w.materials, r["expect"]["object"][own], r["expect"]["local"][own].astype(np.int64))
    assert np.array_equal(got, r["hits"]["material"][own])
