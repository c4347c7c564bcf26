"""The explicit-ray sets over the edge scenes (tests/edge_rays.py) without a GPU: what tests/test_gpu_edge_rays.py relies
on, asserted on the reference side alone.  For every set: tests/path_ref.py's restatement gives the oracle-derived records
bit for bit, with path lengths equal to the oracle's hit counters (what tests/test_path_host.py asserts for the six ordinary
sets); the documented range rule of the explicit-ray calls rejects no ray; the shares of rays that miss, hit and hit twice
are large enough for a green GPU comparison to mean something; and the set reaches the edge its case is named after."""
import numpy as np
import pytest

import edge_rays as er
import shade_ref as sr

HALF = ("near4", "fill_sparse")       # dist 3 .. 4, or 0.5 % fill: second hits are not to be had


def figures(name):
    sc, st, has_bg, origins, vels, lives, draws, exp, trav = er.edge_ray_set(name)
    hits = exp["counters"][:, sr.C_HIT]
    return dict(rays=len(exp), miss=float((hits == 0).mean()), hit1=float((hits >= 1).mean()), hit2=float((hits >= 2).mean()),
                max_hits=int(hits.max()), max_draws=int(exp["counters"][:, sr.C_DRAW].max()), row=int(draws.shape[1]),
                has_bg=has_bg)


@pytest.mark.parametrize("name", er.ALL_CASES)
def test_trace_paths_equals_the_oracle(name):
    """trace_paths' end records are the oracle-derived records bit for bit, every path is as long as the oracle's hit
    counter, and no ray of the full-width set runs out of draws."""
    sc, st, has_bg, origins, vels, lives, draws, exp, trav = er.edge_ray_set(name)
    rec, counts, paths = er.edge_path_set(name)
    assert len(exp) == er.n_rays(name) and (exp["s"] == 0).all() and (rec["s"] == 0).all()
    sr.assert_records_equal(rec, exp)
    assert np.array_equal(counts, exp["counters"][:, sr.C_HIT])
    assert [len(p) for p in paths] == counts.tolist()
    assert int(exp["counters"][:, sr.C_DRAW].max()) <= draws.shape[1]
    assert has_bg == (name != "no_background")          # (the one set built and run without a background)
    for k in ("falloff", "shutter", "lod_bounces", "max_light", "max_bounces", "dist_min"):
        assert st[k] == er.edge_scene(name)[1][k]       # the case's own settings are the set's
    for path in paths:
        steps = [h[0] for h in path]
        assert steps == sorted(steps)
        for step, pos, cell, mat in path:
            assert cell == tuple(int(np.floor(p)) for p in pos) and 1 <= mat <= len(sc.materials)


@pytest.mark.parametrize("name", er.ALL_CASES)
def test_range_rule_rejects_no_ray(name):
    """|origin| + (max(life, 0) + 2 chunk_size + 2) max(1, |vel|_inf) < 2^28 on every axis, for every ray: a rejected ray
    would be hidden from the comparison.  The smallest margin of the set is printed."""
    sc, st, has_bg, origins, vels, lives, draws, exp, trav = er.edge_ray_set(name)
    assert not er.rejected(sc, origins, vels, lives).any()
    reach = (np.maximum(lives, 0) + 2.0 * sc.chunk_size + 2.0) * np.maximum(1.0, np.abs(vels).max(1))
    print(name, "smallest margin:", float((float(1 << 28) - np.abs(origins) - reach[:, None]).min()),
          "largest |vel|:", float(np.abs(vels).max()))
    assert (lives > 0).all() and (lives <= float(st["dist_max"]) - float(st["dist_min"])).all()
    # ... and the rule does reject: the same rays moved to the limit
    assert er.rejected(sc, np.where(origins >= 0, 1.0, -1.0) * float(1 << 28), vels, lives).all()


@pytest.mark.parametrize("name", er.ALL_CASES)
def test_sets_cover_the_cases(name):
    """Conditions on the oracle's records alone.  Share of the rays that miss / hit / hit twice and more, the largest hit
    count and the largest draw count of a ray (the width of the set's rows), as measured here:
        cs64            41.3 %  58.7 %  31.5 %    8   21
        far_pos         20.5 %  79.5 %  48.0 %    8   18
        far_neg         22.0 %  78.0 %  44.2 %    7   21
        far_mixed       70.2 %  29.8 %  10.3 %    5   15
        limit_28_pos    52.0 %  48.0 %  20.5 %    6   15
        limit_28_neg    60.7 %  39.3 %  13.5 %    6   15
        res9            59.8 %  40.2 %   6.5 %    6   15
        fov179          61.5 %  38.5 %  15.3 %    6   15
        fov20           54.2 %  45.8 %  19.5 %    6   18
        bounces_half    36.7 %  63.3 %  37.7 %   30   90
        bounces16       35.7 %  64.3 %  55.0 %  119  348
        lod_full        58.2 %  41.8 %  17.5 %    6   15
        dof10           49.3 %  50.7 %  24.8 %    6   15
        near4           48.3 %  51.7 %   0.0 %    1    3
        rough25_abs7    41.3 %  58.7 %  14.8 %   28   81
        fill_sparse     52.8 %  47.2 %   7.5 %    4   12
        fill_dense      36.0 %  64.0 %  43.5 %   11   27
        w1              48.4 %  51.6 %  29.7 %    5   12
        h1              64.1 %  35.9 %  14.1 %    6   15
        one_pixel       45.3 %  54.7 %  25.0 %    4   12
        no_background   58.7 %  41.3 %  12.5 %    6   15
    (the rays of res9 with a record in a chunk of resolution 5 / 7 / 9: 20 / 61 / 28; cs64: 203 rays visit 3 chunks and more;
    bounces16: 66 rays over 64 hits, 168 over 32; rough25_abs7: all 19 materials)"""
    f = figures(name)
    print(name, "miss %.1f %% hit %.1f %% twice %.1f %% largest count %d largest draw count %d"
          % (100 * f["miss"], 100 * f["hit1"], 100 * f["hit2"], f["max_hits"], f["max_draws"]))
    assert f["row"] == max(1, f["max_draws"])
    if name in HALF:
        assert f["hit1"] >= 0.1 and f["miss"] >= 0.1, f
    elif name == "fill_dense":
        assert f["hit2"] >= 0.1, f
    elif name in er.SMALL:
        assert f["rays"] == 64 and f["hit1"] > 0 and f["miss"] > 0, f
    else:
        assert f["rays"] == 600 and f["miss"] >= 0.1 and f["hit1"] >= 0.1 and f["hit2"] >= 0.05, f


# ---- the edge each set is there for ------------------------------------------------------------------------------------
def test_res9_records_lie_in_chunks_of_resolution_5_7_and_9():
    sc = er.edge_ray_set("res9")[0]
    seen = er.record_resolutions(sc, er.edge_path_set("res9")[2])
    n = {r: sum(1 for s in seen if r in s) for r in (5, 7, 9)}
    print("res9: rays with a record in a chunk of resolution 5 / 7 / 9:", n)
    assert all(v >= 20 for v in n.values()), n


def test_cs64_rays_hit_in_both_resolutions_and_cross_chunks():
    sc, st, has_bg, origins, vels, lives, draws, exp, trav = er.edge_ray_set("cs64")
    assert sc.chunk_size == 64
    seen = er.record_resolutions(sc, er.edge_path_set("cs64")[2])
    assert set().union(*seen) == {1, 2} == set(np.unique(sc.res[sc.present != 0]).tolist())
    many = int((exp["ntrav"] >= 3).sum())
    print("cs64: rays that visit 3 chunks and more:", many)
    assert many >= 100 and np.array_equal(exp["ntrav"], [len(t) for t in trav])


@pytest.mark.parametrize("name", ["far_pos", "far_neg", "far_mixed"])
def test_far_origins_are_far(name):
    sc, st, has_bg, origins = er.edge_ray_set(name)[:4]
    axes = er.far_axes(name)
    assert axes == ([2] if name == "far_mixed" else [0, 1, 2])
    assert (np.abs(origins[:, axes]) >= float((1 << 20) * sc.chunk_size)).all()
    print(name, "smallest |origin| on the displaced axes:", float(np.abs(origins[:, axes]).min()))


@pytest.mark.parametrize("name", er.LIMIT_CASES)
def test_limit_origins_are_beside_the_limit(name):
    sc, st, has_bg, origins = er.edge_ray_set(name)[:4]
    cam = np.asarray(er.edge_scene(name)[2][0][0], np.float64)
    gap = float(1 << 28) - np.abs(origins)
    print(name, "distance from the limit:", float(gap.min()), "..", float(gap.max()))
    assert (gap > 0).all() and (gap <= 2200).all() and (np.sign(origins) == (1 if name.endswith("pos") else -1)).all()
    assert (np.abs(origins - cam) <= 8).all() and (np.abs(origins) <= np.abs(cam)).all()


def test_bounces16_paths_outgrow_the_rows_of_path_rays():
    """More hits than vrt_path_rays keeps at its largest max_hits (64), and draw rows far wider than the 64 of the ordinary
    sets; the median draw count, to which the GPU test cuts the rows, exhausts some rays and not others."""
    sc, st, has_bg, origins, vels, lives, draws, exp, trav = er.edge_ray_set("bounces16")
    counts = er.edge_path_set("bounces16")[1]
    used = exp["counters"][:, sr.C_DRAW]
    print("bounces16: rays over 64 hits:", int((counts > 64).sum()), "over 32:", int((counts > 32).sum()), "most:", int(counts.max()),
          "median draw count:", int(np.median(used)))
    assert (counts > 64).sum() >= 1 and (counts > 32).sum() >= 10 and draws.shape[1] > sr.N_DRAWS
    assert st["max_bounces"] == 16.0 and st["falloff"] == 0.0 and st["lod_bounces"] == 0.0 and st["max_light"] == 100.0
    width = int(np.median(used))
    assert width >= 3 and 0 < (used > width).sum() < len(used)


def test_rough25_abs7_hits_most_materials():
    sc, st = er.edge_ray_set("rough25_abs7")[:2]
    mats = er.record_materials(er.edge_path_set("rough25_abs7")[2])
    print("rough25_abs7: materials hit:", len(mats))
    assert len(sc.materials) == 19 and len(mats) >= 12 and st["falloff"] == 3.0 and st["max_light"] == 0.1
