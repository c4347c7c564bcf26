"""Pin the CPU oracle to the real reference OUTSIDE the reference's own operating envelope: the edge scenes and the
boundary-camera scene of tests/edge_scenes.py -- chunk sizes 8, 32 and 64, Frame resolutions up to 9, 20 and 179 degree lenses,
the extreme settings, worlds 2^26 to 2^28 cells from the origin, one-pixel-wide images, cameras exactly on chunk corners and
faces, no background -- as the reference itself rendered them (tests/golden/edges/, tests/golden/make_golden_edges.py).
tests/test_oracle_golden.py does the same on the default scene at moderate settings; the GPU tests over these scenes
(tests/test_gpu_edges.py, tests/test_gpu_parity.py) compare with the oracle, so this module is what ties them to the
reference's own Python semantics: banker's rounding of the sample count, float // and % on negative coordinates, the box
test that is inclusive on both ends, pos // resolution for resolutions that are no powers of two."""
import numpy as np
import pytest

import edge_scenes as es
import oracle_lib as ol

RENDERS = [r[0] for r in es.reference_renders()]
DOUBLES = ("detail", "energy", "step", "life", "bounces", "pos", "vel")

_fixtures, _oracle = {}, {}


def fixture(name):
    if name not in _fixtures:
        _fixtures[name] = es.load_reference_render(name)
    return _fixtures[name]


def oracle(name, libm):
    """The oracle's frame of a fixture in the given libm mode, computed once and never modified."""
    if (name, libm) not in _oracle:
        g = fixture(name)
        st = g["st"]
        px = np.concatenate(ol.pixel_lists(st["width"], st["height"], 1))
        o = ol.render(g["scene"], st, g["cam_pos"], g["cam_rot"], g["cam_lens"][0], px, libm=libm,
                      has_background=g["has_background"])
        _oracle[(name, libm)] = (px, o)
    return _oracle[(name, libm)]


def check_frame(g, px, o):
    """pix_mean, the traversed list (in order) and the counter totals of an oracle frame are the fixture's."""
    img = np.zeros(g["pix_mean"].shape)
    img[px[:, 1], px[:, 0]] = o["pix_mean"]
    assert np.array_equal(img, g["pix_mean"])
    assert np.array_equal(o["traversed"], g["ref_traversed"])
    assert np.array_equal(o["counters"], g["counters_total"])


def test_the_fixtures_are_the_renders_of_edge_scenes():
    """One fixture per camera of every edge case, no_background and 7 boundary positions x 2 resolution caps; the full
    per-ray form for the cases whose edge lives in double fields."""
    assert len(RENDERS) == len(set(RENDERS)) == 23 + 1 + 14
    full = [n for n in RENDERS if "rays" in fixture(n)]
    assert full == [n for n in RENDERS if n in ("far_pos", "far_neg", "limit_28_pos", "limit_28_neg", "res9", "fov179",
                                                "bounces16", "dof10", "rough25_abs7", "cs64")]
    assert not fixture("no_background")["has_background"] and all(fixture(n)["has_background"] for n in RENDERS if n != "no_background")


@pytest.mark.parametrize("name", RENDERS)
def test_oracle_glibc_bit_exact(name):
    """tests/test_oracle_golden.py's comparison on the edge fixtures: every stored field of every ray, pix_mean, the traversed
    list and the counter totals, bit for bit."""
    g = fixture(name)
    px, o = oracle(name, ol.LIBM_GLIBC)
    got, exp = o["rays"], g["ref_rays"]
    assert len(got) == len(exp) == int(g["n_rays"][0]) == o["n_rays"]
    for f in exp.dtype.names:
        assert np.array_equal(got[f], exp[f]), (f, np.flatnonzero((got[f] != exp[f]).reshape(len(got), -1).any(1))[:5])
    check_frame(g, px, o)


@pytest.mark.parametrize("name", RENDERS)
def test_oracle_portable_libm_integers_identical(name):
    """The oracle with the product's correctly rounded sin / cos / pow -- what the GPU tests compare with: every stored integer,
    pix_mean, the traversed list and the counter totals are the reference's; a stored double differs in at most 2 % of
    the rays of a case (a condition, not a measurement; glibc against the correctly rounded functions measured 0.45 % at worst)."""
    g = fixture(name)
    px, o = oracle(name, ol.LIBM_PORTABLE)
    got, exp = o["rays"], g["ref_rays"]
    assert len(got) == len(exp)
    differs = np.zeros(len(exp), bool)
    for f in exp.dtype.names:
        if f in DOUBLES:
            differs |= (got[f] != exp[f]).reshape(len(exp), -1).any(1)
        else:
            assert np.array_equal(got[f], exp[f]), (f, np.flatnonzero((got[f] != exp[f]).reshape(len(got), -1).any(1))[:5])
    check_frame(g, px, o)
    print("%s: %d of %d rays with a differing double (%.3f %%)" % (name, differs.sum(), len(exp), 100 * differs.mean()))
    assert differs.mean() <= 0.02, (int(differs.sum()), len(exp))


@pytest.mark.parametrize("case", list(es.EDGE_CASES))
def test_the_reference_reaches_the_edge(case):
    """edge_proof on the REFERENCE's rays of the first camera: the scene reaches the edge it is named after in the reference
    itself, not only in the oracle.  (A compact fixture lacks the fields its proof does not read: reading one raises.)"""
    g = fixture(case)
    fig = es.edge_proof(case, dict(rays=g["ref_rays"], traversed=g["ref_traversed"], n_rays=int(g["n_rays"][0])))
    print(case, fig)


def test_no_background_rays_end_without_a_hit():
    """no_background from the fixture alone: rays end without a hit, and they keep the colour and energy they had -- no sky,
    so a ray that never hit anything stays black with energy 0."""
    rays = fixture("no_background")["ref_rays"]
    never = rays["counters"][:, es.CNT["hit"]] == 0
    assert never.sum() > 100 and (rays["counters"][:, es.CNT["broke"]] == 0).sum() >= never.sum()
    assert not rays["color"][never].any() and not rays["energy"][never].any()
