"""The oracle's chunk selection (orc_select_chunks) against the real reference where one ulp of the distance is a whole LOD:
tests/golden/select_edges.npz (tests/golden/make_select_edges.py -- the reference's own Window.chunk_update on small worlds).

The reference's distance is math.dist (lib.py:297-298), which is not sqrt(dx*dx + dy*dy + dz*dz): the two differ by an ulp on
about one input in six, and min(trunc(dist / step), chunk_lod) (init.py:448-449) turns that ulp into a LOD where dist / step
lands on an integer.  The fixture holds exact ties (camera on the tie, one ulp nearer, one ulp farther), 32 constructed pairs
on which the naive formula picks another LOD than the reference did (19 of them a lower one, 13 a higher one), chunk_lod 0,
chunk sizes 8..64, worlds 2^24 cells out and culling with traversed lists that cover some boundary chunks and not others.

With the naive formula in orc_select_chunks (as it was) test_oracle_selects_what_the_reference_selected fails on 38 of the 87
cases -- the 32 flip cases and their 6 repeats under culling that keep the flip chunk -- and on no tie, quad or lod0 case."""
import numpy as np
import pytest

import oracle_lib as ol
from select_edges import bracket_by, edge_cases, kat_dist, on_chunk_grid, oracle_select_one

CASES, FLIPS = edge_cases()


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_oracle_selects_what_the_reference_selected(case):
    pres, res = case.oracle()
    assert np.array_equal(pres, case.want_present), case.name
    assert np.array_equal(res, case.want_res), (case.name, res[case.present > 0], case.want_res[case.present > 0])


def test_fixture_still_discriminates():
    """The fixture must not go blunt unnoticed: the naive formula, recomputed here in numpy, picks another LOD than the
    fixture on at least the recorded number of chunk / camera pairs, on every recorded flip case, in the recorded direction,
    and nowhere on the exact ties; and the fixture covers what its generator asserted."""
    flip_case, flip_dir, up, down = FLIPS
    assert len(flip_case) >= 24 + 6 and up + down >= 24 and up > 0 and down > 0
    differing = 0
    for case in CASES:
        diff = case.naive_res() != case.want_res
        differing += int(diff.sum())
        if case.name.startswith(("tie_", "quad_", "lod0_", "cull_tie_")):
            assert not diff.any(), case.name
    assert differing >= len(flip_case), (differing, len(flip_case))
    for i, d in zip(flip_case, flip_dir):
        case = CASES[i]
        c = tuple(case.cells[0])
        assert case.want_present[c] and int(case.want_res[c]) - int(case.naive_res()[c]) == d, case.name
    assert len({(CASES[i].dist_max, CASES[i].chunk_lod) for i in flip_case}) >= 3 and any(
        (CASES[i].dist_max, CASES[i].chunk_lod) == (1000, 5) for i in flip_case)
    culled = [c for c in CASES if c.culling]
    assert sum(int(c.want_present.sum()) for c in culled) > 0 and sum(int((c.present > c.want_present).sum()) for c in culled) > 0
    assert any(len(c.trav) and (((c.trav - c.origin) // c.cs < 0) | ((c.trav - c.origin) // c.cs >= c.dims)).any() for c in culled)
    assert {c.cs for c in CASES} == {8, 16, 32, 64} and any(c.chunk_lod == 0 for c in CASES)
    assert any(np.abs(c.origin).max() >= 1 << 24 for c in CASES)
    for lod in sorted({c.chunk_lod for c in CASES}):
        seen = {int(r) - 1 for c in CASES if c.chunk_lod == lod for r in c.want_res[c.want_present > 0]}
        assert seen == set(range(lod + 1)), (lod, seen)


def test_bracket_recovers_the_known_distance_through_the_oracle():
    """The two-threshold bracket of tests/select_edges.py (what tests/test_gpu_select_edges.py asks the kernel) reads every
    kat_dist.json.gz value that lies on a chunk grid out of orc_select_chunks bit for bit; and it is sharp: it refuses the
    value one ulp below and one ulp above."""
    import math
    n = 0
    for family, vecs in kat_dist().items():
        usable = [v for v in vecs if on_chunk_grid(v)]
        assert len(usable) >= 100, (family, len(usable))
        for v in usable:
            assert bracket_by(oracle_select_one, v), (family, v.tolist())
            n += 1
        for v in usable[:20]:
            for off in (-math.inf, math.inf):
                w = v.copy()
                w[6] = math.nextafter(v[6], off)
                if w[6] >= 0:
                    assert not bracket_by(oracle_select_one, w), (family, v.tolist())
    assert n >= 1900
