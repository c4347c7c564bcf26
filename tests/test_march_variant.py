"""CPU-only: which march instance a launch runs.  vrt_diag_march_variant asks the library's pure chooser (march_choose in
csrc/vrt_kernels.hip) -- the function launch_march calls -- so a wrong branch of the launch policy shows here, without a GPU.

ROWS was recorded from the launcher as it was before the chooser existed (every launch replaced by a recorder, swept
over all inputs): label, the inputs that differ from _native.VARIANT_DEFAULTS, the instance with every template argument
(None: VRT_ERR_ARG), and the launch's (wt_on, trav_words, tile heads still set) afterwards.  The last rows are combinations
no kernel exists for, which the old launcher ran through another kernel's branch because no caller produces them."""
import ctypes as C
import re

import kernel_report
import test_kernel_resources as kr
from python_raytracer_amd import _native as nat

ERR_ARG = -1
ROWS = [
    ('config 2', dict(resmode=1, deep=1, keys=1, trav_words=256, occ=1), 'march_kernel<8,1,false,false,0,0,false,false,0>', (0, 256, 0)),
    ('config 2 --reseed', dict(resmode=1, deep=1, per_pixel=2, keys=1, trav_words=256, occ=1), 'march_kernel<8,1,false,false,0,3,false,false,0>', (0, 256, 0)),
    ('config 3', dict(pool=1, resmode=1, deep=1, keys=1, occ=1), 'march_pool_kernel<8,1,0,false,false,false>', (0, 0, 0)),
    ('config 3 --reseed', dict(pool=1, resmode=1, deep=1, per_pixel=2, keys=1, occ=1), 'march_pool_kernel<8,1,3,false,false,false>', (0, 0, 0)),
    ('config 5', dict(pool=1, deep=1, per_pixel=1, keys=1, big_scene=1, occ=1), 'march_pool_kernel<8,0,1,false,true,false>', (0, 0, 0)),
    ('config 5 without a ray table', dict(pool=1, deep=1, per_pixel=2, keys=1, big_scene=1, occ=1), 'march_pool_kernel<8,0,3,false,true,false>', (0, 0, 0)),
    ('config 5, one ray per lane: the window bitmap goes', dict(deep=1, per_pixel=1, keys=1, trav_words=256, bm_window=0, big_scene=1, occ=1), 'march_kernel<8,0,false,false,0,2,false,true,0>', (0, 0, 0)),
    ('config 5, VRT_DEFER_VISIT=0', dict(pool=1, deep=1, per_pixel=1, keys=1, big_scene=1, occ=1, defer_visit=0), 'march_pool_kernel<8,0,1,false,false,false>', (0, 0, 0)),
    ('config 3, VRT_DEFER_VISIT=2', dict(pool=1, resmode=1, deep=1, keys=1, occ=1, defer_visit=2), 'march_pool_kernel<8,1,0,false,true,false>', (0, 0, 0)),
    ('config 3 with its bitmap: no DEFER', dict(pool=1, resmode=1, deep=1, keys=1, trav_words=256, occ=1, defer_visit=2), 'march_pool_kernel<8,1,0,false,false,false>', (0, 256, 0)),
    ('config 5 without keys: no DEFER', dict(pool=1, deep=1, per_pixel=1, big_scene=1, occ=1), 'march_pool_kernel<8,0,1,false,false,false>', (0, 0, 0)),
    ('config 5 with a window bitmap: DEFER, the pool keeps it', dict(pool=1, deep=1, per_pixel=1, keys=1, trav_words=256, bm_window=0, big_scene=1, occ=1), 'march_pool_kernel<8,0,1,false,true,false>', (0, 256, 0)),
    ('config 5 with a whole bitmap: no DEFER', dict(pool=1, deep=1, per_pixel=1, keys=1, trav_words=256, big_scene=1, occ=1), 'march_pool_kernel<8,0,1,false,false,false>', (0, 256, 0)),
    ('config 5, one ray per lane, a whole bitmap: no DEFER', dict(deep=1, per_pixel=1, keys=1, trav_words=256, big_scene=1, occ=1), 'march_kernel<8,0,false,false,0,2,false,false,0>', (0, 256, 0)),
    ('config 5 with 4 positions: no DEFER', dict(pool=1, per_pixel=1, keys=1, big_scene=1, occ=1), 'march_pool_kernel<4,0,1,false,false,false>', (0, 0, 0)),
    ('config 5 at the generic resolution: no DEFER', dict(pool=1, resmode=2, deep=1, per_pixel=1, keys=1, big_scene=1, occ=1), 'march_pool_kernel<8,2,1,false,false,false>', (0, 0, 0)),
    ('look-ahead, config 3',dict(pool=1, resmode=1, deep=1, wt_on=1, keys=1, occ=1), 'march_pool_kernel<8,1,0,true,false,false>', (1, 0, 0)),
    ('look-ahead, config 5', dict(pool=1, deep=1, per_pixel=1, wt_on=1, keys=1, big_scene=1, occ=1), 'march_pool_kernel<8,0,1,true,false,false>', (1, 0, 0)),
    ('look-ahead, config 2', dict(resmode=1, deep=1, wt_on=1, keys=1, trav_words=256, occ=1), 'march_kernel<8,1,false,false,0,0,true,false,0>', (1, 256, 0)),
    ('tiled, config 5', dict(pool=1, deep=1, per_pixel=1, keys=1, big_scene=1, tile_heads=1, occ=1), 'march_pool_kernel<8,0,1,false,true,true>', (0, 0, 1)),
    ('tiled, config 3 with VRT_DEFER_VISIT=2', dict(pool=1, resmode=1, deep=1, keys=1, tile_heads=1, occ=1, defer_visit=2), 'march_pool_kernel<8,1,0,false,true,true>', (0, 0, 1)),
    ('tiled asked for, no DEFER: the heads go', dict(pool=1, resmode=1, deep=1, keys=1, tile_heads=1, occ=1), 'march_pool_kernel<8,1,0,false,false,false>', (0, 0, 0)),
    ('tiled asked for, no ray table: the heads go', dict(pool=1, deep=1, per_pixel=2, keys=1, big_scene=1, tile_heads=1, occ=1), 'march_pool_kernel<8,0,3,false,true,false>', (0, 0, 0)),
    ('record launch (vrt_trace_rays)', dict(record=1, resmode=2, keys=1, trav_words=256), 'march_kernel<4,2,true,false,0,4,false,false,0>', (0, 256, 0)),
    ('record launch of a frame: no look-ahead', dict(record=1, resmode=1, deep=1, wt_on=1, keys=1, trav_words=256, occ=1), 'march_kernel<4,2,true,false,0,4,false,false,0>', (0, 256, 0)),
    ('re-trace tier 1', dict(list=1, list_seed=1, resmode=1, deep=1, keys=1, trav_words=256, occ=1), 'march_kernel<4,2,false,true,0,4,false,false,1>', (0, 0, 0)),
    ('re-trace tier 2', dict(list=1, list_seed=2, resmode=1, deep=1, keys=1, trav_words=256, occ=1), 'march_kernel<4,2,false,true,0,4,false,false,2>', (0, 0, 0)),
    ('re-trace tier 1 with records', dict(record=1, list=1, list_seed=1, resmode=1, deep=1, keys=1, trav_words=256, occ=1), 'march_kernel<4,2,true,true,0,4,false,false,1>', (0, 0, 0)),
    ('re-trace tier 2 with records', dict(record=1, list=1, list_seed=2, deep=1, per_pixel=2, keys=1, big_scene=1, occ=1), 'march_kernel<4,2,true,true,0,4,false,false,2>', (0, 0, 0)),
    ('', dict(defer_visit=0), 'march_kernel<4,0,false,false,0,0,false,false,0>', (0, 0, 0)),
    ('', dict(per_pixel=1, defer_visit=0), 'march_kernel<4,0,false,false,0,2,false,false,0>', (0, 0, 0)),
    ('', dict(deep=1, defer_visit=0), 'march_kernel<8,0,false,false,0,0,false,false,0>', (0, 0, 0)),
    ('', dict(deep=1, wt_on=1, defer_visit=0), 'march_kernel<8,0,false,false,0,0,true,false,0>', (1, 0, 0)),
    ('', dict(deep=1, per_pixel=1, defer_visit=0), 'march_kernel<8,0,false,false,0,2,false,false,0>', (0, 0, 0)),
    ('', dict(deep=1, per_pixel=1, wt_on=1, defer_visit=0), 'march_kernel<8,0,false,false,0,2,true,false,0>', (1, 0, 0)),
    ('', dict(deep=1, per_pixel=2, defer_visit=0), 'march_kernel<8,0,false,false,0,3,false,false,0>', (0, 0, 0)),
    ('', dict(resmode=1, defer_visit=0), 'march_kernel<4,1,false,false,0,0,false,false,0>', (0, 0, 0)),
    ('', dict(resmode=1, per_pixel=1, defer_visit=0), 'march_kernel<4,1,false,false,0,2,false,false,0>', (0, 0, 0)),
    ('', dict(resmode=1, deep=1, per_pixel=1, defer_visit=0), 'march_kernel<8,1,false,false,0,2,false,false,0>', (0, 0, 0)),
    ('', dict(resmode=1, deep=1, per_pixel=1, wt_on=1, defer_visit=0), 'march_kernel<8,1,false,false,0,2,true,false,0>', (1, 0, 0)),
    ('', dict(resmode=2, defer_visit=0), 'march_kernel<4,2,false,false,0,0,false,false,0>', (0, 0, 0)),
    ('', dict(resmode=2, per_pixel=1, defer_visit=0), 'march_kernel<4,2,false,false,0,2,false,false,0>', (0, 0, 0)),
    ('', dict(resmode=2, deep=1, defer_visit=0), 'march_kernel<8,2,false,false,0,0,false,false,0>', (0, 0, 0)),
    ('', dict(resmode=2, deep=1, per_pixel=1, defer_visit=0), 'march_kernel<8,2,false,false,0,2,false,false,0>', (0, 0, 0)),
    ('', dict(pool=1, defer_visit=0), 'march_pool_kernel<4,0,0,false,false,false>', (0, 0, 0)),
    ('', dict(pool=1, per_pixel=1, defer_visit=0), 'march_pool_kernel<4,0,1,false,false,false>', (0, 0, 0)),
    ('', dict(pool=1, deep=1, defer_visit=0), 'march_pool_kernel<8,0,0,false,false,false>', (0, 0, 0)),
    ('', dict(pool=1, deep=1, wt_on=1, defer_visit=0), 'march_pool_kernel<8,0,0,true,false,false>', (1, 0, 0)),
    ('', dict(pool=1, deep=1, per_pixel=2, defer_visit=0), 'march_pool_kernel<8,0,3,false,false,false>', (0, 0, 0)),
    ('', dict(pool=1, resmode=1, defer_visit=0), 'march_pool_kernel<4,1,0,false,false,false>', (0, 0, 0)),
    ('', dict(pool=1, resmode=1, per_pixel=1, defer_visit=0), 'march_pool_kernel<4,1,1,false,false,false>', (0, 0, 0)),
    ('', dict(pool=1, resmode=1, deep=1, per_pixel=1, defer_visit=0), 'march_pool_kernel<8,1,1,false,false,false>', (0, 0, 0)),
    ('', dict(pool=1, resmode=1, deep=1, per_pixel=1, wt_on=1, defer_visit=0), 'march_pool_kernel<8,1,1,true,false,false>', (1, 0, 0)),
    ('', dict(pool=1, resmode=2, defer_visit=0), 'march_pool_kernel<4,2,0,false,false,false>', (0, 0, 0)),
    ('', dict(pool=1, resmode=2, per_pixel=1, defer_visit=0), 'march_pool_kernel<4,2,1,false,false,false>', (0, 0, 0)),
    ('', dict(pool=1, resmode=2, deep=1, defer_visit=0), 'march_pool_kernel<8,2,0,false,false,false>', (0, 0, 0)),
    ('', dict(pool=1, resmode=2, deep=1, per_pixel=1, defer_visit=0), 'march_pool_kernel<8,2,1,false,false,false>', (0, 0, 0)),
    ('', dict(deep=1, keys=1, big_scene=1), 'march_kernel<8,0,false,false,0,0,false,true,0>', (0, 0, 0)),
    ('', dict(deep=1, per_pixel=2, keys=1, big_scene=1), 'march_kernel<8,0,false,false,0,3,false,true,0>', (0, 0, 0)),
    ('', dict(resmode=1, deep=1, keys=1, big_scene=1), 'march_kernel<8,1,false,false,0,0,false,true,0>', (0, 0, 0)),
    ('', dict(resmode=1, deep=1, per_pixel=1, keys=1, big_scene=1), 'march_kernel<8,1,false,false,0,2,false,true,0>', (0, 0, 0)),
    ('', dict(resmode=1, deep=1, per_pixel=2, keys=1, big_scene=1), 'march_kernel<8,1,false,false,0,3,false,true,0>', (0, 0, 0)),
    ('', dict(pool=1, deep=1, keys=1, big_scene=1), 'march_pool_kernel<8,0,0,false,true,false>', (0, 0, 0)),
    ('', dict(pool=1, deep=1, keys=1, big_scene=1, tile_heads=1), 'march_pool_kernel<8,0,0,false,true,true>', (0, 0, 1)),
    ('', dict(pool=1, resmode=1, deep=1, per_pixel=1, keys=1, big_scene=1), 'march_pool_kernel<8,1,1,false,true,false>', (0, 0, 0)),
    ('', dict(pool=1, resmode=1, deep=1, per_pixel=1, keys=1, big_scene=1, tile_heads=1), 'march_pool_kernel<8,1,1,false,true,true>', (0, 0, 1)),
    ('', dict(pool=1, resmode=1, deep=1, per_pixel=2, keys=1, big_scene=1), 'march_pool_kernel<8,1,3,false,true,false>', (0, 0, 0)),
    ('', dict(occ=1, lookup=1, defer_visit=0), 'march_kernel<4,0,false,false,1,0,false,false,0>', (0, 0, 0)),
    ('', dict(per_pixel=1, occ=1, lookup=1, defer_visit=0), 'march_kernel<4,0,false,false,1,2,false,false,0>', (0, 0, 0)),
    ('', dict(deep=1, occ=1, lookup=1, defer_visit=0), 'march_kernel<8,0,false,false,1,0,false,false,0>', (0, 0, 0)),
    ('', dict(deep=1, per_pixel=1, occ=1, lookup=1, defer_visit=0), 'march_kernel<8,0,false,false,1,2,false,false,0>', (0, 0, 0)),
    ('', dict(resmode=1, occ=1, lookup=1, defer_visit=0), 'march_kernel<4,1,false,false,1,0,false,false,0>', (0, 0, 0)),
    ('', dict(resmode=1, per_pixel=1, occ=1, lookup=1, defer_visit=0), 'march_kernel<4,1,false,false,1,2,false,false,0>', (0, 0, 0)),
    ('', dict(resmode=1, deep=1, occ=1, lookup=1, defer_visit=0), 'march_kernel<8,1,false,false,1,0,false,false,0>', (0, 0, 0)),
    ('', dict(resmode=1, deep=1, per_pixel=1, occ=1, lookup=1, defer_visit=0), 'march_kernel<8,1,false,false,1,2,false,false,0>', (0, 0, 0)),
    ('', dict(occ=1, lookup=2, defer_visit=0), 'march_kernel<4,0,false,false,2,0,false,false,0>', (0, 0, 0)),
    ('', dict(per_pixel=1, occ=1, lookup=2, defer_visit=0), 'march_kernel<4,0,false,false,2,2,false,false,0>', (0, 0, 0)),
    ('', dict(deep=1, occ=1, lookup=2, defer_visit=0), 'march_kernel<8,0,false,false,2,0,false,false,0>', (0, 0, 0)),
    ('', dict(deep=1, per_pixel=1, occ=1, lookup=2, defer_visit=0), 'march_kernel<8,0,false,false,2,2,false,false,0>', (0, 0, 0)),
    ('', dict(resmode=1, occ=1, lookup=2, defer_visit=0), 'march_kernel<4,1,false,false,2,0,false,false,0>', (0, 0, 0)),
    ('', dict(resmode=1, per_pixel=1, occ=1, lookup=2, defer_visit=0), 'march_kernel<4,1,false,false,2,2,false,false,0>', (0, 0, 0)),
    ('', dict(resmode=1, deep=1, occ=1, lookup=2, defer_visit=0), 'march_kernel<8,1,false,false,2,0,false,false,0>', (0, 0, 0)),
    ('', dict(resmode=1, deep=1, per_pixel=1, occ=1, lookup=2, defer_visit=0), 'march_kernel<8,1,false,false,2,2,false,false,0>', (0, 0, 0)),
    ('lookup variant without an occupancy table', dict(deep=1, keys=1, lookup=1), None, None),
    ('lookup variant at the generic resolution', dict(resmode=2, deep=1, occ=1, lookup=2), None, None),
    ('no ray table, 4 positions', dict(resmode=1, per_pixel=2, occ=1), None, None),
    ('no ray table, generic resolution', dict(resmode=2, deep=1, per_pixel=2, occ=1), None, None),
    ('no ray table, lookup variant', dict(deep=1, per_pixel=2, occ=1, lookup=1), None, None),
    ('no ray table, 4 positions, pool', dict(pool=1, resmode=1, per_pixel=2, occ=1), None, None),
    ('no ray table with the look-ahead, pool', dict(pool=1, deep=1, per_pixel=2, wt_on=1, occ=1), None, None),
    ('look-ahead at the generic resolution, pool', dict(pool=1, resmode=2, deep=1, wt_on=1, occ=1), None, None),
    ('look-ahead at the generic resolution', dict(resmode=2, deep=1, wt_on=1, occ=1), None, None),
    ('look-ahead, 4 positions', dict(resmode=1, wt_on=1, occ=1), None, None),
    ('look-ahead, lookup variant', dict(deep=1, wt_on=1, occ=1, lookup=1), None, None),
    ('look-ahead without a ray table', dict(deep=1, per_pixel=2, wt_on=1, occ=1), None, None),
    ('pool with a lookup variant', dict(pool=1, deep=1, occ=1, lookup=1), None, None),
    ('pool with records', dict(record=1, pool=1), None, None),
    ('pool with a re-trace', dict(list=1, list_seed=1, pool=1), None, None),
    ('re-trace without a tier', dict(list=1), None, None),
]


def test_every_row_runs_the_recorded_instance():
    wrong = []
    for label, inputs, name, effects in ROWS:
        got = nat.march_variant(**inputs)
        if got != ((0, name, effects) if name else (ERR_ARG, None, None)):
            wrong.append((label, inputs, got, name, effects))
    assert not wrong, wrong


def test_rows_cover_every_instance_a_launch_can_select():
    """Every march_kernel / march_pool_kernel instance of the library's table but the one no launch selects, and the
    kernels tests/test_kernel_resources.py names for the shipped operating points."""
    src = open(kernel_report.SRC).read()
    table = re.findall(r"^    X\((\d), (\w+), (\d), (\w+), (\w+), (\d), (\d), (\w+), (\w+), (\w+), (\d)\)", src, re.M)
    spec = {"VRT_SPEC": "4", "VRT_SPEC_DEEP": "8", "8": "8"}
    shipped = set()
    for pool, s, res, rec, lst, lk, pp, w, d, t, seed in table:
        if (rec, lst, pp) == ("false", "false", "4"):
            continue   # the record / re-trace variant that neither records nor re-traces
        shipped.add("march_pool_kernel<%s>" % ",".join((spec[s], res, pp, w, d, t)) if pool == "1" else
                    "march_kernel<%s>" % ",".join((spec[s], res, rec, lst, lk, pp, w, d, seed)))
    assert len(table) == 74 and len(shipped) == 73
    assert {name for _, _, name, _ in ROWS if name} == shipped

    def mangled(name):
        fam, args = name[:-1].split("<")
        return "_Z%d%sI%sEv11MarchParams" % (len(fam), fam, "".join(
            "Lb%dE" % (a == "true") if a in ("true", "false") else "Li%sE" % a for a in args.split(",")))
    assert set(kr.FRAME_KERNELS) | set(kr.RAYGEN_KERNELS) <= {mangled(name) for _, _, name, _ in ROWS if name}


def test_every_error_return_is_in_the_rows():
    labels = {label for label, _, name, _ in ROWS if name is None}
    assert len(labels) == 16 and all(labels)


def test_march_variant_diagnostic_is_exported_and_checks_its_arguments():
    """Outside include/vrt.h and _native.EXPORTS (no ABI change), host memory only."""
    L = nat.lib()
    assert "vrt_diag_march_variant" not in nat.EXPORTS
    assert "vrt_diag_march_variant" not in open(kernel_report.SRC.replace("python_raytracer_amd/csrc/vrt_kernels.hip", "include/vrt.h")).read()
    n = len(nat.VARIANT_INPUTS)
    words = (C.c_int32 * n)(*[nat.VARIANT_DEFAULTS[k] for k in nat.VARIANT_INPUTS])
    name, eff = C.create_string_buffer(128), (C.c_int32 * 3)(-7, -7, -7)
    assert L.vrt_diag_march_variant(None, n, name, 128, eff) == ERR_ARG
    assert L.vrt_diag_march_variant(words, n - 1, name, 128, eff) == ERR_ARG
    assert L.vrt_diag_march_variant(words, n + 1, name, 128, eff) == ERR_ARG
    assert L.vrt_diag_march_variant(words, n, None, 128, eff) == ERR_ARG
    assert L.vrt_diag_march_variant(words, n, name, 128, None) == ERR_ARG
    assert L.vrt_diag_march_variant(words, n, name, 8, eff) == ERR_ARG        # no room for the name
    assert list(eff) == [-7, -7, -7]
    assert L.vrt_diag_march_variant(words, n, name, 128, eff) == 0
    assert name.value == b"march_kernel<4,0,false,false,0,0,false,false,0>" and list(eff) == [0, 0, 0]
    for key, bad in (("resmode", 3), ("resmode", -1), ("per_pixel", 3), ("lookup", 3), ("lookup", -1), ("trav_words", -1)):
        assert nat.march_variant(**{key: bad})[0] == ERR_ARG, (key, bad)


# ---- the launch census (vrt_diag_launch_census, _native.launch_census) ------------------------------------------------------
# The instances of the families a launch chooses by resolution mode alone (VRT_BY_RES in csrc/vrt_kernels.hip) and the two
# re-trace instances of the batched views, with every template argument: the census' rows behind the march table's.
BY_RES_NAMES = [
    'march_views_kernel<8,0,false,0>', 'march_views_kernel<8,1,false,0>', 'march_views_kernel<4,2,false,0>',
    'march_views_kernel<4,2,true,1>', 'march_views_kernel<4,2,true,2>',
    'first_hit_kernel<8,0,1,false>', 'first_hit_kernel<8,0,0,false>', 'first_hit_kernel<8,1,1,false>', 'first_hit_kernel<8,1,0,false>',
    'first_hit_kernel<4,2,1,false>', 'first_hit_kernel<4,2,0,false>',
    'first_hit_kernel<8,0,1,true>', 'first_hit_kernel<8,0,0,true>', 'first_hit_kernel<8,1,1,true>', 'first_hit_kernel<8,1,0,true>',
    'first_hit_kernel<4,2,1,true>', 'first_hit_kernel<4,2,0,true>',
    'cast_kernel<8,0>', 'cast_kernel<8,1>', 'cast_kernel<4,2>',
    'shade_kernel<8,0,true>', 'shade_kernel<8,1,true>', 'shade_kernel<4,2,true>',
    'shade_kernel<8,0,false>', 'shade_kernel<8,1,false>', 'shade_kernel<4,2,false>',
]
UNSELECTED = 'march_kernel<4,2,false,false,0,4,false,false,0>'   # the table's one row no launch selects


def census_row(L, row, cap=128):
    name, count = C.create_string_buffer(b"?" * (cap - 1), cap), C.c_int64(-7)
    return L.vrt_diag_launch_census(row, name, cap, C.byref(count)), name.value.decode(), count.value


def test_launch_census_is_exported_and_checks_its_arguments():
    """Outside include/vrt.h and _native.EXPORTS (no ABI change); callable without a GPU; a refusal writes nothing."""
    L = nat.lib()
    assert "vrt_diag_launch_census" not in nat.EXPORTS and L.vrt_abi_version() == 9
    assert "vrt_diag_launch_census" not in open(kernel_report.SRC.replace("python_raytracer_amd/csrc/vrt_kernels.hip", "include/vrt.h")).read()
    n, first, count = census_row(L, 0)
    assert n == 74 + len(BY_RES_NAMES) and first == 'march_kernel<4,2,true,false,0,4,false,false,0>' and count >= 0
    name, cnt = C.create_string_buffer(b"?" * 127, 128), C.c_int64(-7)
    for row, nm, cap, ct in ((-1, name, 128, cnt), (n, name, 128, cnt), (1 << 30, name, 128, cnt), (0, None, 128, cnt),
                             (0, name, 128, None), (0, name, 0, cnt), (0, name, -5, cnt), (0, name, len(first), cnt)):
        assert L.vrt_diag_launch_census(row, nm, cap, C.byref(ct) if ct is not None else None) == ERR_ARG, (row, cap)
        assert name.value == b"?" * 127 and cnt.value == -7, (row, cap)
    assert L.vrt_diag_launch_census(0, name, len(first) + 1, C.byref(cnt)) == n and name.value.decode() == first


def test_launch_census_rows_are_the_table_and_the_by_resolution_instances():
    """Row for row: the march table in its order -- its names are the ones vrt_diag_march_variant gives for ROWS, plus the one
    row no launch selects -- then the by-resolution families."""
    L = nat.lib()
    n = census_row(L, 0)[0]
    names = [census_row(L, row)[1] for row in range(n)]
    src = open(kernel_report.SRC).read()
    table = re.findall(r"^    X\((\d), (\w+), (\d), (\w+), (\w+), (\d), (\d), (\w+), (\w+), (\w+), (\d)\)", src, re.M)
    assert len(names) == len(set(names)) == len(table) + len(BY_RES_NAMES)
    march, by_res = names[:len(table)], names[len(table):]
    chosen = {nat.march_variant(**inputs)[1] for _, inputs, name, _ in ROWS if name}
    assert set(march) == chosen | {UNSELECTED} and UNSELECTED not in chosen
    assert by_res == BY_RES_NAMES
    assert list(nat.launch_census()) == names


def test_launch_census_counts_nothing_in_a_process_that_launched_nothing():
    """(in a child: this process may have rendered before)  Asking the chooser is no launch."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-c", "from python_raytracer_amd import _native as nat\nnat.march_variant(pool=1)\n"
                          "c = nat.launch_census()\nprint('CENSUS', len(c), sum(c.values()), min(c.values()))"],
                         cwd=root, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    assert [l for l in out.stdout.splitlines() if l.startswith("CENSUS")] == ["CENSUS %d 0 0" % (74 + len(BY_RES_NAMES))]
