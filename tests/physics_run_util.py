"""What the tests of the multi-tick physics share (tests/test_physics_run_host.py, tests/test_gpu_physics_run.py): how a recorded
run is cut into segments, and the comparison of a run's per-tick records with a fixture.  Nothing of the GPU is imported.

The fixtures (tests/golden/physics_*.npz) were recorded one tick at a time: before tick k the scene's script runs and `redraw` is
cleared on every object that has a sprite.  A run of many ticks cannot be interrupted, so a scene is run in SEGMENTS that start
at the script's ticks, and a tick's recorded `redraw` is derived from the run's records as a tick derives it: the object moved,
or its visibility changed -- or-ed, at a segment's first tick, with the flag the object had on entry, and at every tick for an
object without a sprite, whose flag nothing ever clears."""
import numpy as np


def segments(spec):
    """[(first tick, one past the last)] of the runs between the script's ticks."""
    cuts = sorted({0, spec["ticks"]} | {int(k) for k in spec["script"]})
    return list(zip(cuts[:-1], cuts[1:]))


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def assert_segment(z, first, trace, entry, has_sprite, what):
    """trace: [ticks][n] records of _native.BODY_SAMPLE_FIELDS for the fixture's ticks first, first + 1, ...; entry:
    physics_scenes.state() of the objects as the run found them (script applied, redraw cleared)."""
    seen = entry["visible"]
    for i, row in enumerate(trace):
        k = first + i
        for f in ("pos", "vel"):
            assert np.array_equal(bits(row[f]), bits(z[f][k])), "%s, tick %d: %s\n%r\n%r" % (what, k, f, row[f], z[f][k])
        for f in ("mins", "maxs"):
            assert np.array_equal(row[f], z[f][k]), "%s, tick %d: %s" % (what, k, f)
        visible = row["visible"] != 0
        assert np.array_equal(visible, z["visible"][k]), "%s, tick %d: visible" % (what, k)
        redraw = (row["moved"] != 0) | (visible != seen) | (entry["redraw"] if i == 0 else entry["redraw"] & ~has_sprite)
        assert np.array_equal(redraw, z["redraw"][k]), "%s, tick %d: redraw\n%r\n%r" % (what, k, redraw, z["redraw"][k])
        if "awake" in getattr(z, "files", z):
            assert np.array_equal(row["awake"] != 0, z["awake"][k]), "%s, tick %d: awake" % (what, k)
        seen = visible


def same_records(a, b):
    """Two structured arrays hold the same bytes."""
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
