#!/usr/bin/env python3
"""Generate tests/golden/physics_follow.npz: the reference's own physics under a camera attached to a body, observed tick by
tick on the scene of tests/physics_follow_scenes.py.

Needs the reference checkout make_golden.py needs; the test-suite only reads the committed output.  Nothing of the reference is
copied: its modules are imported in place (make_golden.load_reference), the scene is built from ITS Material, Sprite and Object,
the camera is attached with ITS Object.set_camera, and every tick is `for obj in objects: obj.update(data.player.cam_pos)` --
what Window.update does (init.py:464, 469-470).

    pos, vel           float64 [ticks, objects, 3]   after every tick
    mins, maxs         int64   [ticks, objects, 3]
    visible, redraw    bool    [ticks, objects]
    awake              bool    [ticks, objects]      math.dist(pos, camera) <= dist_move at the start of the tick (worked out here)
    cam_pos            float64 [ticks, 3]            data.player.cam_pos after every tick
    cam_start          float64 [3]                   ... and before the first
    weight             float64 [objects]
    spec               the scene (JSON)
    fixed_final_pos    float64 [objects, 3]          where the same scene ends under a camera held at cam_start

Between ticks `redraw` is cleared on every object that has a sprite, as the renderer would.
The file is written only if the attachment matters: compared with the same scene under the camera held at its first position,
some body's `awake` and some body's `visible` differ at some tick, and the final positions differ.

Usage:  python tests/golden/make_physics_follow.py
"""
import json
import os
import sys

import numpy as np

from make_golden import load_reference

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(OUT))
sys.path.insert(0, os.path.dirname(os.path.dirname(OUT)))

from make_physics import arrays, observe, unchanged  # noqa: E402


def run_reference(data, lib, spec, follow):
    """follow: the camera is data.player.cam_pos before every tick; else it is held where set_camera first put it."""
    import physics_follow_scenes as fs
    import physics_scenes as ps
    data.objects.clear()
    for k, v in spec["settings"].items():
        setattr(data.settings, k, v)
    objects, _, _ = ps.build(spec, data.Material, data.Sprite, data.Object, lib.vec3)
    data.player = fs.attach(objects, lib.vec2)
    start = [float(c) for c in data.player.cam_pos.tuple()]
    assert max(abs(a - b) for a, b in zip(start, spec["cam"])) < 1e-9, start      # (the scene names it to the nearest unit)
    rec = {k: [] for k in ("pos", "vel", "mins", "maxs", "visible", "redraw")}
    awake, cams = [], []
    for k in range(spec["ticks"]):
        ps.clear_redraw(objects)
        cam = data.player.cam_pos if follow else lib.vec3(*start)
        awake.append([bool(o.pos.distance(cam) <= data.settings.dist_move) for o in objects])
        for o in objects:
            o.update(cam)
        observe(objects, rec)
        cams.append([float(c) for c in data.player.cam_pos.tuple()])
    out = arrays(rec, objects)
    out.update(awake=np.array(awake, bool), cam_pos=np.array(cams, np.float64), cam_start=np.array(start, np.float64))
    return out


def main():
    import physics_follow_scenes as fs
    data, lib, mod = load_reference()
    spec = json.loads(json.dumps(fs.SCENE))
    ref = run_reference(data, lib, spec, True)
    held = run_reference(data, lib, spec, False)
    differ = dict(awake=int((ref["awake"] != held["awake"]).any(axis=0).sum()), visible=int((ref["visible"] != held["visible"]).any(axis=0).sum()),
                  final_pos=int((ref["pos"][-1] != held["pos"][-1]).any(axis=1).sum()))
    print("bodies that differ from the run under a held camera:", differ)
    assert all(v >= 1 for v in differ.values()), "the attachment does not matter in this scene: %r" % (differ,)
    assert (ref["cam_pos"][-1] != ref["cam_start"]).any()
    print("followed body: y %s -> %s (held camera: %s)" % (spec["objects"][spec["follow"]]["pos"][1], ref["pos"][-1][spec["follow"]][1],
                                                          held["pos"][-1][spec["follow"]][1]))
    out = dict(ref, fixed_final_pos=held["pos"][-1], spec=np.frombuffer(json.dumps(spec).encode(), np.uint8))
    if unchanged(fs.PATH, out):
        print(os.path.relpath(fs.PATH, OUT), "unchanged")
        return
    np.savez_compressed(fs.PATH, **out)
    print(os.path.relpath(fs.PATH, OUT), os.path.getsize(fs.PATH), "bytes")


if __name__ == "__main__":
    main()
