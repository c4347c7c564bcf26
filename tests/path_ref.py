"""Reference for the hit paths of explicit rays (Camera.path_rays -> vrt_path_rays, path_kernel).

`trace_path` restates shade_ref.trace -- init.py:66-120 and tile()'s alpha in Python floats over an oracle_lib.Scene -- and
records the ray's state in front of every lib.material: (step, pos, floor(pos), material), which is what vrt_cast_rays
stores for the first of them.  tests/test_path_host.py pins its end record to the oracle-derived records of shade_ref's six
ray sets, bit for bit, and the length of every path to the oracle's hit counter; the GPU tests compare with `path_set`."""
import math

import numpy as np

import shade_ref as sr

HIT_DTYPE = np.dtype([("step", "<f8"), ("pos", "<f8", 3), ("cell", "<i4", 3), ("material", "<i4")])
C_LOOKUP, C_NBR, C_RESNAP, C_CGET, C_HIT, C_DRAW, C_ADV, C_BROKE = range(8)


def unused():
    """The record of a slot that holds no hit: material -1, every other field 0."""
    rec = np.zeros(1, HIT_DTYPE)
    rec["material"] = -1
    return rec[0]


def trace_path(sc, settings, origin, vel, life, draws, has_background=True):
    """shade_ref.trace with the path: returns (vrt_ray record, [(step, pos, cell, material), ...]).  A ray that needs more
    draws than it was given reports nothing: the marker record (s = -3) and an empty path."""
    cs = sc.chunk_size
    radius = settings["chunk_radius"]
    pos = [float(v) for v in origin]
    vel = [float(v) for v in vel]
    life = float(life)
    step = bounces = energy = 0.0
    color = [0, 0, 0]
    cnt = [0] * 8
    trav = []
    path = []
    cmin = cmax = (0.0, 0.0, 0.0)
    chunk = None
    broke = 0
    pow_y = 1 + settings["falloff"]
    while step < life:
        if not all(p >= c for p, c in zip(pos, cmin)) or not all(p <= c for p, c in zip(pos, cmax)):
            cmin = tuple((p // cs) * cs for p in pos)
            cmax = tuple(c + cs for c in cmin)
            chunk = sr._chunk(sc, cmin)
            key = tuple(int(c) for c in cmin)
            if key not in trav:
                trav.append(key)
            cnt[C_RESNAP] += 1
        broke = 0
        if chunk is not None:
            cell = [math.floor(p) for p in pos]
            mat_id = sr._lookup(sc, chunk, cmin, cell)
            cnt[C_LOOKUP] += 1
            if mat_id:
                path.append((step, tuple(pos), tuple(int(c) for c in cell), mat_id))
                m = sc.materials[mat_id - 1]
                rough, absorb, ior, emit = float(m[3]), float(m[4]), float(m[5]), float(m[6])
                # lib.material (lib.py:448-460)
                a = absorb / sr._pow(1 + bounces, pow_y)
                if not a < 1:
                    a = 1
                color = sr._mix_rgb(color, m[:3], a)
                energy = energy * (1 - a) + emit * a
                life *= 1 - (rough * a)
                if rough != 0.0:
                    if cnt[C_DRAW] + 3 > len(draws):
                        return sr.marker(-3), []
                    for ax in range(3):
                        vel[ax] += (-1 + float(draws[cnt[C_DRAW] + ax]) * 2) * rough
                    cnt[C_DRAW] += 3
                cnt[C_HIT] += 1
                broke = 1
                bounces += absorb
                life /= float(int(sc.res[chunk])) + absorb * settings["lod_bounces"]
                ref = max(abs(vel[0]), abs(vel[1]), abs(vel[2]))
                if ref != 0.0 and ref != 1.0:
                    vel = [v / ref for v in vel]
                if step >= life or energy >= settings["max_light"] or bounces >= settings["max_bounces"] + 1:
                    break
                if ior != 0.0:
                    direction = (ior - 0.5) * 2
                    solid = []
                    for ax in range(3):
                        npos = list(pos)
                        npos[ax] = pos[ax] + 1 if vel[ax] < direction else pos[ax] - 1
                        if all(p >= c for p, c in zip(npos, cmin)) and all(p <= c for p, c in zip(npos, cmax)):
                            nchunk, ncmin = chunk, cmin
                        else:
                            ncmin = tuple((p // cs) * cs for p in npos)
                            nchunk = sr._chunk(sc, ncmin)
                            cnt[C_CGET] += 1
                        nid = 0
                        if nchunk is not None:
                            nid = sr._lookup(sc, nchunk, ncmin, [math.floor(p) for p in npos])
                            cnt[C_NBR] += 1
                        solid.append(bool(nid) and float(sc.materials[nid - 1][5]) == ior)
                    for ax in range(3):
                        if not solid[ax]:
                            vel[ax] -= vel[ax] * ior * 2
        if chunk is not None:
            size = float(int(sc.res[chunk]) if int(sc.res[chunk]) else 1)
        else:
            size = 1 + abs(radius - (min(pos) + radius) % cs)
        step += size
        pos = [p + v * size for p, v in zip(pos, vel)]
        cnt[C_ADV] += 1
        broke = 0
    cnt[C_BROKE] = broke
    if has_background:      # lib.material_background (lib.py:463-476)
        a = 1 / sr._pow(1 + bounces, pow_y)
        if not a < 1:
            a = 1
        up = vel[1] if vel[1] > 0 else 0
        color = sr._mix_rgb(color, [127, 127 + up * 64, 127 + up * 128], a)
        energy = energy * (1 - a) + (1 + up) * a
        color = [min(255, int(round(float(c) * energy))) for c in color]
    rec = np.zeros(1, sr.RAY_DTYPE)[0]
    rec["color"] = color
    rec["alpha"] = int(round(min(1, energy + settings["shutter"]) * 255))
    rec["ntrav"] = len(trav)
    rec["counters"] = cnt
    rec["detail"], rec["energy"], rec["step"], rec["life"], rec["bounces"] = 1.0, energy, step, life, bounces
    rec["pos"], rec["vel"] = pos, vel
    return rec, path


def trace_paths(sc, settings, origins, vels, lives, draws, has_background=True):
    """`trace_path` for a set of rays: (vrt_ray records [n], counts int32 [n] -- the hits of a completed ray, -3 for one whose
    draws ran out --, the rays' paths)."""
    n = len(origins)
    exp = np.zeros(n, sr.RAY_DTYPE)
    counts = np.zeros(n, np.int32)
    paths = []
    for k in range(n):
        exp[k], path = trace_path(sc, settings, origins[k], vels[k], lives[k], draws[k] if draws is not None else (), has_background)
        counts[k] = -3 if exp[k]["s"] == -3 else len(path)
        paths.append(path)
    return exp, counts, paths


def rows(paths, counts, max_hits):
    """The [n, max_hits] records vrt_path_rays must write for these paths: the first max_hits hits of every completed ray,
    every other slot unused."""
    out = np.zeros((len(paths), max_hits), HIT_DTYPE)
    out[:] = unused()
    for k, path in enumerate(paths):
        if counts[k] < 0:
            continue
        for j, (step, pos, cell, mat) in enumerate(path[:max_hits]):
            out[k, j] = (step, pos, cell, mat)
    return out


def assert_rows_equal(got, exp):
    """Bit for bit, field by field (the doubles as their 64-bit patterns)."""
    assert got.shape == exp.shape, (got.shape, exp.shape)
    for f in ("cell", "material"):
        assert np.array_equal(got[f], exp[f]), (f, np.argwhere((got[f] != exp[f]).reshape(got.shape + (-1,)).any(-1))[:8])
    for f in ("step", "pos"):
        a, b = np.ascontiguousarray(got[f]).view(np.uint64), np.ascontiguousarray(exp[f]).view(np.uint64)
        assert np.array_equal(a, b), (f, np.argwhere((a != b).reshape(got.shape + (-1,)).any(-1))[:8])


# ---- the six sets of shade_ref with their paths: computed once, shared by the CPU and the GPU tests, never changed ----------
_paths = {}


def path_set(name):
    """(records, counts, paths) of trace_paths over shade_ref.ray_set(name), with the set's full draw rows."""
    if name not in _paths:
        sc, st, has_bg, origins, vels, lives, draws, exp, trav = sr.ray_set(name)
        rec, counts, paths = trace_paths(sc, st, origins, vels, lives, draws, has_bg)
        rec.setflags(write=False)
        counts.setflags(write=False)
        _paths[name] = (rec, counts, paths)
    return _paths[name]
