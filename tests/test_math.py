"""python_raytracer_amd/csrc/vrt_math.h (the sin / cos / pow the kernels and the oracle's portable mode share) against the
correctly rounded value computed with mpmath at 300 bits, in the argument ranges the trace path uses:
camera half-angles (|x| < 2 rad; lib.py:323-338 via init.py:41-43), (1 + bounces) ** (1 + falloff) (lib.py:450, 465).
The header claims the correctly rounded result; glibc's own functions are only "< 1 ulp" and are counted beside it.
vrt_dist3 (the chunk selection's distance, math.dist of lib.py:297-298) is held to CPython's known answers and to the
correctly rounded distance, with the naive sqrt(dx*dx + dy*dy + dz*dz) counted beside it."""
import ctypes as C

import mpmath
import numpy as np
import pytest

import oracle_lib as ol

mpmath.mp.prec = 300
N = 20000          # per function; tools/math_soak.py runs millions


def _lib():
    L = ol.lib()
    for f in (L.orc_sin, L.orc_cos):
        f.restype = C.c_double
        f.argtypes = [C.c_int, C.c_double]
    L.orc_pow.restype = C.c_double
    L.orc_pow.argtypes = [C.c_int, C.c_double, C.c_double]
    L.orc_dist3.restype = C.c_double
    L.orc_dist3.argtypes = [C.c_double, C.c_double, C.c_double]
    return L


def _correct(fn, *args):
    """Correctly rounded binary64 value of fn at exactly-representable arguments."""
    return float(fn(*[mpmath.mpf(a) for a in args]))     # mpf -> float rounds to nearest even from 300 bits


def test_sin_cos_are_correctly_rounded():
    L = _lib()
    rng = np.random.default_rng(11)
    xs = np.concatenate([rng.uniform(-2.0, 2.0, N), rng.uniform(-0.45, 0.45, N),      # half-angles of a 90-degree lens
                         rng.uniform(-1e-3, 1e-3, 500), [0.0, -0.0, 1e-300, np.pi / 4, np.pi / 2, -np.pi / 2, 2.0 ** -30]])
    bad = {"sin": 0, "cos": 0, "glibc_sin": 0, "glibc_cos": 0}
    for x in xs.tolist():
        s, c = _correct(mpmath.sin, x), _correct(mpmath.cos, x)
        bad["sin"] += L.orc_sin(ol.LIBM_PORTABLE, x) != s
        bad["cos"] += L.orc_cos(ol.LIBM_PORTABLE, x) != c
        bad["glibc_sin"] += L.orc_sin(ol.LIBM_GLIBC, x) != s
        bad["glibc_cos"] += L.orc_cos(ol.LIBM_GLIBC, x) != c
    assert bad["sin"] == 0 and bad["cos"] == 0, bad
    # the sign of a zero result follows the argument, like libm
    assert np.signbit(L.orc_sin(ol.LIBM_PORTABLE, -0.0)) and not np.signbit(L.orc_sin(ol.LIBM_PORTABLE, 0.0))


def test_joint_sin_cos_equals_the_single_functions():
    """vrt_sincos2 (the HIP ray generation's call: sin and cos of both lens half-angles in one straight-line block) returns
    bit for bit what vrt_sin / vrt_cos return -- inside its fast block's domain and outside it (zeros, |x| >= pi/4)."""
    L = _lib()
    L.orc_sincos2.restype = C.c_int
    L.orc_sincos2.argtypes = [C.c_double, C.c_double, C.POINTER(C.c_double)]
    rng = np.random.default_rng(13)
    a = np.concatenate([rng.uniform(-0.78, 0.78, N), rng.uniform(-2.0, 2.0, N // 4), rng.uniform(-1e-6, 1e-6, 200),
                        [0.0, -0.0, 0.3, np.pi / 4, -np.pi / 4, 0.7853981633974482, 1e-300]])
    b = rng.permutation(a)
    out = (C.c_double * 4)()
    fast = 0
    for x, y in zip(a.tolist(), b.tolist()):
        fast += L.orc_sincos2(x, y, out)
        want = (L.orc_sin(ol.LIBM_PORTABLE, x), L.orc_cos(ol.LIBM_PORTABLE, x), L.orc_sin(ol.LIBM_PORTABLE, y), L.orc_cos(ol.LIBM_PORTABLE, y))
        assert np.array(out[:]).tobytes() == np.array(want).tobytes(), (x, y, out[:], want)
    assert fast > N // 2          # the fast block is what camera lenses use
    assert L.orc_sincos2(0.0, 0.3, out) == 0 and L.orc_sincos2(0.3, 1.0, out) == 0 and L.orc_sincos2(0.3, -0.5, out) == 1


def test_pow_is_correctly_rounded():
    L = _lib()
    rng = np.random.default_rng(12)
    # bases: 1 + sums of material absorptions (a few of 0.05 .. 7); exponents: 1 + falloff in [1, 3]
    xs = np.concatenate([1 + rng.uniform(0, 30, N), 1 + rng.integers(1, 200, N // 4) * 0.25, rng.uniform(0.01, 1.0, N // 4)])
    ys = np.concatenate([rng.uniform(1.0, 3.0, N), np.full(N // 4, 1.25), rng.uniform(0.1, 4.0, N // 4)])
    bad = glibc_bad = 0
    for x, y in zip(xs.tolist(), ys.tolist()):
        v = _correct(mpmath.power, x, y)
        bad += L.orc_pow(ol.LIBM_PORTABLE, x, y) != v
        glibc_bad += L.orc_pow(ol.LIBM_GLIBC, x, y) != v
    assert bad == 0, (bad, glibc_bad)
    assert L.orc_pow(ol.LIBM_PORTABLE, 1.0, 1.25) == 1.0 and L.orc_pow(ol.LIBM_PORTABLE, 4.0, 0.5) == 2.0


def test_known_answers_from_cpython():
    """tests/golden/kat_math.json: math.sin / math.cos / ** of the build container's CPython (glibc) on the reference's
    call pattern ([argument(s)..., value] as hex floats).  The portable functions agree wherever glibc itself is
    correctly rounded, and are the correctly rounded value where it is not."""
    import json
    import os
    kat = json.load(open(os.path.join(ol.GOLDEN, "kat_math.json")))
    L = _lib()
    n = same = 0
    for name, fn, ref in (("sin", lambda a: L.orc_sin(ol.LIBM_PORTABLE, a[0]), mpmath.sin),
                          ("cos", lambda a: L.orc_cos(ol.LIBM_PORTABLE, a[0]), mpmath.cos),
                          ("pow", lambda a: L.orc_pow(ol.LIBM_PORTABLE, a[0], a[1]), mpmath.power)):
        for rec in kat[name]:
            vals = [float.fromhex(v) for v in rec]
            args, want = vals[:-1], vals[-1]
            got = fn(args)
            n += 1
            if got == want:
                same += 1
            else:
                assert got == _correct(ref, *args), (name, args)
    assert n > 100 and same / n > 0.99, (n, same)


def _kat_dist():
    import gzip
    import json
    import os
    with gzip.open(os.path.join(ol.GOLDEN, "kat_dist.json.gz"), "rt") as f:
        kat = json.load(f)
    return kat, {k: [[float.fromhex(v) for v in rec] for rec in recs] for k, recs in kat["vectors"].items()}


def _naive_dist(dx, dy, dz):
    return float(np.sqrt(np.float64(dx) * np.float64(dx) + np.float64(dy) * np.float64(dy) + np.float64(dz) * np.float64(dz)))


def test_dist3_known_answers_from_cpython():
    """tests/golden/kat_dist.json.gz: math.dist(chunk centre, camera) of the CPython that produced the golden fixtures
    ([cx, cy, cz, px, py, pz, value] as hex floats; tests/golden/make_kat_dist.py), about 2,000 pairs in six families.
    vrt_dist3 of the three rounded differences equals every value bit for bit; the naive formula misses the number of them
    the generator counted, at least one in ten.  The expected values come from the file, never from this interpreter."""
    kat, fam = _kat_dist()
    assert kat["cpython"].startswith("3.") and set(fam) == {"integer", "far", "exact", "pythagorean", "boundary", "tiny"}
    L = _lib()
    n = naive_bad = 0
    for name, vecs in fam.items():
        assert len(vecs) >= 150, name
        for cx, cy, cz, px, py, pz, want in vecs:
            d = (cx - px, cy - py, cz - pz)
            got = L.orc_dist3(*d)
            assert got == want and not np.signbit(got), (name, [v.hex() for v in (cx, cy, cz, px, py, pz)], got.hex(), want.hex())
            naive_bad += _naive_dist(*d) != want
            n += 1
    assert n >= 1900 and naive_bad == kat["naive_misses"] and naive_bad >= n // 10, (n, naive_bad)
    # a difference's sign and order do not matter; zero differences never divide
    assert L.orc_dist3(0.0, 0.0, 0.0) == 0.0 and L.orc_dist3(-0.0, 0.0, -3.0) == 3.0 and L.orc_dist3(3.0, -4.0, 0.0) == 5.0


def test_dist3_is_correctly_rounded():
    """vrt_dist3 against sqrt(dx^2 + dy^2 + dz^2) of the rounded differences, correctly rounded (mpmath, 300 bits), on the
    kat_dist.json.gz pairs and 20,000 fresh ones: integer chunk centres against float cameras near the origin and 2^24 .. 2^28
    cells out, cameras on halves, differences below 1.  The naive formula is counted beside it and misses thousands."""
    _, fam = _kat_dist()
    L = _lib()
    rng = np.random.default_rng(14)
    diffs = [(cx - px, cy - py, cz - pz) for vecs in fam.values() for cx, cy, cz, px, py, pz, _ in vecs]
    c = np.concatenate([rng.integers(-320, 320, (N // 2, 3)) * 8 + 4,
                        (rng.integers(1 << 21, 1 << 25, (N // 4, 3)) * 8 + 4) * rng.choice([-1, 1], (N // 4, 3)),
                        rng.integers(-320, 320, (N // 4, 3)) * 8 + 4]).astype(np.float64)
    p = np.concatenate([rng.uniform(-2600, 2600, (N // 2, 3)), c[N // 2:3 * N // 4] + rng.uniform(-300, 300, (N // 4, 3)),
                        c[3 * N // 4:7 * N // 8] + rng.integers(-400, 400, (N // 8, 3)) / 2, c[7 * N // 8:] + rng.uniform(-1, 1, (N // 8, 3))])
    assert len(c) == len(p) == N
    diffs += [tuple(v) for v in (c - p).tolist()]
    bad = naive_bad = 0
    for dx, dy, dz in diffs:
        m = [mpmath.mpf(v) for v in (dx, dy, dz)]
        want = float(mpmath.sqrt(m[0] * m[0] + m[1] * m[1] + m[2] * m[2]))
        bad += L.orc_dist3(dx, dy, dz) != want
        naive_bad += _naive_dist(dx, dy, dz) != want
    assert bad == 0, (bad, naive_bad)
    assert naive_bad > len(diffs) // 10, naive_bad
