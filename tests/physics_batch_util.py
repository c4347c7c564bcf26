"""What the tests of the batched physics share (tests/test_physics_batch_host.py, tests/test_gpu_physics_batch.py): hand-made twins
of a scene's objects, variants described by the objects' places in the physics order, and the five altered variants every scene is
run with; and the calls of vrt_physics_run_batch that it refuses before any HIP call.  Nothing of the GPU is imported."""
import copy
import ctypes as C

from python_raytracer_amd import _native as nat
from python_raytracer_amd.lib import vec3

VECTORS = ("pos", "rot", "vel", "size", "mins", "maxs", "cam_pos")


def twins(objects):
    """Copies of the objects made here, not by the code under test: new Objects and vectors, the sprites shared."""
    out = []
    for o in objects:
        t = copy.copy(o)
        for f in VECTORS:
            v = getattr(o, f)
            setattr(t, f, vec3(v.x, v.y, v.z))
        out.append(t)
    return out


def mapping(objects, change):
    """A variant of run_many from {index: {"pos": (x, y, z), "vel": (x, y, z)}}."""
    return {objects[k]: {key: vec3(*v) for key, v in c.items()} for k, c in change.items()}


def altered(objects, change):
    """A hand-made twin of the objects with the change applied as the issue defines it: Object.move, the velocity replaced."""
    out = twins(objects)
    for k, c in change.items():
        if "pos" in c:
            out[k].move(vec3(*c["pos"]))
        if "vel" in c:
            out[k].vel = vec3(*c["vel"])
    return out


def changes(objects, cam):
    """{} and five altered variants for any scene: a moved body, a thrown body, both, two bodies, and a body thrown downwards
    over an obstacle that has moved.  `a` is the physical body with a sprite that is nearest to the camera (the first of them:
    awake, if any is), `b` the last other object that has one."""
    near = [(o.pos.distance(vec3(*cam)), k) for k, o in enumerate(objects) if o.physics and o.sprite]
    a = min(near)[1]
    b = [k for k, o in enumerate(objects) if o.sprite and k != a][-1]
    pa, pb = objects[a].pos.tuple(), objects[b].pos.tuple()
    return [{},
            {a: dict(pos=(pa[0] + 1, pa[1] + 2.5, pa[2]))},
            {a: dict(vel=(0.75, -1.5, 0.25))},
            {a: dict(pos=(pa[0] - 0.5, pa[1] + 1, pa[2] + 1.25), vel=(-1.25, 0.5, 0))},
            {a: dict(vel=(0, 2.0, -0.5)), b: dict(pos=(pb[0] + 2, pb[1], pb[2] - 1))},
            {a: dict(vel=(0, -7.5, 0)), b: dict(pos=(pb[0], pb[1] - 1, pb[2]), vel=(0.5, 0, 0))}]


def batch_call(L):
    """vrt_physics_run_batch with made-up device pointers, which nothing reads before the checks are through."""
    fake = 0x1000
    good = nat.VrtPhysicsParams(1.0, 1.0, 0.1, 0.01, 10.0)

    def run_params(**change):
        rp = nat.VrtPhysicsRunParams((C.c_double * 3)(0.0, 4.0, 3.0), (C.c_double * 3)(0.0, 4.0, 3.0), 40.0, 24.0, 1 << 16, 8, 2)
        for k, v in change.items():
            setattr(rp, k, v)
        return rp

    def call(bodies=fake, runs=3, n=4, models=fake, models_bytes=64, remap=fake, remap_bytes=8, matphys=fake, n_materials=3, params=good,
             run=run_params(), done=fake, trace=fake, stats=fake):
        return L.vrt_physics_run_batch(bodies, runs, n, models, models_bytes, remap, remap_bytes, matphys, n_materials,
                                       C.byref(params) if params is not None else None, C.byref(run) if run is not None else None,
                                       done, trace, stats, None)
    return call, run_params, fake


def assert_refusals(L):
    call, run_params, fake = batch_call(L)
    # what vrt_physics_run refuses
    assert call(stats=None) == -1 and call(params=None) == -1 and call(stats=fake + 4) == -1
    assert call(n=-1) == -1 and call(n=(1 << 20) + 1, runs=1) == -1
    assert call(bodies=None) == -1 and call(bodies=fake + 4) == -1 and call(matphys=None) == -1 and call(matphys=fake + 4) == -1
    assert call(models=None) == -1 and call(remap=None) == -1 and call(models_bytes=-1) == -1 and call(remap_bytes=-1) == -1
    assert call(n_materials=-1) == -1 and call(n_materials=256) == -1
    assert call(params=nat.VrtPhysicsParams(1.0, 1.0, float("nan"), 0.01, 10.0)) == -1
    assert call(run=None) == -1 and call(run=run_params(n_ticks=0)) == -1 and call(run=run_params(budget=0)) == -1
    assert call(run=run_params(follow=-2)) == -1 and call(run=run_params(follow=4)) == -1
    assert call(run=run_params(dist_max=float("inf"))) == -1 and call(run=run_params(dist_move=float("nan"))) == -1
    assert call(trace=fake + 4) == -1
    # ... and the batch's own
    assert call(runs=0) == -1 and call(runs=-1) == -1 and call(runs=4097) == -1
    assert call(runs=4096, n=257) == -1 and call(runs=2, n=(1 << 19) + 1) == -1       # n_runs * n_bodies > 2^20
    assert call(done=None) == -1 and call(done=fake + 2) == -1 and call(done=fake + 1) == -1
