"""The scenes of tests/golden/physics_run_draws.npz: worlds in which everything Object.update does per tick comes together -- the
flags from a camera that follows a body, sprites animated under a clock, and materials of fractional solidity decided by the
reference's random draws -- described once for tests/golden/make_physics_run_draws.py, which builds them from the real
reference's classes with random.seed(seed) and a scripted clock, and for the tests, which build them from this project's.
Plain data in the vocabulary of tests/physics_anim_scenes.py (whose builder builds them); nothing of the GPU is imported.

  wade  the cube that carries the camera (set_camera, follow=) falls into a pool of solidity 0.25 over a solid floor.  A second
        physical cube lies in the pool near the floor with a velocity of its own, further from the camera than dist_move: asleep,
        it draws nothing.  The falling cube brings the camera near and wakes it; under a HELD camera it sleeps on, and every tick
        from then on makes other draws.  The cubes are of solidity 0.5 and 0.75: tests against the fluid are undecided.
  tide  two 12 x 2 x 12 platforms show one sprite of three frames -- solid, solidity 0.5, empty -- that the clock switches every
        other tick; a raft of solidity 0.5 rests on each.  In the physics order: raft, platform, raft, platform.  The first
        platform makes every switch: the raft before it has by then drawn against the old frame, the raft after it draws against
        the new one on a platform whose own turn is still to come."""
import json
import os

import physics_anim_scenes as an
import physics_scenes as ps

PATH = os.path.join(ps.GOLDEN, "physics_run_draws.npz")

# by index; every weight, friction and elasticity is a dyadic rational
MATS = [ps.mat(solidity=1, weight=2.0 ** -9, friction=0.5, elasticity=0.0),              # 0 solid
        ps.mat(solidity=0.25, weight=2.0 ** -9, friction=0.25, elasticity=0.125),       # 1 fluid ("for fluids")
        ps.mat(solidity=0.5, weight=2.0 ** -9, friction=0.5, elasticity=0.25),          # 2 half
        ps.mat(solidity=0.75, weight=2.0 ** -9, friction=1.0, elasticity=0.0)]          # 3 thick

SETTINGS = dict(ps.BASE, friction=2.0 ** -4)


def _wade():
    pool = dict(size=[14, 8, 14], lod=0, boxes=[[[0, 0, 0], [13, 1, 13], 0], [[0, 2, 0], [13, 7, 13], 1]])
    spec = dict(settings=dict(SETTINGS, dist_move=11, dist_max=96), cam=[3.0, 14.0, 0.0], materials=MATS,
                sprites={"pool": pool, "wader": ps.full((4, 4, 4), 2), "sleeper": ps.full((4, 4, 4), 3)},
                objects=[ps.obj("pool", (0, 0, 0), physics=False), ps.obj("wader", (0, 10, 0), vel=(0, -1, 0), rot=(0, 90, 0)),
                         ps.obj("sleeper", (3, 1, 2), vel=(0, -0.5, 0))],
                ticks=20, script={}, seed=20271)
    spec["clock"] = [0, 50]
    spec["follow"], spec["cam_vec"] = 1, [3, 4]
    return spec


def _tide():
    plat = an.frames((12, 2, 12), [[an.box((0, 0, 0), (11, 1, 11), 0)], [an.box((0, 0, 0), (11, 1, 11), 2)], []], (0, 2, 0.1))
    spec = dict(settings=dict(SETTINGS), cam=[0.0, 0.0, 0.0], materials=MATS,
                sprites={"plat": plat, "raft": ps.full((8, 2, 8), 2)},
                objects=[ps.obj("raft", (-10, 2, 0)), ps.obj("plat", (-10, 0, 0), physics=False),
                         ps.obj("raft", (10, 2, 0)), ps.obj("plat", (10, 0, 0), physics=False)],
                ticks=14, script={}, seed=20272)
    spec["clock"] = [0, 50]
    return spec


SCENES = {"wade": _wade(), "tide": _tide()}

_fixture = None


def load_fixture():
    """(the arrays of tests/golden/physics_run_draws.npz, {scene name: spec}, what the generator reached), read once."""
    global _fixture
    if _fixture is None:
        import numpy as np
        z = np.load(PATH)
        _fixture = ({k: z[k] for k in z.files}, json.loads(bytes(z["spec"]).decode()), json.loads(bytes(z["reached"]).decode()))
    return _fixture


def fresh(name):
    """The scene from this project's classes as a run finds it, `redraw` cleared: (fixture arrays, spec, objects, sprites, settings
    store, followed object or None)."""
    z, specs, _ = load_fixture()
    spec = specs[name]
    objects, sprites, _, st, who = an.project_scene(spec)
    ps.clear_redraw(objects)
    return z, spec, objects, sprites, st, who


def state_words(generator):
    """The 625 words of a random.Random as numpy uint32."""
    import numpy as np
    return np.array(generator.getstate()[1], np.uint32)
