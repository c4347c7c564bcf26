"""The scene of tests/golden/run_flags.npz (tests/golden/make_run_flags.py): 1100 bodies that do not move, each at a distance
from the camera that is one of its limits, the double below it or the double above it -- settings.dist_move for the sleep flag,
settings.dist_max + max(half extent) for visibility -- for the flags DeviceWorld.run works out on the device every tick
(vrt_physics_run.hip: vrt_dist3 against dist_move and dist_max + max(half)).  The file pins what the generating interpreter's
math.dist returned; the tests never ask the running one what the flags should be.  Plain data and a builder; nothing of the
GPU is imported."""
import json
import os

import numpy as np

import physics_scenes as ps

PATH = os.path.join(ps.GOLDEN, "run_flags.npz")
N = 1100                                 # more than one tile of 1024 bodies
DIST_MOVE, DIST_MAX = 24, 40
CAM = [3.3, 2.3, 7.9]                    # no coordinate is a dyadic rational of few bits: the differences round
UP = 1.0                                 # the followed body's attachment, vec2(0, UP): it stands at CAM - (0, UP, 0)
KINDS = ("dot", "plank", None)           # by body: index % 3
SPRITES = {"dot": ps.full((2, 2, 2)), "plank": ps.full((4, 2, 6))}
HALF = {"dot": 1, "plank": 3, None: 0}   # max(half extent): trunc(size / 2)


def settings():
    return dict(ps.BASE, gravity=0.0, dist_move=DIST_MOVE, dist_max=DIST_MAX)


def spec_of(pos, follower=False):
    """The scene as tests/physics_scenes.py describes one: body i at pos[i]; follower: one more body, without a sprite, where
    the attachment vec2(0, UP) puts the camera at CAM."""
    objects = [ps.obj(KINDS[i % 3], [float(c) for c in p], physics=False) for i, p in enumerate(pos)]
    if follower:
        objects.append(ps.obj(None, [CAM[0], CAM[1] - UP, CAM[2]], physics=False))
    return ps.scene(SPRITES, objects, 1, cam=CAM, **settings())


def load():
    """(the arrays of the file, the positions as a list of lists of Python floats)."""
    z = np.load(PATH)
    assert json.loads(bytes(z["spec"]).decode()) == dict(n=N, dist_move=DIST_MOVE, dist_max=DIST_MAX, cam=CAM, up=UP, kinds=list(KINDS),
                                                         half=[HALF[k] for k in KINDS])
    return z, z["pos"].tolist()
