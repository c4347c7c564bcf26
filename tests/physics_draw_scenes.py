"""The scenes of tests/golden/physics_{fluid,brim,classes,crowd_fluid}.npz (tests/golden/make_physics_draws.py records them from
the real reference): worlds with materials of fractional solidity, for the tick that makes the reference's random draws
(DeviceWorld.tick(rng=), vrt_physics_tick_draws).  Described with the vocabulary of tests/physics_scenes.py -- the same dict, the
same builder -- but with materials of their own; plain data, nothing of the GPU is imported.  `fluid` comes first; `brim`,
`classes` and `crowd_fluid`, for the sizes and boundaries the kernel dimensions itself for, are described where they stand.

`fluid`: one pass of 1024 tests of the device holds every kind of test: slab voxels that meet no voxel of the pool (no draw), voxels of
solidity 0, -0.5 and voxels under the raft's dug-out strip (one draw), of solidity 1 and 2.0 under a raft voxel (two draws), and
of solidity 0.25 and 0.75 under a raft voxel (one or two: their own first draw decides).  The raft's slab is 37 x 2 x 31 = 2294
voxels, three passes; a tick makes about 1500 draws, 3000 outputs of the generator, five states of 624 words.
Every weight, friction and elasticity is a dyadic rational; the stripe of solidity 2.0 has friction 2^-53, which is lost when it
is added after the larger terms and kept when added before them, so the order of the friction sum shows."""
import physics_scenes as ps

P53 = ps.P53
SEED = 20261

# by index; solidity 1, 0.25 ("for fluids", the reference's README), 0.5, 0.75, 0, 2.0, -0.5
MATS = [ps.mat(solidity=1, weight=2.0 ** -12, friction=0.5, elasticity=0.0),                 # 0 solid
        ps.mat(solidity=0.25, weight=2.0 ** -12, friction=0.25, elasticity=0.125),          # 1 fluid
        ps.mat(solidity=0.5, weight=2.0 ** -12, friction=0.5, elasticity=0.25),             # 2 half
        ps.mat(solidity=0.75, weight=2.0 ** -11, friction=1.0, elasticity=0.0),             # 3 thick
        ps.mat(solidity=0, weight=2.0 ** -12, friction=1.0, elasticity=1.0),                # 4 never solid
        ps.mat(solidity=2.0, weight=2.0 ** -12, friction=P53, elasticity=0.0),              # 5 more than solid
        ps.mat(solidity=-0.5, weight=2.0 ** -12, friction=1.0, elasticity=1.0)]             # 6 less than not solid

# the pool, 40 x 6 x 34: two solid floor rows, four rows of fluid, and in the top rows stripes along z of every other material
POOL = dict(size=[40, 6, 34], lod=0, boxes=[[[0, 0, 0], [39, 1, 33], 0], [[0, 2, 0], [39, 5, 33], 1],
                                            [[4, 4, 0], [6, 5, 33], 4], [[10, 4, 0], [13, 5, 33], 3], [[18, 4, 0], [19, 5, 33], 5],
                                            [[24, 4, 0], [26, 5, 33], 6], [[30, 4, 0], [31, 5, 33], 0],
                                            [[34, 4, 4], [36, 5, 20], None]])
# the raft, 36 x 2 x 30 of solidity 0.5: a solid strip, a strip dug out again, and one that is never solid
RAFT = dict(size=[36, 2, 30], lod=0, boxes=[[[0, 0, 0], [35, 1, 29], 2], [[0, 0, 0], [35, 1, 2], 0], [[8, 0, 10], [27, 1, 13], None],
                                            [[0, 0, 24], [35, 1, 26], 4]])

FLUID = dict(settings=dict(ps.BASE, friction=2.0 ** -6), cam=[0.0, 0.0, 0.0], materials=MATS,
             sprites={"pool": POOL, "raft": RAFT, "half": ps.full((4, 4, 4), 2), "thick": ps.full((4, 4, 4), 3)},
             objects=[ps.obj("pool", (0, 0, 0), physics=False), ps.obj("raft", (0, 6.5, 0), vel=(0.25, 0, 0.125)),
                      ps.obj("half", (-8, 11, 3), vel=(0, -1, 0)), ps.obj("thick", (21, 7, 0), rot=(0, 90, 0))],
             ticks=24, script={}, seed=SEED)


# ---- full passes ------------------------------------------------------------------------------------------------------------------
# `brim`: three stations 60 apart, each a 40 x 6 x 40 non-physical bath and over it a 32 x 4 x 32 physical plate that comes down
# at 0.5.  The plate stands on half-integer x and z, so its inclusive box is exactly 32 wide and no column of its slab lacks a voxel
# of the plate; at y = 4 its bottom row lies in the bath's top row, so both layers of the slab hold a voxel of the bath under a
# voxel of the plate.  Every step is one blocked step of 32 x 2 x 32 = 2048 tests -- two passes of the device, each of 1024 tests
# that may draw twice -- and the plate never moves.  Stations, in physics order:
#   1  bath of solidity 1, plate of 0.5: every test makes two draws and the plate's decides;
#   2  bath of 0.75, plate of 0.5: every test's own first draw decides whether there is a second;
#   3  bath of 1 - 2^-53 and friction 2^-53 (its first columns: friction 1), plate of solidity 1: every test is undecided, every
#      first draw passes, every test is a contact: 1024 contacts a pass, and a friction sum whose order shows.
NEAR = 1.0 - P53
BRIM_SEED = 20262
BRIM_MATS = [ps.mat(solidity=1, weight=2.0 ** -12, friction=0.5),                                  # 0 solid (bath 1, plate 3)
             ps.mat(solidity=0.5, weight=2.0 ** -12, friction=0.25, elasticity=0.125),             # 1 the plates of 1 and 2
             ps.mat(solidity=0.75, weight=2.0 ** -12, friction=1.0),                               # 2 bath 2
             ps.mat(solidity=NEAR, weight=2.0 ** -12, friction=P53),                               # 3 bath 3
             ps.mat(solidity=NEAR, weight=2.0 ** -12, friction=1.0)]                               # 4 ... its first columns
BRIM_STATIONS = (("bath_solid", "plate_half"), ("bath_thick", "plate_half"), ("bath_near", "plate_solid"))


def _brim():
    sprites = {"bath_solid": ps.full((40, 6, 40), 0), "bath_thick": ps.full((40, 6, 40), 2),
               "bath_near": dict(size=[40, 6, 40], lod=0, boxes=[[[0, 0, 0], [39, 5, 39], 3], [[0, 0, 0], [7, 5, 39], 4]]),
               "plate_half": ps.full((32, 4, 32), 1), "plate_solid": ps.full((32, 4, 32), 0)}
    objects = []
    for i, (bath, plate) in enumerate(BRIM_STATIONS):
        x = 60 * i - 60
        objects += [ps.obj(bath, (x, 0, 0), physics=False), ps.obj(plate, (x + 0.5, 4, 0.5), vel=(0, -0.5, 0))]
    return dict(settings=dict(ps.BASE, friction=2.0 ** -6, dist_move=256, dist_max=256), cam=[0.0, 0.0, 0.0], materials=BRIM_MATS,
                sprites=sprites, objects=objects, ticks=3, script={}, seed=BRIM_SEED)


BRIM = _brim()

# ---- the boundaries of the classes ------------------------------------------------------------------------------------------------
# `classes`: a pool whose top rows are ten stripes along z, two columns each, of the solidities at which the count of draws
# changes -- 1 - 2^-53 (undecided, and passes unless the draw is the largest there is), 1.0, nextafter(1, 2) and +inf (two draws),
# NaN, -inf, -0.0 and 0.0 (one draw, which fails), 2^-53 and 5e-324 (undecided, and pass only a draw of 0.0) -- in a body of
# solidity 0.25.  A raft of solidity 0.5 with a dug-out strip, heavy enough for gravity alone to lift it over min_velocity every
# tick, comes down on the stripes and stays there: one blocked step of 37 x 2 x 31 tests a tick, three passes.
CLASS_SEED = 20264
STRIPES = [NEAR, 1.0, 1.0 + 2.0 ** -52, float("inf"), float("nan"), float("-inf"), -0.0, 0.0, P53, 5e-324]     # materials 0 .. 9
CLASS_MATS = [ps.mat(solidity=s, weight=2.0 ** -12, friction=2.0 ** -(i % 4), elasticity=0.0) for i, s in enumerate(STRIPES)] + [
    ps.mat(solidity=0.5, weight=2.0 ** -12, friction=0.5, elasticity=0.25),                        # 10 the raft
    ps.mat(solidity=0.25, weight=2.0 ** -12, friction=0.25, elasticity=0.125)]                     # 11 the pool's body
CLASS_POOL = dict(size=[40, 6, 34], lod=0, boxes=[[[0, 0, 0], [39, 5, 33], 11]] + [[[6 + 2 * i, 4, 0], [7 + 2 * i, 5, 33], i] for i in range(10)])
CLASS_RAFT = dict(size=[36, 2, 30], lod=0, boxes=[[[0, 0, 0], [35, 1, 29], 10], [[0, 0, 10], [35, 1, 13], None]])
CLASSES = dict(settings=dict(ps.BASE, friction=2.0 ** -6), cam=[0.0, 0.0, 0.0], materials=CLASS_MATS,
               sprites={"pool": CLASS_POOL, "raft": CLASS_RAFT},
               objects=[ps.obj("pool", (0, 0, 0), physics=False), ps.obj("raft", (0, 5.5, 0), vel=(0, -0.25, 0))],
               ticks=8, script={}, seed=CLASS_SEED)

# ---- undecided tests on both sides of body 1024 -----------------------------------------------------------------------------------
# `crowd_fluid`: physics_scenes.CROWD but for two solidities -- material 3 (the bar and block_low, body 1) 0.5, material 4
# (block_high, body 1050) 0.75: the bar's blocked step draws for candidates in both tiles of 1024 bodies.
CROWD_FLUID_SEED = 20263


def _crowd_fluid():
    mats = [dict(m) for m in ps.MATS]
    mats[3]["solidity"], mats[4]["solidity"] = 0.5, 0.75
    return dict(ps.CROWD, materials=mats, seed=CROWD_FLUID_SEED)


CROWD_FLUID = _crowd_fluid()

SCENES = {"fluid": FLUID, "brim": BRIM, "classes": CLASSES, "crowd_fluid": CROWD_FLUID}
