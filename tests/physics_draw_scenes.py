"""The scene of tests/golden/physics_fluid.npz (tests/golden/make_physics_draws.py records it from the real reference): a world
with materials of fractional solidity, for the tick that makes the reference's random draws (DeviceWorld.tick(rng=),
vrt_physics_tick_draws).  Described with the vocabulary of tests/physics_scenes.py -- the same dict, the same builder -- but with
materials of its own; plain data, nothing of the GPU is imported.

One pass of 1024 tests of the device holds every kind of test: slab voxels that meet no voxel of the pool (no draw), voxels of
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

SCENES = {"fluid": FLUID}
