"""The scene of tests/golden/physics_follow.npz: a world in which the camera is attached to a falling body (the reference's
Object.set_camera), described once for tests/golden/make_physics_follow.py, which builds it from the real reference's classes,
and for the tests, which build it from this project's.  Plain data on top of tests/physics_scenes.py.

dist_move 24, dist_max 40.  A 32 x 2 x 32 slab at the origin; a 4^3 ball at (6, 10, 0), asleep while the camera is high above
it; a 2^3 dot at (30, 2, 0), out of sight from up there; and, last in the physics order, the 4^3 cube at (0, 40, 0) that carries
the camera at set_camera(vec2(3, 4)): 3 forward and 4 up.  The cube is turned by rot.y = 90, so forward is the x axis but for
the rounding of sin and cos of 45 degrees, and the camera starts at about (3, 44, 0): the fixture's cam_start has the bits.
Under a camera held there the cube falls out of dist_move and stops in mid-air, the ball never wakes and the dot never shows.
Under the camera that follows, the cube lands on the slab, the ball wakes and falls, and the dot comes into view."""
import physics_scenes as ps

FOLLOW = 4            # the cube's place in the physics order
CAM_VEC = [3, 4]      # set_camera(vec2(3, 4))


def _follow():
    spec = ps.scene({"slab": ps.full((32, 2, 32), 0), "ball": ps.full((4, 4, 4), 1), "dot": ps.full((2, 2, 2), 3), "cube": ps.full((4, 4, 4), 0)},
                    [ps.obj("slab", (0, 0, 0), physics=False), ps.obj("ball", (6, 10, 0)), ps.obj("dot", (30, 2, 0), physics=False),
                     ps.obj(None, (3, 3, 3), vel=(1, 0, 0)), ps.obj("cube", (0, 40, 0), rot=(0, 90, 0))], 16, cam=(3.0, 44.0, 0.0), dist_move=24, dist_max=40)
    spec["follow"], spec["cam_vec"] = FOLLOW, CAM_VEC
    return spec


SCENE = _follow()
PATH = ps.fixture_path("follow")


def attach(objects, vec2):
    """set_camera on the followed object, with either project's vec2; returns it."""
    who = objects[SCENE["follow"]]
    who.set_camera(vec2(*SCENE["cam_vec"]))
    return who
