"""Scripts for the tests that keep ONE Camera and ONE DeviceWorld alive while things change underneath them
(tests/test_gpu_sequences.py), and what every step of them expects.  Plain definitions: no pytest marks, nothing of the GPU is
imported.  tests/test_sequences_host.py asserts on the CPU, from the oracle and the host world alone, that the scripts reach
what their steps are named for.

Walk A (walk_a): one camera over the default scene, one settings store, a walk through every setting the library reads.  A
Shot is one render call with the complete state it is made in -- so the oracle and a fresh camera can restate it from
scratch -- the changes that lead to it from the previous shot, and the cached objects the camera must rebuild for it:
"pixels" (the uploaded pixel list of the thread), "plan", "draw" and "ray" (DevicePixels.plan, draw_table, ray_table).

Script B (ScriptB): nine objects over seven sprites in a world of 8^3-voxel chunks, 40 ticks of one to three operations
each, then DeviceWorld.update().  The script carries its own model of what update() has to do: the merge order
(DeviceWorld.merge_order's rule, applied here), the world box, and the number of chunks a tick rebuilds (from the old and
the new boxes of the objects that redraw and from edit_world_box of the edits made without redraw)."""
import numpy as np

import oracle_lib as ol

# ---------------------------------------------------------------------------------------------------------------- walk A
BASE_A = dict(width=40, height=30, samples=2, max_bounces=4.0, threads=1, dof=0.5, lod_samples=0.5, lod_random=0.25,
              lod_edge=0.25)
ALL = frozenset(("pixels", "plan", "draw", "ray"))
TABLES = frozenset(("plan", "draw", "ray"))
RAY = frozenset(("ray",))
NOTHING = frozenset()
NONCE_A = 0x5EED1235           # the non-static frame of step 14 (odd, as Camera draws its own)
MOVED_POS = (1.5, 0.25, -2.0)  # step 1: added to the fixture's camera position
MOVED_ROT = (0.05, 0.3, -0.1, 0.94)
VIEW_OFFSETS = ((0.0, 0.0, 0.0), (-2.5, 0.5, 1.25))   # step 17: the two poses of render_views, relative to the camera


class Shot:
    """One render of walk A.  st: the oracle-style settings dict of the frame; changes: the settings the step assigns on the
    live store before it (name -> value, derived fields excluded); windows: the (width, height, threads) the step passes through
    finalize_settings, in order, before the render; rebuilt: what the camera must rebuild for this render and nothing more;
    twin: the oracle's frame equals the previous shot's; kind: "render", or "families" (step 17: first_hit, pixel_rays,
    render_views, then the render)."""

    def __init__(self, step, label, st, pos, rot, lens, thread, changes, windows, rebuilt, nonce=0, cache_draws=True,
                 background=True, twin=False, kind="render", lens_scale=None, moved=False):
        self.step, self.label, self.st, self.pos, self.rot, self.lens, self.thread = step, label, st, pos, rot, lens, thread
        self.changes, self.windows, self.rebuilt, self.nonce, self.cache_draws = changes, windows, frozenset(rebuilt), nonce, cache_draws
        self.background, self.twin, self.kind, self.lens_scale, self.moved = background, twin, kind, lens_scale, moved

    @property
    def pixels(self):
        return ol.pixel_lists(self.st["width"], self.st["height"], self.st["threads"])[self.thread]

    def __repr__(self):
        return "Shot(%d %s)" % (self.step, self.label)


def per_pixel(st):
    """ray_table_per_pixel of the library, restated: one ray record per pixel instead of per sample slot."""
    return st["dof"] == 0 and st["lod_random"] == 0 and st["lod_samples"] == 0


_walk = {}


def walk_a():
    """The shots of walk A, in order (built once)."""
    if "a" in _walk:
        return _walk["a"]
    sc = ol.default_scene()
    cur = dict(BASE_A)
    pose = dict(pos=tuple(float(v) for v in sc.cam_pos), rot=tuple(float(v) for v in sc.cam_rot), lens=float(sc.cam_lens))
    shots = []

    def shot(step, label, rebuilt, windows=(), thread=0, lens_scale=None, move=False, **kw):
        extra = {k: kw.pop(k) for k in ("nonce", "cache_draws", "background", "twin", "kind") if k in kw}
        cur.update(kw)
        for w, h, t in windows:
            cur.update(width=w, height=h, threads=t)
        if move:
            pose["pos"] = tuple(float(a + b) for a, b in zip(sc.cam_pos, MOVED_POS))
            pose["rot"] = MOVED_ROT
        if lens_scale is not None:
            pose["lens"] = pose["lens"] * lens_scale
        shots.append(Shot(step, label, ol.make_settings(**cur), pose["pos"], pose["rot"], pose["lens"], thread, dict(kw),
                          tuple(windows), rebuilt, lens_scale=lens_scale, moved=move, **extra))

    shot(0, "baseline", ALL)
    shot(1, "moved and turned", NOTHING, move=True)
    shot(1, "twin", NOTHING, twin=True)
    shot(2, "lens 0.8", RAY, lens_scale=0.8)
    shot(3, "per pixel", RAY, dof=0.0, lod_random=0.0, lod_samples=0.0)
    shot(4, "per slot again", RAY, dof=0.5)
    shot(5, "samples 5", TABLES, samples=5)
    shot(6, "samples 1", TABLES, samples=1)
    shot(7, "unused slots", TABLES, samples=4, lod_edge=1.0, lod_samples=3.0)
    shot(7, "lod_edge alone", TABLES, lod_edge=0.5)            # (the plan's key lists it beside the sample count)
    shot(8, "30x40", ALL, windows=[(30, 40, 1)])
    shot(9, "64x16 then 16x64", ALL, windows=[(64, 16, 1), (16, 64, 1)])
    shot(10, "40x30 thread 0 of 4", ALL, windows=[(40, 30, 4)], thread=0)
    for t in (1, 2, 3):
        shot(10, "thread %d of 4" % t, ALL, thread=t)
    shot(10, "thread 0 again", NOTHING, thread=0)
    shot(11, "dist_max 48", RAY, dist_max=48)
    shot(11, "dist_max 192", RAY, dist_max=192)
    shot(11, "dist_min 4", RAY, dist_min=4)
    shot(12, "falloff 3", NOTHING, falloff=3.0)
    shot(12, "falloff 0", NOTHING, falloff=0.0)
    shot(12, "falloff 0.25", NOTHING, falloff=0.25)
    shot(13, "by value only", NOTHING, max_bounces=0.5, lod_bounces=0.0, shutter=0.0, max_light=4.0)
    shot(14, "not static", NOTHING, static=False, nonce=NONCE_A)
    shot(14, "static again", NOTHING, static=True)
    # (twins besides step 1's: cache_draws and the calls of step 17 are no setting of the oracle's, so its frame cannot differ)
    shot(15, "no cached draws", NOTHING, cache_draws=False, twin=True)
    shot(15, "cached draws again", NOTHING, twin=True)
    shot(16, "no background", NOTHING, background=False)
    shot(16, "background again", NOTHING)
    shot(17, "families", NOTHING, kind="families", twin=True)
    _walk["a"] = shots
    return shots


# the memo leg: 70 falloff values on one camera, a fresh pow table each (the library keeps 64 per process)
MEMO_SETTINGS = dict(width=8, height=8, samples=1, max_bounces=4.0, threads=1)
MEMO_FALLOFFS = [0.03125 * (k + 1) for k in range(70)]
MEMO_HELD = (0, 63, 64, 69)     # the first, the 64th, the 65th and the last are held to the oracle


# --------------------------------------------------------------------------------------------------------------- script B
CS_B = 8
N_TICKS_B = 40
N_RAYS_B = 256
SETTINGS_B = dict(width=32, height=24, samples=2, chunk_size=CS_B, chunk_lod=2, culling=True, dist_max=96, fov=150.0)
CAM_ROT_B = (0.0, 0.0, 0.0, 1.0)     # looks along +z
SELECT_EVERY = 3                     # Camera.chunk_update runs on ticks divisible by this (the reference's chunk_rate)
QUIET_TICKS = (13, 16)               # 13: no operation at all; 16: an operation that changes nothing visible
OPERATIONS = ("move_inside", "move_border", "move_out", "turn_counts", "turn_ignored", "hide", "show", "append", "remove",
              "frame_switch", "set_voxel", "set_voxel+redraw", "set_area", "set_area+redraw", "clear", "clear+redraw", "mix",
              "mix+redraw")
COMBINATIONS = ("edit_and_move", "edit_hidden", "new_material", "rebuild_after_new_material", "edit_shared", "edit_lod",
                "mix_after_edit", "no_operation", "nothing_visible")


def cam_pos_b(k):
    """The camera of script B at tick k: in front of the world on -z, drifting a little every tick."""
    return (-1.5 + 0.75 * (k % 5), 2.25 - 0.5 * (k % 3), -13.5 + 0.125 * k)


def _v(x, y, z):
    from python_raytracer_amd.lib import vec3
    return vec3(x, y, z)


def _extent(spr):
    return tuple(int(v) - 1 for v in (spr.size.x, spr.size.y, spr.size.z))


class ScriptB:
    """The world of script B and its 40 ticks.  run(k) applies tick k's operations to the host objects and sprites and returns
    the tick's expectations; the caller then calls DeviceWorld.update(self.objs) -- or, on the host, done() in its place.
    Everything random is drawn once from numpy.random.default_rng(SEED) in __init__: two instances are the same script.
    o[k] are the nine objects by their first index (self.objs, the list update() gets, loses and gains objects);
    the sprite "cube_b" stands twice (objects 1 and 8) besides "shared" (objects 6 and 7)."""
    SEED = 20250

    def __init__(self):
        from python_raytracer_amd import Material
        from python_raytracer_amd.lib import rgb, material
        from python_raytracer_amd.world import Sprite, Object
        rng = np.random.default_rng(self.SEED)
        self.cs = CS_B
        props = [(0.0, 1.0, 0.0, 0.0), (0.3, 0.5, 0.0, 0.0), (0.1, 0.25, 0.75, 0.0), (0.0, 1.0, 0.0, 1.5), (0.6, 2.0, 0.0, 0.0)]
        self.mats = [Material(function=material, albedo=rgb(25 * i + 5, 250 - 22 * i, (67 * i) % 256), roughness=props[i % 5][0],
                              absorption=props[i % 5][1], ior=props[i % 5][2], energy=props[i % 5][3]) for i in range(10)]
        start, self.late = self.mats[:8], self.mats[8:]            # the two late materials appear only through edits

        def filled(size, frames, lod, fill):
            spr = Sprite(size=_v(*size), frames=frames, lod=lod)
            for f in range(frames):
                spr.get_frame(f).set_voxels({(x, y, z): start[int(rng.integers(len(start)))] for x in range(size[0])
                                             for y in range(size[1]) for z in range(size[2]) if rng.random() < fill}, True)
            return spr

        # seven sprites: two cubic, two with exactly two equal extents, one with lod = 1, one with two frames, one shared
        sizes = dict(cube_a=(8, 8, 8), cube_b=(6, 6, 6), flat_y=(10, 4, 10), flat_x=(4, 8, 8), lod=(8, 6, 10), two=(6, 10, 4),
                     shared=(10, 8, 6))
        self.sprites = {name: filled(size, 2 if name == "two" else 1, 1 if name == "lod" else 0, 0.55)
                        for name, size in sizes.items()}
        self.sprites["new0"] = filled((6, 6, 6), 1, 0, 0.6)        # the brand-new sprites of the two appended objects
        self.sprites["new1"] = filled((4, 10, 8), 1, 0, 0.6)
        # one layer across the camera's view (it looks along +z from z = -13), so that every object shows; the lod sprite and
        # the two hidden objects stand behind others: a ray aimed at them while they are away or hidden meets those
        place = [("cube_a", (4, 4, 4), (0, 0, 0), True), ("cube_b", (13, 4, 4), (0, 90, 0), True),
                 ("flat_y", (4, 13, 6), (0, 0, 0), True), ("flat_x", (9, 8, 5), (90, 0, 0), True),
                 ("lod", (12, -8, 16), (0, 0, 0), True), ("two", (-5, 4, 4), (0, 0, 0), True),
                 ("shared", (12, -7, 6), (0, 0, 0), True), ("shared", (4, 12, 16), (0, 0, 0), False),
                 ("cube_b", (-5, 4, 12), (0, 0, 90), False)]
        self.objs = []
        for name, pos, rot, vis in place:
            ob = Object(pos=_v(*[float(p) for p in pos]), rot=_v(*rot), sprite=self.sprites[name])
            ob.visible = vis
            self.objs.append(ob)
        self.o = list(self.objs)
        self.home = [tuple(float(p) for p in pl[1]) for pl in place]
        self.order = []          # the merge order the device must have: DeviceWorld.merge_order's rule applied here
        self.last = {}           # id(object) -> record key as of its last voxelisation
        self.origin = self.dims = None
        self.edited = set()      # names of the sprites edited so far
        self.tick = -1
        self.ops = []
        self._pending = {}       # (sprite name, frame) -> model box (lo, hi) of this tick's edits made without redraw
        self._world_mats = set() # ids of the materials a voxel of the host world has ever held

    # ---- operations (each names itself in self.ops) ------------------------------------------------------------------------
    def _cells(self, mins, maxs):
        cs = self.cs
        return (tuple(int(v) // cs for v in mins), tuple((int(v) - 1) // cs for v in maxs))

    def move_to(self, ob, pos):
        cs = self.cs
        was = self._cells((ob.mins.x, ob.mins.y, ob.mins.z), (ob.maxs.x, ob.maxs.y, ob.maxs.z))
        ob.move(_v(*[float(p) for p in pos]))
        mn, mx = np.array([ob.mins.x, ob.mins.y, ob.mins.z]), np.array([ob.maxs.x, ob.maxs.y, ob.maxs.z])
        now = self._cells(mn, mx)
        out = (mn < self.origin).any() or (mx > self.origin + self.dims * cs).any()
        self.ops.append("move_out" if out else "move_inside" if was == now else "move_border")

    def move(self, ob, dx, dy, dz):
        self.move_to(ob, (ob.pos.x + dx, ob.pos.y + dy, ob.pos.z + dz))

    def turn(self, ob, axis, quarters=1):
        r = [ob.rot.x, ob.rot.y, ob.rot.z]
        r[axis] += 90 * quarters
        ob.rot = _v(*r)
        ob.redraw = True
        s = (ob.sprite.size.x, ob.sprite.size.y, ob.sprite.size.z)
        self.ops.append("turn_counts" if s[(axis + 1) % 3] == s[(axis + 2) % 3] else "turn_ignored")

    def show(self, ob, visible):
        ob.visible = bool(visible)
        ob.redraw = True
        self.ops.append("show" if visible else "hide")

    def append(self, name, pos):
        from python_raytracer_amd.world import Object
        ob = Object(pos=_v(*[float(p) for p in pos]), rot=_v(0, 0, 0), sprite=self.sprites[name])
        ob.visible = True
        self.objs.append(ob)
        self.o.append(ob)
        self.ops.append("append")
        return ob

    def remove(self, ob):
        self.objs.remove(ob)
        self.ops.append("remove")

    def frame_switch(self, name, frame):
        self.sprites[name].frame = frame
        self.ops.append("frame_switch")

    def _after_edit(self, op, name, lo, hi, redraw, frame=0):
        spr = self.sprites[name]
        self.edited.add(name)
        self.ops.append(op + ("+redraw" if redraw else ""))
        if spr.lod:              # (its model is copied anew: the whole of it may have changed)
            lo, hi = (0, 0, 0), _extent(spr)
        if redraw:
            for ob in self.objs:
                if ob.sprite is spr:
                    ob.redraw = True
        else:
            b = self._pending.get((name, frame))
            self._pending[(name, frame)] = (lo, hi) if b is None else (tuple(min(p, q) for p, q in zip(b[0], lo)),
                                                                    tuple(max(p, q) for p, q in zip(b[1], hi)))

    def set_voxel(self, name, pos, mat, force, redraw):
        self.sprites[name].set_voxel(0, _v(*pos), mat, force)
        self._after_edit("set_voxel", name, tuple(pos), tuple(pos), redraw)

    def set_area(self, name, lo, hi, mat, force, redraw):
        self.sprites[name].set_voxels_area(0, _v(*lo), _v(*hi), mat, force)
        self._after_edit("set_area", name, tuple(lo), tuple(hi), redraw)

    def clear(self, name, redraw):
        self.sprites[name].clear(0)
        self._after_edit("clear", name, (0, 0, 0), _extent(self.sprites[name]), redraw)

    def mix(self, name, source, force, redraw):
        self.sprites[name].mix(self.sprites[source], force)
        self._after_edit("mix", name, (0, 0, 0), _extent(self.sprites[name]), redraw)

    # ---- the ticks --------------------------------------------------------------------------------------------------------
    def _operations(self, k):
        m, late, o, also = self.mats, self.late, self.o, self.ops.append
        if k == 1:
            self.move(o[1], 0, 0, 1)
        elif k == 2:
            self.move(o[2], 1, 0, 0)
            self.set_voxel("cube_a", (2, 3, 0), m[5], True, False)
        elif k == 3:
            self.turn(o[0], 1)                                            # a cube: the turn counts
            self.set_area("cube_b", (0, 0, 0), (1, 1, 1), None, True, True)
        elif k == 4:
            self.turn(o[2], 0)                                            # 10 x 4 x 10 about x: ignored (y != z)
            self.set_area("flat_y", (1, 0, 1), (4, 2, 6), m[2], True, False)
        elif k == 5:
            self.show(o[6], False)
            self.set_area("flat_x", (0, 2, 2), (3, 5, 5), None, True, True)
        elif k == 6:
            self.set_area("cube_a", (6, 6, 0), (7, 7, 1), m[1], True, False)   # an edit and a move of the same object
            self.move(o[0], 0, 3, 0)
            also("edit_and_move")
        elif k == 7:
            self.frame_switch("two", 1)
            self.move(o[1], 0, 0, -1)
        elif k == 8:
            self.set_area("shared", (2, 1, 1), (7, 6, 4), m[6], True, False)   # both its objects are hidden: 6 is shown at 11
            self.move(o[2], -1, 0, 0)
            also("edit_hidden")
        elif k == 9:
            self.move_to(o[3], (33, 8, 5))                                # leaves the world box: a full rebuild
        elif k == 10:
            self.set_area("lod", (2, 2, 2), (5, 3, 7), m[0], True, False) # lod = 1: the model is copied anew
            also("edit_lod")
        elif k == 11:
            self.show(o[6], True)                                         # three ticks after the edit of tick 8
        elif k == 12:
            self.set_area("cube_a", (0, 0, 0), (3, 3, 7), late[0], True, False)   # a material the world has never held
            also("new_material")
        elif k == 13:
            also("no_operation")
        elif k == 14:
            self.set_area("cube_b", (2, 2, 0), (3, 3, 5), late[1], True, False)   # a new material again ...
            self.move_to(o[3], self.home[3])
            also("new_material")
        elif k == 15:
            self.move_to(o[4], (12, -30, 16))                             # ... followed directly by a move out of the box
            also("rebuild_after_new_material")
        elif k == 16:
            self.clear("two", False)                                      # frame 0, while frame 1 is shown
            also("nothing_visible")
        elif k == 17:
            self.append("new0", (-4, 12, 4))
            self.clear("flat_y", False)
        elif k == 18:
            self.set_area("flat_y", (0, 0, 0), (9, 2, 9), m[3], True, True)
            self.turn(o[3], 1)                                            # 4 x 8 x 8 about y: ignored (x != z)
        elif k == 19:
            self.show(o[7], True)
            self.set_voxel("shared", (0, 0, 0), m[4], True, False)
            self.set_area("shared", (0, 0, 5), (9, 7, 5), None, True, False)
            also("edit_shared")
        elif k == 20:
            self.frame_switch("two", 0)                                   # the frame that tick 16 cleared
            self.set_area("two", (1, 1, 0), (4, 8, 3), m[7], False, False)
        elif k == 21:
            self.show(o[8], True)
            self.turn(o[8], 2)                                            # a cube about z: counts
        elif k == 22:
            self.set_area("cube_b", (4, 0, 4), (5, 5, 5), m[2], True, False)   # the source of the mix, edited first
            self.mix("new0", "cube_b", True, False)
            also("mix_after_edit")
        elif k == 23:
            self.remove(o[2])
            self.move_to(o[4], self.home[4])
        elif k == 24:
            self.append("new1", (14, -2, 12))
            self.set_voxel("lod", (4, 4, 4), None, True, True)
            also("edit_lod")
        elif k == 25:
            self.move_to(o[8], (-5, 4, 36))                              # out of the box, between two selections: the camera
                                                                         # marches the new world's own table for two ticks
        elif k == 26:
            self.mix("cube_b", "new0", False, True)
        elif k == 27:
            self.show(o[1], False)
            self.move_to(o[8], self.home[8])
        elif k == 28:
            self.clear("cube_b", True)
        elif k == 29:
            self.set_area("cube_b", (0, 0, 0), (5, 4, 5), m[1], False, False)
            self.show(o[1], True)
        elif k == 30:
            self.set_voxel("cube_b", (0, 5, 0), m[0], True, True)
            self.move(o[6], 2, -1, 1)
        elif k == 31:
            self.remove(o[10])
            self.set_area("shared", (0, 0, 0), (9, 7, 0), None, True, False)
            also("edit_shared")
        elif k == 32:
            self.turn(o[0], 2)
            self.turn(o[1], 0, 2)
        elif k == 33:
            self.set_voxel("two", (0, 0, 0), late[0], True, False)
            self.set_voxel("two", (5, 9, 3), None, True, False)
            self.move(o[0], 0, 0, 8)
        elif k == 34:
            self.move(o[0], 1, 1, 1)
            self.set_voxel("flat_x", (1, 1, 1), m[3], False, True)
        elif k == 35:
            self.show(o[5], False)
            self.set_area("lod", (0, 0, 0), (3, 3, 3), m[6], False, True)
        elif k == 36:
            self.mix("new0", "cube_b", True, False)
        elif k == 37:
            self.clear("new0", True)
            self.move_to(o[1], (9, 5, 3))
        elif k == 38:
            self.set_voxel("flat_x", (3, 7, 7), m[5], True, False)
            self.move(o[5], 0, 0, 9)
        elif k == 39:
            self.mix("cube_b", "new0", True, True)
            self.move(o[3], 0, 0, 1)

    # ---- the model of update() ------------------------------------------------------------------------------------------
    @staticmethod
    def record_key(o):
        turns = tuple(round(r / 90) % 4 for r in (o.rot.x, o.rot.y, o.rot.z))
        return ((int(o.mins.x), int(o.mins.y), int(o.mins.z)), (int(o.maxs.x), int(o.maxs.y), int(o.maxs.z)), turns,
                id(o.sprite), int(o.sprite.frame))

    def _box_of(self, vis):
        cs = self.cs
        lo = np.array([[o.mins.x, o.mins.y, o.mins.z] for o in vis], np.int64).min(0)
        hi = np.array([[o.maxs.x, o.maxs.y, o.maxs.z] for o in vis], np.int64).max(0)
        return (lo // cs) * cs, (hi // cs) - (lo // cs) + 1

    def run(self, k):
        """Apply tick k (they run in order) and return dict(ops, full, chunks, cells, order): whether update() has to fall back
        to a full rebuild, how many chunks it rebuilds (and which: cells of the world box), and the merge order after it.
        Sets self.origin / self.dims: the world box the device keeps (it changes at a full rebuild only)."""
        from python_raytracer_amd.world import edit_world_box
        assert k == self.tick + 1
        self.tick, self.ops, self._pending = k, [], {}
        self._operations(k)
        cs = self.cs
        vis = [o for o in self.objs if o.visible and o.sprite]
        if k == 0:
            self.order = list(vis)
            self.origin, self.dims = self._box_of(vis)
            self.last = {id(o): self.record_key(o) for o in vis}
            return dict(ops=[], full=True, chunks=int(np.prod(self.dims)), cells=None, order=list(self.order))
        vis_ids = {id(o) for o in vis}
        names = {id(s): n for n, s in self.sprites.items()}
        boxes = []
        for o in self.order:                              # edits without redraw: the world image of the edited box
            b = self._pending.get((names[id(o.sprite)], int(o.sprite.frame))) if id(o) in vis_ids else None
            if b is not None:
                w = edit_world_box(o.sprite.size, o.rot, o.mins, o.maxs, b[0], b[1])
                if w is not None:
                    boxes.append(w)
        changed = set()
        for o in self.order:
            rec = self.record_key(o) if id(o) in vis_ids else None
            if rec is None or o.redraw or rec != self.last[id(o)]:
                changed.add(id(o))
                boxes.append(self.last[id(o)][:2])
        have = {id(o) for o in self.order}
        stay = [o for o in self.order if id(o) not in changed]           # DeviceWorld.merge_order's rule
        moved = [o for o in vis if id(o) in changed or id(o) not in have]
        boxes += [self.record_key(o)[:2] for o in moved]
        self.order = stay + moved
        hi_box = self.origin + self.dims * cs
        full = any((np.asarray(mn) < self.origin).any() or (np.asarray(mx) > hi_box).any() for mn, mx in boxes)
        cells = None
        if full:
            self.origin, self.dims = self._box_of(self.order)
            chunks = int(np.prod(self.dims))
        else:
            cells = set()
            for mn, mx in boxes:
                mn, mx = np.asarray(mn, np.int64), np.asarray(mx, np.int64)
                if (mx <= mn).any():
                    continue
                c0, c1 = (mn - self.origin) // cs, (mx - 1 - self.origin) // cs
                cells |= {(x, y, z) for x in range(c0[0], c1[0] + 1) for y in range(c0[1], c1[1] + 1)
                          for z in range(c0[2], c1[2] + 1)}
            chunks = len(cells)
        if boxes:
            self.last = {id(o): self.record_key(o) for o in self.order}
        return dict(ops=list(self.ops), full=full, chunks=chunks, cells=cells, order=list(self.order))

    def done(self):
        """What update() leaves behind on the host objects: the redraw flags of the objects it voxelised are cleared."""
        for o in self.order:
            o.redraw = False

    def host_world(self):
        """build_world(owners=True) over the script's merge order, placed in the box the device keeps: (the World, its grid in
        that box -- build_world's own material numbers: first use in merge order --, its owner grid in that box)."""
        from python_raytracer_amd.world import build_world
        w = build_world(list(self.order), self.cs, owners=True)
        shape = tuple(int(d) * self.cs for d in self.dims)
        grid, own = np.zeros(shape, np.uint8), np.full(shape, -1, np.int32)
        if w.grid.any():   # (build_world's own box may be a layer of empty chunks larger: it counts maxs as inside)
            a = np.asarray(w.origin, np.int64) - self.origin
            lo = np.maximum(a, 0)
            hi = np.minimum(a + w.grid.shape, shape)
            dst = tuple(slice(int(lo[i]), int(hi[i])) for i in range(3))
            src = tuple(slice(int(lo[i] - a[i]), int(hi[i] - a[i])) for i in range(3))
            grid[dst], own[dst] = w.grid[src], w.owner[src]
            assert int((grid != 0).sum()) == int((w.grid != 0).sum())      # nothing of the world lies outside the box
        return w, grid, own

    def make_rays(self):
        """The 256 rays of the owner check, fixed after tick 0: from points around the camera's first position, each towards
        the middle third of the box one of the nine objects has then (the two hidden ones stand in front of others) -- the
        camera's own lines of sight, so that the chunks they cross are chunks a selection with culling keeps -- and on
        behind it."""
        rng = np.random.default_rng(self.SEED + 1)
        org, vel = [], []
        for i in range(N_RAYS_B):
            ob = self.o[i % 9]
            lo = np.array([ob.mins.x, ob.mins.y, ob.mins.z], np.float64)
            ext = np.array([ob.maxs.x, ob.maxs.y, ob.maxs.z], np.float64) - lo
            t = lo + ext * rng.uniform(1 / 3, 2 / 3, 3)
            a = np.asarray(cam_pos_b(0)) + rng.uniform(-1.5, 1.5, 3)
            d = t - a
            org.append(a)
            vel.append(d / np.abs(d).max())
        return np.array(org, np.float64), np.array(vel, np.float64), np.full(N_RAYS_B, 90.0)


def present_of(grid, cs):
    d = [s // cs for s in grid.shape]
    return grid.reshape(d[0], cs, d[1], cs, d[2], cs).any(axis=(1, 3, 5)).astype(np.uint8)


class CameraB:
    """The host's model of the one Camera of script B: which chunk table it marches.  None: the world's own table -- every
    present chunk at resolution 1, as of NOW (after set_world_scene, which a new scene object asks for); else the (present,
    res) of its last chunk_update(), which outlives the ticks in between: slots are cell indices and never move, so a listed
    chunk that has emptied since is all air and a chunk that appeared since is invisible."""

    def __init__(self):
        self.table = None
        self.selected_at = None
        self.traversed = []      # the traversed list of the last frame: what the next selection culls by

    def new_scene(self):
        self.table, self.selected_at = None, None

    def select(self, k, origin, dims, cs, present):
        self.table = fresh_selection(k, origin, dims, cs, present, self.traversed)
        self.selected_at = k

    def scene(self, origin, dims, cs, grid, rows):
        """The oracle_lib.Scene the camera marches over the world grid of this tick (ids and material rows are the caller's)."""
        present, res = self.table if self.table is not None else (present_of(grid, cs), None)
        if res is None:
            res = np.ones_like(present)
        cam_grid = ol.Scene.camera_grid(grid, origin, dims, cs, present, res)
        return ol.Scene(origin, dims, cs, present, res, cam_grid, rows)


def fresh_selection(k, origin, dims, cs, present, traversed):
    st = ol.make_settings(**SETTINGS_B)
    return ol.select_chunks(origin, dims, cs, present, cam_pos_b(k), st["dist_max"], st["chunk_lod"], st["culling"],
                            np.asarray(traversed, np.int64).reshape(-1, 3))


def render_b(k, scene):
    """The oracle's frame of tick k over `scene`."""
    st = ol.make_settings(**SETTINGS_B)
    return ol.render(scene, st, cam_pos_b(k), CAM_ROT_B, st["fov"] * np.pi / 8, ol.pixel_lists(st["width"], st["height"], 1)[0],
                     libm=ol.LIBM_PORTABLE)
