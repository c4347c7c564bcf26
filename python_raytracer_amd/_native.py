"""Build + ctypes binding of the HIP library behind include/vrt.h.

There is no CPU fallback: if the shared object is missing or fails to load, importing this module raises.
"""
import ctypes as C
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
# VRT_DIAG=1 selects the instrumented build (python_raytracer_amd/_vrt_diag.so, -DVRT_DIAG; tools/diag_march.py); VRT_DIAG=2
# the one that also counts how far each march step's speculation got (_vrt_diaghist.so, -DVRT_DIAG_HIST: its extra LDS rows
# may cost a launch the ray pool)
DIAG = os.environ.get("VRT_DIAG", "0") not in ("", "0")
DIAG_HIST = os.environ.get("VRT_DIAG", "0") == "2"
# VRT_SO=<path> loads another build of the same sources instead (tools/build_variant.sh: measurement variants such as
# -DVRT_POOL_SLOTS=32); it is never built or rebuilt from here
SO_OVERRIDE = os.environ.get("VRT_SO", "")
SO_PATH = SO_OVERRIDE or os.path.join(HERE, ("_vrt_diaghist.so" if DIAG_HIST else "_vrt_diag.so") if DIAG else "_vrt.so")
# the translation units of the one library (UNITS: vrt_surface.hip holds the surface pass, vrt_kernels.hip everything else) and
# what they include: a change to any of them rebuilds it
UNITS = [os.path.join(HERE, "csrc", f) for f in ("vrt_kernels.hip", "vrt_surface.hip")]
# the object physics (vrt_physics_tick) is a third unit of the same library, listed on its own
PHYSICS_UNITS = [os.path.join(HERE, "csrc", "vrt_physics.hip")]
# ... and the tick that makes the reference's random draws (vrt_physics_tick_draws) a fourth, with a kernel of its own
PHYSICS_DRAWS_UNITS = [os.path.join(HERE, "csrc", "vrt_physics_draws.hip")]
# ... and many ticks in one launch (vrt_physics_run) a fifth, again with a kernel of its own
PHYSICS_RUN_UNITS = [os.path.join(HERE, "csrc", "vrt_physics_run.hip")]
# ... and that run with the sprites animated (vrt_physics_run_anim) a sixth, again with a kernel of its own
PHYSICS_ANIM_UNITS = [os.path.join(HERE, "csrc", "vrt_physics_anim.hip")]
# ... and the animated run that makes the reference's random draws (vrt_physics_run_draws) a seventh, with kernels of its own
PHYSICS_RUN_DRAWS_UNITS = [os.path.join(HERE, "csrc", "vrt_physics_run_draws.hip")]
# the per-chunk object lists and the two passes that read them (vrt_chunk_lists_build, vrt_voxelize_lists, vrt_hit_owners_lists): an
# eighth, which restates the few helpers of vrt_kernels.hip it needs
CHUNK_LISTS_UNITS = [os.path.join(HERE, "csrc", "vrt_chunk_lists.hip")]
# many what-if runs in one launch, one workgroup each (vrt_physics_run_batch): a ninth, again with a kernel of its own
PHYSICS_BATCH_UNITS = [os.path.join(HERE, "csrc", "vrt_physics_batch.hip")]
# ... and those runs with the reference's random draws, a generator per run (vrt_physics_run_batch_draws): a tenth, likewise
PHYSICS_BATCH_DRAWS_UNITS = [os.path.join(HERE, "csrc", "vrt_physics_batch_draws.hip")]
# ... and the batch that keeps a contact log per run (vrt_physics_run_batch_contacts): an eleventh, with its own helper header
PHYSICS_CONTACTS_UNITS = [os.path.join(HERE, "csrc", "vrt_physics_contacts.hip")]
# ... and the batch that takes scripted accelerations per run, with or without a log (vrt_physics_run_batch_impulses): a twelfth
PHYSICS_IMPULSES_UNITS = [os.path.join(HERE, "csrc", "vrt_physics_impulses.hip")]
SOURCES = UNITS + PHYSICS_UNITS + PHYSICS_DRAWS_UNITS + PHYSICS_RUN_UNITS + PHYSICS_ANIM_UNITS + PHYSICS_RUN_DRAWS_UNITS + CHUNK_LISTS_UNITS + \
    PHYSICS_BATCH_UNITS + PHYSICS_BATCH_DRAWS_UNITS + PHYSICS_CONTACTS_UNITS + PHYSICS_IMPULSES_UNITS + \
    [os.path.join(HERE, "csrc", f) for f in ("vrt_math.h", "vrt_math_consts.h", "vrt_physics_common.h", "vrt_physics_contacts.h")]
SOURCES.append(os.path.join(ROOT, "include", "vrt.h"))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
HIPCC_FLAGS = ["-O3", "--offload-arch=gfx950", "-ffp-contract=off", "-std=c++17", "-fPIC", "-shared"] + \
    (["-DVRT_DIAG"] if DIAG else []) + (["-DVRT_DIAG_HIST"] if DIAG_HIST else [])

ABI_VERSION = 9
SCENE_TABLE_IS_IDENTITY = 1   # vrt_scene.flags
SCENE_LAYOUT_DENSE = 2
ERR_WORKSPACE = -3   # VRT_ERR_WORKSPACE
NCOUNTERS = 8
NPROF = 8
PROF_NAMES = ["rng", "march", "retrace", "resolve", "raygen"]
PLAN_MAGIC = 0x5652544e414c5032
NSTATS = 16
COUNTER_NAMES = ["lookup", "nbr", "resnap", "chunk_get", "hit", "draw", "adv", "broke"]
S_RAYS, S_RNG_RETRACED, S_RNG_EXHAUSTED, S_TRAV_OUTSIDE, S_POOL_GROUPS, S_STALLED, S_LOOKAHEAD_GROUPS = 8, 9, 10, 11, 12, 13, 14
S_RAYGEN_GROUPS = 15
S_CAST_REJECTED = 9   # vrt_cast_rays only: rays the device refused (VRT_S_CAST_REJECTED)
# vrt_hit_owners only (VRT_S_OWNER_*): records examined, resolved to an object, orphans, explained by two chunks
S_OWNER_EXAMINED, S_OWNER_RESOLVED, S_OWNER_ORPHANS, S_OWNER_AMBIGUOUS = 8, 4, 9, 10
# vrt_chunk_lists_build only (VRT_S_LISTS_*): items the lists need, 1 if that is more than their capacity
S_LISTS_ITEMS, S_LISTS_OVERFLOW = 8, 9
LISTS_SENTINEL = 0xFFFFFFFF   # d_offsets[n_chunks] of lists that did not fit: the consumers walk every object
# vrt_hit_surfaces only (VRT_S_SURFACE_*): records examined, resolved, orphans, explained differently by two chunks, refused
# by the device, resolved with no open incoming side
S_SURFACE_EXAMINED, S_SURFACE_RESOLVED, S_SURFACE_ORPHANS, S_SURFACE_AMBIGUOUS, S_SURFACE_INVALID, S_SURFACE_ENCLOSED = 8, 4, 9, 10, 11, 12


def needs_build():
    if SO_OVERRIDE:
        return False
    if not os.path.exists(SO_PATH):
        return True
    t = os.path.getmtime(SO_PATH)
    return any(os.path.getmtime(s) > t for s in SOURCES)


def build(force=False, verbose=False):
    """Compile python_raytracer_amd/_vrt.so for gfx950 (hipcc cross-compiles without a GPU)."""
    if not force and not needs_build():
        return SO_PATH
    cmd = [HIPCC] + HIPCC_FLAGS + UNITS + PHYSICS_UNITS + PHYSICS_DRAWS_UNITS + PHYSICS_RUN_UNITS + PHYSICS_ANIM_UNITS + \
        PHYSICS_RUN_DRAWS_UNITS + CHUNK_LISTS_UNITS + PHYSICS_BATCH_UNITS + PHYSICS_BATCH_DRAWS_UNITS + \
        PHYSICS_CONTACTS_UNITS + PHYSICS_IMPULSES_UNITS + ["-o", SO_PATH]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    return SO_PATH


class VrtSettings(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("samples", C.c_int32), ("chunk_size", C.c_int32),
                ("chunk_radius", C.c_int32), ("has_background", C.c_int32), ("seed_nonce", C.c_uint64),
                ("proportions", C.c_double), ("shutter", C.c_double), ("falloff", C.c_double), ("dof", C.c_double),
                ("dist_min", C.c_double), ("dist_max", C.c_double), ("max_light", C.c_double),
                ("max_bounces", C.c_double), ("lod_bounces", C.c_double), ("lod_samples", C.c_double),
                ("lod_random", C.c_double), ("lod_edge", C.c_double)]


class VrtCamera(C.Structure):
    _fields_ = [("pos", C.c_double * 3), ("rot", C.c_double * 4), ("lens", C.c_double)]


class VrtScene(C.Structure):
    _fields_ = [("origin", C.c_int64 * 3), ("dims", C.c_int32 * 3), ("chunk_size", C.c_int32),
                ("n_slots", C.c_int32), ("n_materials", C.c_int32), ("d_chunk_table", C.c_void_p),
                ("d_voxels", C.c_void_p), ("d_materials", C.c_void_p), ("d_occupancy", C.c_void_p),
                ("max_resolution", C.c_int32), ("flags", C.c_int32), ("d_world_tables", C.c_void_p)]


class VrtObject(C.Structure):
    _fields_ = [("mins", C.c_int32 * 3), ("maxs", C.c_int32 * 3), ("size", C.c_int32 * 3), ("turns", C.c_int32 * 3),
                ("model", C.c_int64), ("remap", C.c_int32), ("pad", C.c_int32)]


class VrtTraversed(C.Structure):
    _fields_ = [("origin", C.c_int64 * 3), ("dims", C.c_int32 * 3), ("reset", C.c_int32), ("d_keys", C.c_void_p)]


RAY_FIELDS = [("x", "<i4"), ("y", "<i4"), ("s", "<i4"), ("color", "<i4", 3), ("alpha", "<i4"), ("ntrav", "<i4"),
              ("counters", "<i4", 8), ("detail", "<f8"), ("energy", "<f8"), ("step", "<f8"), ("life", "<f8"),
              ("bounces", "<f8"), ("pos", "<f8", 3), ("vel", "<f8", 3)]
RAY_BYTES = 152


class VrtHit(C.Structure):
    """vrt_hit (include/vrt.h): one first-hit record, 48 bytes."""
    _fields_ = [("step", C.c_double), ("pos", C.c_double * 3), ("cell", C.c_int32 * 3), ("material", C.c_int32)]


HIT_FIELDS = [("step", "<f8"), ("pos", "<f8", 3), ("cell", "<i4", 3), ("material", "<i4")]
HIT_BYTES = 48


class VrtCastRay(C.Structure):
    """vrt_cast_ray (include/vrt.h): one explicit ray of vrt_cast_rays, 64 bytes."""
    _fields_ = [("origin", C.c_double * 3), ("vel", C.c_double * 3), ("life", C.c_double), ("reserved", C.c_double)]


CAST_RAY_BYTES = 64
HIT_REJECTED = -2   # vrt_hit.material of a ray vrt_cast_rays refused
RAY_REJECTED, RAY_EXHAUSTED = -2, -3   # vrt_ray.s of a ray vrt_shade_rays refused / whose draws ran out
PATH_REJECTED, PATH_EXHAUSTED = -2, -3   # d_counts of a ray vrt_path_rays refused / whose draws ran out
HIT_UNUSED = -1   # vrt_hit.material of an unused sample slot (vrt_first_hit) or an unused slot of a ray's row (vrt_path_rays)
PATH_MAX_HITS = 64   # vrt_path_rays: hit records kept per ray at most
S_PATH_TRUNCATED, S_PATH_RECORDS = 12, 13   # vrt_path_rays only: completed rays with more hits than max_hits / records written


class VrtOwner(C.Structure):
    """vrt_owner (include/vrt.h): which object and which voxel of its model a hit record belongs to, 32 bytes."""
    _fields_ = [("object", C.c_int32), ("resolution", C.c_int32), ("voxel", C.c_int32 * 3), ("local", C.c_int32 * 3)]


OWNER_FIELDS = [("object", "<i4"), ("resolution", "<i4"), ("voxel", "<i4", 3), ("local", "<i4", 3)]
OWNER_BYTES = 32
OWNER_NONE, OWNER_ORPHAN = -1, -2   # vrt_owner.object of a record that is no hit / that no object accounts for


class VrtChunkLists(C.Structure):
    """vrt_chunk_lists (include/vrt.h): the chunk box, the capacity of d_items and the two device arrays, 64 bytes."""
    _fields_ = [("origin", C.c_int64 * 3), ("dims", C.c_int32 * 3), ("chunk_size", C.c_int32), ("n_items_cap", C.c_int64),
                ("d_offsets", C.c_void_p), ("d_items", C.c_void_p)]


class VrtSurface(C.Structure):
    """vrt_surface (include/vrt.h): how the surface lies at a hit record -- the velocity after the reflection, the position
    one step on, the normal, what the neighbour lookups asked and found, 64 bytes."""
    _fields_ = [("vel", C.c_double * 3), ("next", C.c_double * 3), ("normal", C.c_int8 * 3), ("status", C.c_int8),
                ("neighbour", C.c_uint8 * 3), ("resolution", C.c_uint8), ("reflect", C.c_uint8), ("side", C.c_uint8),
                ("fetched", C.c_uint8), ("open", C.c_uint8), ("pad", C.c_uint8 * 4)]


SURFACE_FIELDS = [("vel", "<f8", 3), ("next", "<f8", 3), ("normal", "i1", 3), ("status", "i1"), ("neighbour", "u1", 3),
                  ("resolution", "u1"), ("reflect", "u1"), ("side", "u1"), ("fetched", "u1"), ("open", "u1"), ("pad", "u1", 4)]
SURFACE_BYTES = 64
SURFACE_OK, SURFACE_NONE, SURFACE_ORPHAN, SURFACE_INVALID = 0, -1, -2, -3   # vrt_surface.status


class VrtEdit(C.Structure):
    """vrt_edit (include/vrt.h): one box of a model set to a local material id (0 clears), 64 bytes."""
    _fields_ = [("model", C.c_int64), ("size", C.c_int32 * 3), ("lo", C.c_int32 * 3), ("hi", C.c_int32 * 3),
                ("value", C.c_int32), ("force", C.c_int32), ("pad", C.c_int32 * 3)]


EDIT_FIELDS = [("model", "<i8"), ("size", "<i4", 3), ("lo", "<i4", 3), ("hi", "<i4", 3), ("value", "<i4"), ("force", "<i4"),
               ("pad", "<i4", 3)]
EDIT_BYTES = 64
S_EDIT_INVALID = 9   # vrt_edit_models only (VRT_S_EDIT_INVALID): records the device refused


class VrtBody(C.Structure):
    """vrt_body (include/vrt.h): one object of a physics tick, 192 bytes; `object` is its vrt_object."""
    _fields_ = [("pos", C.c_double * 3), ("vel", C.c_double * 3), ("weight", C.c_double), ("object", VrtObject),
                ("half", C.c_int32 * 3), ("visible_before", C.c_int32), ("visible_now", C.c_int32), ("awake", C.c_int32),
                ("physics", C.c_int32), ("has_sprite", C.c_int32), ("steps", C.c_int32), ("blocked_steps", C.c_int32),
                ("contacts", C.c_int32), ("transfers", C.c_int32), ("moved", C.c_int32), ("status", C.c_int32),
                ("rim", C.c_int64), ("pad", C.c_int32 * 2)]


OBJECT_FIELDS = [("mins", "<i4", 3), ("maxs", "<i4", 3), ("size", "<i4", 3), ("turns", "<i4", 3), ("model", "<i8"), ("remap", "<i4"),
                 ("pad", "<i4")]
BODY_FIELDS = [("pos", "<f8", 3), ("vel", "<f8", 3), ("weight", "<f8"), ("object", OBJECT_FIELDS), ("half", "<i4", 3),
               ("visible_before", "<i4"), ("visible_now", "<i4"), ("awake", "<i4"), ("physics", "<i4"), ("has_sprite", "<i4"),
               ("steps", "<i4"), ("blocked_steps", "<i4"), ("contacts", "<i4"), ("transfers", "<i4"), ("moved", "<i4"),
               ("status", "<i4"), ("rim", "<i8"), ("pad", "<i4", 2)]
BODY_BYTES = 192
BODY_OK, BODY_SKIPPED, BODY_REFUSED = 0, -1, -3   # vrt_body.status


class VrtPhysicsParams(C.Structure):
    """vrt_physics_params (include/vrt.h): the [PHYSICS] settings a tick reads."""
    _fields_ = [("gravity", C.c_double), ("friction", C.c_double), ("friction_air", C.c_double), ("min_velocity", C.c_double),
                ("max_velocity", C.c_double)]


# vrt_physics_tick only (VRT_S_PHYSICS_*): bodies stepped, refused, steps, blocked steps, contacts, transfers, iteration-cap hits
S_PHYSICS_BODIES, S_PHYSICS_REFUSED, S_PHYSICS_STEPS, S_PHYSICS_BLOCKED = 8, 9, 10, 11
S_PHYSICS_CONTACTS, S_PHYSICS_TRANSFERS, S_PHYSICS_CAPPED = 12, 13, 14
# vrt_physics_tick_draws only: the index word of d_rng was out of range (the tick did nothing), random.random() calls of the tick
S_PHYSICS_RNG_INVALID, S_PHYSICS_DRAWS = 7, 15
RNG_WORDS = 625   # d_rng of vrt_physics_tick_draws: random.Random.getstate()[1]
PHYSICS_MAX_VEL, PHYSICS_MAX_HALF, PHYSICS_STEP_CAP = 1024, 1024, 3 * (1024 + 2)


class VrtPhysicsRunParams(C.Structure):
    """vrt_physics_run_params (include/vrt.h): the camera, its attachment, the two distances, the work budget and the ticks of
    one vrt_physics_run launch, 80 bytes."""
    _fields_ = [("cam", C.c_double * 3), ("offset", C.c_double * 3), ("dist_max", C.c_double), ("dist_move", C.c_double),
                ("budget", C.c_int64), ("n_ticks", C.c_int32), ("follow", C.c_int32)]


class VrtBodySample(C.Structure):
    """vrt_body_sample (include/vrt.h): one body after one tick of vrt_physics_run, 104 bytes."""
    _fields_ = [("pos", C.c_double * 3), ("vel", C.c_double * 3), ("mins", C.c_int32 * 3), ("maxs", C.c_int32 * 3),
                ("visible", C.c_int32), ("awake", C.c_int32), ("out", C.c_int32 * 6)]


# (the six `out` words by name: PHYSICS_COUNTER_FIELDS of world.py)
BODY_SAMPLE_FIELDS = [("pos", "<f8", 3), ("vel", "<f8", 3), ("mins", "<i4", 3), ("maxs", "<i4", 3), ("visible", "<i4"), ("awake", "<i4"),
                      ("steps", "<i4"), ("blocked_steps", "<i4"), ("contacts", "<i4"), ("transfers", "<i4"), ("moved", "<i4"),
                      ("status", "<i4")]
BODY_SAMPLE_BYTES = 104
# vrt_physics_run only: work units counted, ticks done by the launch
S_PHYSICS_WORK, S_PHYSICS_TICKS = 5, 6
BODY_EVER_MOVED, BODY_EVER_FLIPPED = 1, 2   # vrt_body.pad[0] after vrt_physics_run
BODY_EVER_SWITCHED = 4   # ... after vrt_physics_run_anim: some tick's anim_update changed the frame at this body's turn
PHYSICS_RUN_BUDGET = 1 << 13   # VRT_PHYSICS_RUN_BUDGET: about 23 ms of the dearest measured work units
PHYSICS_RUN_DRAWS_BUDGET = 1 << 12   # VRT_PHYSICS_RUN_DRAWS_BUDGET: about 15 ms of the dearest measured units with draws (section 6h)
# vrt_physics_run_batch only: runs per launch at most, and the word a run sets whose d_ticks_done entry was out of range
PHYSICS_BATCH_MAX_RUNS, S_PHYSICS_BATCH_BADTICK = 4096, 4


class VrtContact(C.Structure):
    """vrt_contact (include/vrt.h): one record of a run's contact log, 40 bytes."""
    _fields_ = [("tick", C.c_int32), ("mover", C.c_int32), ("other", C.c_int32), ("step", C.c_int32), ("voxel", C.c_int32 * 3),
                ("dir", C.c_int8 * 3), ("mat_other", C.c_uint8), ("mat_mover", C.c_uint8), ("reserved", C.c_uint8 * 7)]


class VrtContactLog(C.Structure):
    """vrt_contact_log (include/vrt.h): the records, counts and mask of vrt_physics_run_batch_contacts, 32 bytes."""
    _fields_ = [("d_records", C.c_void_p), ("d_counts", C.c_void_p), ("d_mask", C.c_void_p), ("capacity", C.c_int32), ("mode", C.c_int32)]


CONTACT_FIELDS = [("tick", "<i4"), ("mover", "<i4"), ("other", "<i4"), ("step", "<i4"), ("voxel", "<i4", 3), ("dir", "i1", 3),
                  ("mat_other", "u1"), ("mat_mover", "u1"), ("reserved", "u1", 7)]
CONTACT_BYTES = 40
CONTACTS_VOXELS, CONTACTS_PAIRS = 0, 1   # vrt_contact_log.mode
CONTACT_MASK_MOVER, CONTACT_MASK_OTHER = 1, 2   # bits of a d_mask byte


class VrtImpulse(C.Structure):
    """vrt_impulse (include/vrt.h): Object.accelerate(vel) on `body` before tick `tick` of a run, 32 bytes."""
    _fields_ = [("tick", C.c_int32), ("body", C.c_int32), ("vel", C.c_double * 3)]


class VrtImpulseList(C.Structure):
    """vrt_impulse_list (include/vrt.h): all runs' entries and the rows' bounds of vrt_physics_run_batch_impulses, 24 bytes."""
    _fields_ = [("d_impulses", C.c_void_p), ("d_first", C.c_void_p), ("total", C.c_int32)]


IMPULSE_FIELDS = [("tick", "<i4"), ("body", "<i4"), ("vel", "<f8", 3)]
IMPULSE_BYTES = 32
PHYSICS_MAX_IMPULSES = 1 << 20   # VRT_PHYSICS_MAX_IMPULSES
S_PHYSICS_IMPULSES, S_PHYSICS_IMPULSES_BAD = 0, 1   # entries applied, entries skipped (vrt_physics_run_batch_impulses only)


class VrtAnimSprite(C.Structure):
    """vrt_anim_sprite (include/vrt.h): one animated sprite of vrt_physics_run_anim, 16 bytes."""
    _fields_ = [("frame", C.c_int32), ("n_frames", C.c_int32), ("first_row", C.c_int32), ("pad", C.c_int32)]


class VrtAnimFrame(C.Structure):
    """vrt_anim_frame (include/vrt.h): where one frame of an animated sprite lies on the device and what it weighs, 32 bytes."""
    _fields_ = [("model", C.c_int64), ("rim", C.c_int64), ("remap", C.c_int32), ("pad", C.c_int32), ("weight", C.c_double)]


class VrtAnimSample(C.Structure):
    """vrt_anim_sample (include/vrt.h): one body's animation state after one tick of vrt_physics_run_anim, 16 bytes."""
    _fields_ = [("weight", C.c_double), ("frame", C.c_int32), ("switched", C.c_int32)]


ANIM_SPRITE_FIELDS = [("frame", "<i4"), ("n_frames", "<i4"), ("first_row", "<i4"), ("pad", "<i4")]
ANIM_FRAME_FIELDS = [("model", "<i8"), ("rim", "<i8"), ("remap", "<i4"), ("pad", "<i4"), ("weight", "<f8")]
ANIM_SAMPLE_FIELDS = [("weight", "<f8"), ("frame", "<i4"), ("switched", "<i4")]
ANIM_SPRITE_BYTES, ANIM_FRAME_BYTES, ANIM_SAMPLE_BYTES = 16, 32, 16

_lib = None


class VrtError(RuntimeError):
    pass


def lib():
    """Load the shared object (building it first if the sources are newer)."""
    global _lib
    if _lib is not None:
        return _lib
    if needs_build():
        if not os.path.exists(HIPCC):
            raise ImportError("python_raytracer_amd/_vrt.so is missing and hipcc is not available to build it; "
                              "run `python -c 'import __graft_entry__ as g; g.build()'` on a ROCm machine")
        build()
    L = C.CDLL(SO_PATH)
    vp, i64, i32 = C.c_void_p, C.c_int64, C.c_int32
    L.vrt_abi_version.restype = C.c_int
    L.vrt_status_string.restype = C.c_char_p
    L.vrt_status_string.argtypes = [C.c_int]
    L.vrt_last_hip_error.restype = C.c_int
    L.vrt_release_caches.restype = C.c_int
    L.vrt_device_count.restype = C.c_int
    L.vrt_device_count.argtypes = [C.POINTER(C.c_int)]
    L.vrt_voxel_offset.restype = i64
    L.vrt_voxel_offset.argtypes = [i32, i32, i32, i32]
    L.vrt_max_samples.restype = i32
    L.vrt_max_samples.argtypes = [C.POINTER(VrtSettings)]
    L.vrt_plan_bytes.restype = C.c_int
    L.vrt_plan_bytes.argtypes = [C.POINTER(VrtSettings), i64, C.POINTER(i64), C.POINTER(i64)]
    L.vrt_plan_build.restype = C.c_int
    L.vrt_plan_build.argtypes = [C.POINTER(VrtSettings), vp, i64, vp, i64, vp, i64, vp]
    L.vrt_workspace_bytes.restype = C.c_int
    L.vrt_workspace_bytes.argtypes = [C.POINTER(VrtSettings), i64, i64, i32, i32, C.POINTER(i64)]
    L.vrt_render_tile.restype = C.c_int
    L.vrt_render_tile.argtypes = [C.POINTER(VrtScene), C.POINTER(VrtSettings), C.POINTER(VrtCamera), vp, i64, vp, i64,
                                  i32, vp, vp, vp, i64, vp, vp, vp, vp, vp, C.POINTER(VrtTraversed), vp]
    L.vrt_views_workspace_bytes.restype = C.c_int
    L.vrt_views_workspace_bytes.argtypes = [C.POINTER(VrtSettings), i32, i64, C.POINTER(i64)]
    L.vrt_render_views.restype = C.c_int
    L.vrt_render_views.argtypes = [C.POINTER(VrtScene), C.POINTER(VrtSettings), vp, i32, vp, i64, vp, i64, i32, vp, vp, vp, i64,
                                   vp, vp, vp, vp, vp, C.POINTER(VrtTraversed), vp]
    L.vrt_first_hit.restype = C.c_int
    L.vrt_first_hit.argtypes = [C.POINTER(VrtScene), C.POINTER(VrtSettings), C.POINTER(VrtCamera), vp, i64, vp, i64, vp, i32,
                                vp, vp, vp]
    L.vrt_first_hit_views_workspace_bytes.restype = C.c_int
    L.vrt_first_hit_views_workspace_bytes.argtypes = [i32, C.POINTER(i64)]
    L.vrt_first_hit_views.restype = C.c_int
    L.vrt_first_hit_views.argtypes = [C.POINTER(VrtScene), C.POINTER(VrtSettings), vp, i32, vp, i64, vp, i64, vp, i32, vp, i64,
                                      vp, vp, vp]
    L.vrt_cast_rays.restype = C.c_int
    L.vrt_cast_rays.argtypes = [C.POINTER(VrtScene), C.POINTER(VrtSettings), vp, i64, C.c_double, vp, vp, vp]
    L.vrt_shade_workspace_bytes.restype = C.c_int
    L.vrt_shade_workspace_bytes.argtypes = [i64, C.POINTER(i64)]
    L.vrt_shade_rays.restype = C.c_int
    L.vrt_shade_rays.argtypes = [C.POINTER(VrtScene), C.POINTER(VrtSettings), vp, i64, C.c_double, vp, i32, vp, i64, vp, vp, vp,
                                 C.POINTER(VrtTraversed), vp]
    L.vrt_path_workspace_bytes.restype = C.c_int
    L.vrt_path_workspace_bytes.argtypes = [i64, C.POINTER(i64)]
    L.vrt_path_rays.restype = C.c_int
    L.vrt_path_rays.argtypes = [C.POINTER(VrtScene), C.POINTER(VrtSettings), vp, i64, C.c_double, vp, i32, i32, vp, i64, vp, vp, vp,
                                vp, vp]
    L.vrt_pixel_rays.restype = C.c_int
    L.vrt_pixel_rays.argtypes = [C.POINTER(VrtScene), C.POINTER(VrtSettings), C.POINTER(VrtCamera), vp, i64, vp, i64, vp, i32,
                                 vp, vp, vp]
    L.vrt_draw_table_bytes.restype = C.c_int
    L.vrt_draw_table_bytes.argtypes = [i64, i32, C.POINTER(i64)]
    L.vrt_draw_table_build.restype = C.c_int
    L.vrt_draw_table_build.argtypes = [C.POINTER(VrtSettings), vp, i64, vp, i64, i32, vp, i64, vp]
    L.vrt_ray_table_bytes.restype = C.c_int
    L.vrt_ray_table_bytes.argtypes = [C.POINTER(VrtSettings), i64, C.POINTER(i64)]
    L.vrt_ray_table_build.restype = C.c_int
    L.vrt_ray_table_build.argtypes = [C.POINTER(VrtSettings), C.c_double, vp, i64, vp, vp, i32, vp, i64, vp]
    L.vrt_pow_memo_create.restype = C.c_int
    L.vrt_pow_memo_create.argtypes = [C.c_double]
    L.vrt_occupancy_build.restype = C.c_int
    L.vrt_occupancy_build.argtypes = [vp, i64, vp, vp]
    L.vrt_world_tables_bytes.restype = C.c_int
    L.vrt_world_tables_bytes.argtypes = [C.POINTER(i32), i32, C.POINTER(i64)]
    L.vrt_world_tables_build.restype = C.c_int
    L.vrt_world_tables_build.argtypes = [C.POINTER(i32), i32, vp, i64, vp]
    L.vrt_trace_workspace_bytes.restype = C.c_int
    L.vrt_trace_workspace_bytes.argtypes = [i64, C.POINTER(i64)]
    L.vrt_trace_rays.restype = C.c_int
    L.vrt_trace_rays.argtypes = [C.POINTER(VrtScene), C.POINTER(VrtSettings), C.POINTER(VrtCamera), vp, vp, vp, vp, i32,
                                 i64, vp, i64, vp, vp, C.POINTER(VrtTraversed), vp]
    L.vrt_rng_draws.restype = C.c_int
    L.vrt_rng_draws.argtypes = [vp, i64, i32, vp, vp]
    L.vrt_select_chunks.restype = C.c_int
    L.vrt_select_chunks.argtypes = [vp, C.POINTER(i64), C.POINTER(i32), i32, C.POINTER(C.c_double), C.c_double, i32, i32,
                                    C.POINTER(VrtTraversed), vp, vp]
    L.vrt_voxelize.restype = C.c_int
    L.vrt_voxelize.argtypes = [vp, i32, vp, vp, C.POINTER(i64), C.POINTER(i32), i32, vp, i64, vp, vp, vp]
    L.vrt_hit_owners.restype = C.c_int
    L.vrt_hit_owners.argtypes = [C.POINTER(VrtScene), vp, i64, vp, i32, vp, vp, vp, vp, vp]
    L.vrt_chunk_lists_build.restype = C.c_int
    L.vrt_chunk_lists_build.argtypes = [vp, i32, C.POINTER(VrtChunkLists), vp, vp]
    L.vrt_voxelize_lists.restype = C.c_int
    L.vrt_voxelize_lists.argtypes = L.vrt_voxelize.argtypes[:-1] + [C.POINTER(VrtChunkLists), vp]
    L.vrt_hit_owners_lists.restype = C.c_int
    L.vrt_hit_owners_lists.argtypes = [C.POINTER(VrtScene), vp, i64, vp, i32, vp, vp, vp, C.POINTER(VrtChunkLists), vp, vp]
    L.vrt_hit_surfaces.restype = C.c_int
    L.vrt_hit_surfaces.argtypes = [C.POINTER(VrtScene), vp, vp, i64, vp, vp, vp]
    L.vrt_edit_models.restype = C.c_int
    L.vrt_edit_models.argtypes = [vp, i64, vp, i32, vp, vp]
    L.vrt_stamp_model.restype = C.c_int
    L.vrt_stamp_model.argtypes = [vp, i64, i64, i64, C.POINTER(i32), vp, i32, vp]
    L.vrt_physics_tick.restype = C.c_int
    L.vrt_physics_tick.argtypes = [vp, i32, vp, i64, vp, i32, vp, i32, C.POINTER(VrtPhysicsParams), vp, vp]
    L.vrt_physics_tick_draws.restype = C.c_int
    L.vrt_physics_tick_draws.argtypes = [vp, i32, vp, i64, vp, i32, vp, i32, C.POINTER(VrtPhysicsParams), vp, vp, vp]
    L.vrt_physics_run.restype = C.c_int
    L.vrt_physics_run.argtypes = [vp, i32, vp, i64, vp, i32, vp, i32, C.POINTER(VrtPhysicsParams), C.POINTER(VrtPhysicsRunParams),
                                  vp, vp, vp]
    L.vrt_physics_run_anim.restype = C.c_int
    L.vrt_physics_run_anim.argtypes = L.vrt_physics_run.argtypes + [vp, vp, i32, vp, i32, vp, vp]
    L.vrt_physics_run_draws.restype = C.c_int
    L.vrt_physics_run_draws.argtypes = L.vrt_physics_run_anim.argtypes + [vp, vp]
    L.vrt_physics_run_batch.restype = C.c_int
    L.vrt_physics_run_batch.argtypes = [vp, i32, i32, vp, i64, vp, i32, vp, i32, C.POINTER(VrtPhysicsParams), C.POINTER(VrtPhysicsRunParams),
                                        vp, vp, vp, vp]
    L.vrt_physics_run_batch_draws.restype = C.c_int
    L.vrt_physics_run_batch_draws.argtypes = L.vrt_physics_run_batch.argtypes + [vp, vp]
    L.vrt_physics_run_batch_contacts.restype = C.c_int
    L.vrt_physics_run_batch_contacts.argtypes = L.vrt_physics_run_batch_draws.argtypes + [C.POINTER(VrtContactLog)]
    L.vrt_physics_run_batch_impulses.restype = C.c_int
    L.vrt_physics_run_batch_impulses.argtypes = L.vrt_physics_run_batch_contacts.argtypes + [C.POINTER(VrtImpulseList)]
    L.vrt_canvas_blit.restype = C.c_int
    L.vrt_canvas_blit.argtypes = [vp, vp, i32, i32, vp, i64, vp]
    L.vrt_profile_begin.restype = C.c_int
    L.vrt_profile_begin_kinds.restype = C.c_int
    L.vrt_profile_begin_kinds.argtypes = [C.c_uint32]
    L.vrt_profile_end.restype = C.c_int
    L.vrt_profile_end.argtypes = [vp, vp]
    L.vrt_synth_volume.restype = C.c_int
    L.vrt_synth_volume.argtypes = [i32, i32, vp, vp, vp]
    # diagnostic, not part of include/vrt.h: what the calling thread's last frame-march launch kept in LDS (PLAN_* below)
    L.vrt_diag_last_plan.restype = C.c_int
    L.vrt_diag_last_plan.argtypes = [C.POINTER(i64), C.c_int]
    # diagnostic, not part of include/vrt.h: which march instance a launch with the given inputs runs (march_variant below)
    L.vrt_diag_march_variant.restype = C.c_int
    L.vrt_diag_march_variant.argtypes = [C.POINTER(i32), C.c_int, C.c_char_p, C.c_int, C.POINTER(i32)]
    # diagnostic, not part of include/vrt.h: how often this process has launched each kernel instance (launch_census below)
    L.vrt_diag_launch_census.restype = C.c_int
    L.vrt_diag_launch_census.argtypes = [C.c_int, C.c_char_p, C.c_int, C.POINTER(i64)]
    if L.vrt_abi_version() != ABI_VERSION:
        raise ImportError("python_raytracer_amd/_vrt.so has ABI version %d, expected %d"
                          % (L.vrt_abi_version(), ABI_VERSION))
    _lib = L
    return L


EXPORTS = ["vrt_abi_version", "vrt_status_string", "vrt_last_hip_error", "vrt_device_count", "vrt_release_caches", "vrt_voxel_offset",
           "vrt_max_samples", "vrt_plan_bytes", "vrt_plan_build", "vrt_workspace_bytes", "vrt_render_tile",
           "vrt_views_workspace_bytes", "vrt_render_views",
           "vrt_first_hit", "vrt_first_hit_views_workspace_bytes", "vrt_first_hit_views", "vrt_cast_rays",
           "vrt_shade_workspace_bytes", "vrt_shade_rays", "vrt_path_workspace_bytes", "vrt_path_rays", "vrt_pixel_rays",
           "vrt_draw_table_bytes", "vrt_draw_table_build", "vrt_ray_table_bytes", "vrt_ray_table_build",
           "vrt_pow_memo_create", "vrt_occupancy_build", "vrt_canvas_blit", "vrt_world_tables_bytes", "vrt_world_tables_build",
           "vrt_trace_workspace_bytes", "vrt_trace_rays", "vrt_rng_draws",
           "vrt_synth_volume", "vrt_profile_begin", "vrt_profile_begin_kinds", "vrt_profile_end", "vrt_select_chunks", "vrt_voxelize",
           "vrt_hit_owners", "vrt_chunk_lists_build", "vrt_voxelize_lists", "vrt_hit_owners_lists", "vrt_hit_surfaces", "vrt_edit_models", "vrt_stamp_model", "vrt_physics_tick",
           "vrt_physics_tick_draws", "vrt_physics_run", "vrt_physics_run_batch", "vrt_physics_run_batch_draws",
           "vrt_physics_run_batch_contacts", "vrt_physics_run_batch_impulses",
           "vrt_physics_run_draws", "vrt_physics_run_anim"]


PLAN_FIELDS = ("launches", "pool", "wt_on", "trav_words", "bm_window", "ct_cells", "n_materials", "dyn_bytes", "static_bytes")
PLAN_PROBE_FIELDS = ("wt_on", "trav_words", "dyn_bytes", "static_bytes", "groups_per_cu")


def last_plan():
    """vrt_diag_last_plan as a dict: PLAN_FIELDS of the calling thread's last frame-march launch, and `probes`: one dict of
    PLAN_PROBE_FIELDS per configuration the ray pool's planner asked the runtime about, in the order it tried them."""
    L = lib()
    n = L.vrt_diag_last_plan((C.c_int64 * 1)(), 0)
    if n < 0:
        check(n, "vrt_diag_last_plan")
    buf = (C.c_int64 * n)()
    L.vrt_diag_last_plan(buf, n)
    w = [int(v) for v in buf]
    plan = dict(zip(PLAN_FIELDS, w))
    k = len(PLAN_FIELDS) + 1
    plan["probes"] = [dict(zip(PLAN_PROBE_FIELDS, w[k + 5 * i:k + 5 * i + 5])) for i in range(w[len(PLAN_FIELDS)])]
    return plan


VARIANT_INPUTS = ("record", "list", "list_seed", "pool", "resmode", "deep", "per_pixel", "wt_on", "keys", "trav_words", "bm_window",
                  "big_scene", "tile_heads", "occ", "lookup", "defer_visit")
VARIANT_DEFAULTS = {**dict.fromkeys(VARIANT_INPUTS, 0), "bm_window": -1, "defer_visit": 1}


def march_variant(**inputs):
    """vrt_diag_march_variant: the march instance a launch with these VARIANT_INPUTS runs (those not given: no records, no
    list, no pool, resolution mode 0, nothing set, VRT_DEFER_VISIT unset), as (status, name, effects) -- name with every
    template argument, effects the launch's (wt_on, trav_words, tile heads still set); name and effects are None unless status is 0.
    Host memory only: needs no GPU."""
    unknown = set(inputs) - set(VARIANT_INPUTS)
    if unknown:
        raise TypeError("unknown inputs: %s" % sorted(unknown))
    words = (C.c_int32 * len(VARIANT_INPUTS))(*[int({**VARIANT_DEFAULTS, **inputs}[k]) for k in VARIANT_INPUTS])
    name, effects = C.create_string_buffer(128), (C.c_int32 * 3)()
    status = lib().vrt_diag_march_variant(words, len(VARIANT_INPUTS), name, len(name), effects)
    return (status, name.value.decode(), tuple(effects)) if status == 0 else (status, None, None)


def launch_census():
    """vrt_diag_launch_census as {instance name with every template argument: launches since the process started}: the rows
    of the march table (launch_march: frames, records, re-traces), then the instances of the families chosen by resolution
    mode (batched views and their re-traces, first hit, cast, shade).  Host memory only: needs no GPU, synchronises nothing."""
    L = lib()
    name, count = C.create_string_buffer(128), C.c_int64(0)
    census, row, n = {}, 0, 1
    while row < n:
        n = L.vrt_diag_launch_census(row, name, len(name), C.byref(count))
        if n < 0:
            check(n, "vrt_diag_launch_census")
        census[name.value.decode()] = int(count.value)
        row += 1
    return census


def check(status, what):
    if status != 0:
        L = lib()
        msg = L.vrt_status_string(status).decode()
        if status == -2:
            msg += " (hipError %d)" % L.vrt_last_hip_error()
        raise VrtError("%s failed: %s" % (what, msg))
