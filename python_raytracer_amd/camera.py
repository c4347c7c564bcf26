"""Camera: the drop-in entry point of the trace path (reference init.py:13-150).

Same attributes (`pos`, `rot`, `lens`, `chunks`) and methods (`chunk_set`, `chunk_get`, `trace`, `tile`) as the
reference's Camera; the per-pixel / per-ray loops run on the GPU through the C ABI of include/vrt.h
(python_raytracer_amd/_vrt.so).  There is no host fallback.
"""
import ctypes as C
import math
import random

import numpy as np

from . import _native as nat
from . import data as _data
from .lib import vec3, quaternion, rgb, store, is_default_background
from .scene import PackedScene
from .results import RenderResult, HitResult, CastResult, ShadeResult, PathResult, SurfaceResult, _traversed_positions


def _xyz(v):
    return [float(v.x), float(v.y), float(v.z)]


# why a frame's or a batch's rays are left over (d_stats[VRT_S_RNG_EXHAUSTED]): the capacities of include/vrt.h,
# vrt_workspace_bytes, restated for the VrtError of _check_stats
_EXHAUSTED_RULE = ("they consumed more than 1024 random draws (341 rough hits), or a re-trace list of their march launch (at "
                   "most 2**28 ray slots of the %s) was full: more than 4096 rays of the launch needed more than 113 draws, or "
                   "more rays than 1/64 of the launch, held between 2**18 and 2**22 (the whole launch if it is smaller), "
                   "outran the 64-draw table; lower max_bounces or raise material absorption")


def _check_stats(stats, draws, what):
    """What the host statistics (numpy int64[16]) of a "frame" (render) or a "batch" (render_views) marched with `draws`
    draws per seed ask for.  Returns (retry, draws64): retry -- more rays outran the 32-draw table than the re-trace list
    holds: render again with 64; draws64 -- use 64 draws per seed from now on (a retry, or many rays were re-traced).
    Raises VrtError for rays left over at 64 draws and for the internal errors (a batch does not report stalled waves)."""
    frame = what == "frame"
    if stats[nat.S_RNG_EXHAUSTED]:
        if draws == 32:
            return True, True
        raise nat.VrtError("%d rays%s could not be completed: %s"
                           % (int(stats[nat.S_RNG_EXHAUSTED]), "" if frame else " of the batch", _EXHAUSTED_RULE % what))
    if frame and stats[nat.S_STALLED]:
        raise nat.VrtError("%d waves of the march found nothing to run and gave up (internal error, frame "
                           "invalid)" % int(stats[nat.S_STALLED]))
    if stats[nat.S_TRAV_OUTSIDE]:
        raise nat.VrtError("%d chunk visits fell outside the traversed %s (internal bound violated)"
                           % (int(stats[nat.S_TRAV_OUTSIDE]), "box" if frame else "boxes"))
    # many rays outran the 32-draw table and were re-traced: keep 64 draws per seed from now on
    return False, bool(draws == 32 and stats[nat.S_RNG_RETRACED] * 50 > max(1, stats[nat.S_RAYS]))


def _floats(v, name, who, shape, dev, any_dtype=False):
    """Argument `name` of `who` -- a torch tensor or whatever numpy takes -- as a float64 tensor on `dev` of `shape`: one
    entry per dimension, an int for a size that must match, a string for one that is free (and how the message names it).
    Booleans, strings and integer tensors are refused unless `any_dtype` (lives: converted as they are)."""
    import torch
    if isinstance(v, torch.Tensor):
        if not (any_dtype or v.dtype.is_floating_point):
            raise ValueError("%s: %s must be floating point, not %s" % (who, name, v.dtype))
        t = v.to(device=dev, dtype=torch.float64)
    else:
        a = np.asarray(v)
        if not any_dtype and a.dtype.kind not in "fiu":
            raise ValueError("%s: %s must be numbers, not %s" % (who, name, a.dtype))
        t = torch.from_numpy(np.array(a, np.float64)).to(dev)
    if t.dim() != len(shape) or any(isinstance(w, int) and int(g) != w for g, w in zip(t.shape, shape)):
        raise ValueError("%s: %s must have shape [%s], not %s" % (who, name, ", ".join(str(w) for w in shape), list(t.shape)))
    return t


def _seeds(v, n, who, dev):
    """Argument `seeds` of `who` as a contiguous int64 tensor [n] on `dev`.  numpy seeds are range-checked; a torch tensor
    is taken as it is (checking it would synchronise)."""
    import torch
    if isinstance(v, torch.Tensor):
        if v.dtype.is_floating_point or v.dtype == torch.bool:
            raise ValueError("%s: seeds must be integers, not %s" % (who, v.dtype))
        t = v.to(device=dev, dtype=torch.int64)
    else:
        a = np.asarray(v)
        if a.dtype.kind not in "iu" or (a.size and (int(a.min()) < 0 or int(a.max()) >= 1 << 63)):
            raise ValueError("%s: seeds must be integers in [0, 2**63)" % who)
        t = torch.from_numpy(np.array(a, np.int64)).to(dev)
    if t.dim() != 1 or int(t.shape[0]) != n:
        raise ValueError("%s: seeds must have shape [%d], not %s" % (who, n, list(t.shape)))
    return t.contiguous()


def _max_life(max_life, default, who):
    """The bound on how long a lane may march, as `who` was given it (None: `default`)."""
    max_life = float(default if max_life is None else max_life)
    if not (max_life > 0) or max_life > float(1 << 28):
        raise ValueError("%s: max_life must lie in (0, 2**28], not %r" % (who, max_life))
    return max_life


_POW_MEMOS = set()   # (device index, falloff) pairs for which vrt_pow_memo_create has run in this process


def _ensure_pow_memo(torch, dev, falloff):
    """The library's cross-frame pow table for (device, falloff): allocated here, explicitly and outside any stream
    capture, never inside vrt_render_tile / vrt_trace_rays (include/vrt.h)."""
    key = (dev.index, float(falloff))
    if key not in _POW_MEMOS:
        with torch.cuda.device(dev):
            rc = nat.lib().vrt_pow_memo_create(float(falloff))
        # the library keeps at most 64 tables per process (an animated falloff gets there): without one a frame memoises
        # into its own workspace, which only costs speed -- not an error
        if rc != nat.ERR_WORKSPACE:
            nat.check(rc, "vrt_pow_memo_create")
        _POW_MEMOS.add(key)


def release_caches():
    """Free the library's per-(device, falloff) pow tables (vrt_release_caches); the next render re-creates its own."""
    _POW_MEMOS.clear()
    nat.check(nat.lib().vrt_release_caches(), "vrt_release_caches")


class DevicePixels:
    """A pixel list already resident on the device (Camera.upload_pixels), reusable across frames, together with
    its tile plan (the static distinct-seed index of include/vrt.h, built on first use)."""

    def __init__(self, tensor, array):
        self.tensor, self.array = tensor, array
        self.plan = None          # uint8 tensor
        self.plan_key = None
        self.n_distinct = 0
        self.full_frame = False   # the plan found the list to be the whole window
        self.draw_table = None    # uint8 tensor: cached draw table of a static-seed run (Camera.cache_draws)
        self.draw_key = None
        self.ray_table = None     # uint8 tensor: cached lens-quaternion / life table of a static-seed run
        self.ray_key = None
        # the tables are built asynchronously on the stream that was current then: an event per build, and the streams
        # that are already ordered behind it (Camera._order_after_table_builds)
        self.table_events = []
        self.table_streams = set()


class Camera:
    def __init__(self, settings=None, device=None):
        import torch
        self._torch = torch
        self.settings = settings
        s = self._settings()
        self.pos = vec3(0, 0, 0)
        self.rot = quaternion(0, 0, 0, 0)
        self.lens = s.fov * math.pi / 8          # reference init.py:17
        self._chunks = {}
        self._scene = None
        self._scene_dirty = True
        self._materials = []
        self._device = torch.device("cuda", torch.cuda.current_device() if device is None else device) \
            if torch.cuda.is_available() else None
        self._workspace = {}  # per stream
        self._pixel_cache = {}
        self._world = None
        self._camera_table = None
        self._camera_table_max_res = 0
        self._views_cams = None   # (records as bytes, their device copy) of the last batch of poses: _device_poses
        self.last_stats = None
        self.fast_draws = 32   # draws per seed in the frame table (32 | 64): speed only, auto-raised by render()
        # static seeds (settings.static, the reference default) make every frame's random draws -- and with them the
        # lens jitter and the life of every ray -- the same function of (pixel, sample): the draw table and the ray
        # table (include/vrt.h) are built once per pixel list and reused.  cache_draws = False re-seeds MT19937 and
        # regenerates the ray table in every frame instead (what a non-static run has to do anyway).
        self.cache_draws = True

    # ------------------------------------------------------------------ settings / background
    def _settings(self):
        return self.settings if self.settings is not None else _data.settings

    def _has_background(self):
        bg = _data.background
        if bg is None:
            return False
        if not is_default_background(bg):
            raise TypeError("data.background must be lib.material_background or None: a custom background "
                            "callback cannot run inside the GPU kernel")
        return True

    # ------------------------------------------------------------------ chunks (reference init.py:21-33)
    @property
    def chunks(self):
        return self._chunks

    @chunks.setter
    def chunks(self, value):
        self._chunks = value
        self._scene_dirty = True

    def chunk_set(self, post, chunk):
        """Add or clear the Frame of the chunk at position `post` (reference init.py:21-25)."""
        if chunk:
            self._chunks[post] = chunk
            self._scene_dirty = True
        elif post in self._chunks:
            del self._chunks[post]
            self._scene_dirty = True

    def chunk_get(self, pos):
        """Frame of the chunk containing `pos`, or None (reference init.py:28-33)."""
        cs = self._settings().chunk_size
        key = tuple((v // cs) * cs for v in (pos.x, pos.y, pos.z))
        return self._chunks.get(key)

    def invalidate(self):
        """Call after mutating a Frame or Material in place: the packed device copy is a snapshot."""
        self._scene_dirty = True

    def set_packed_scene(self, scene):
        """Use an already flattened scene (PackedScene) instead of `chunks` (bench / fixtures)."""
        self._scene = scene.to(self._require_device())
        self._scene_dirty = False

    # ------------------------------------------------------------------ world scene + per-frame chunk selection
    def set_world_scene(self, scene):
        """Keep every world chunk resident at full resolution (a PackedScene whose table lists all chunks that hold
        voxels); chunk_update() then decides per frame which of them the camera renders and at which LOD."""
        self._world = scene.to(self._require_device())
        self._scene = self._world
        self._scene_dirty = False
        self._camera_table = None
        self._camera_table_max_res = 0

    def chunk_update(self, traversed=None):
        """The selection loop of the reference's Window.chunk_update (init.py:447-452) on the device: keep a world
        chunk iff culling is off or it was traversed, at LOD min(trunc(dist / (dist_max / (1 + chunk_lod))), chunk_lod).
        traversed: the previous frame's RenderResult (its device-side visit keys are used in place), a list / tuple of
        RenderResults of the same frame (one per tile, like the reference's per-thread lists that init.py:393 unpacks
        into one), a list of chunk positions as tile() returns it, or None (nothing traversed).  In a multi-process
        run use multigpu.chunk_update_all_ranks, which unions the keys over the ranks first."""
        torch = self._torch
        L = nat.lib()
        if self._world is None:
            raise RuntimeError("chunk_update() needs set_world_scene() first")
        s = self._settings()
        w = self._world
        cs = int(s.chunk_size)
        dev = self._require_device()
        box = ()   # (origin, dims, keys) of what was traversed
        if isinstance(traversed, (list, tuple)) and traversed and all(isinstance(t, RenderResult) for t in traversed):
            from .multigpu import merge_traversed
            with_keys = [t for t in traversed if t.traversed_keys is not None]
            if any(t.trav_origin != with_keys[0].trav_origin or t.trav_dims != with_keys[0].trav_dims for t in with_keys):
                raise ValueError("the RenderResults were rendered with different cameras (traversed boxes differ)")
            merged = RenderResult()
            if with_keys:
                merged.traversed_keys = merge_traversed([t.traversed_keys for t in with_keys])
                merged.trav_origin, merged.trav_dims = with_keys[0].trav_origin, with_keys[0].trav_dims
            traversed = merged
        if isinstance(traversed, RenderResult):
            if traversed.traversed_keys is not None:
                box = (traversed.trav_origin, traversed.trav_dims, traversed.traversed_keys)
        elif traversed:
            pts = np.asarray([[int(v) for v in p] for p in traversed], np.int64).reshape(-1, 3)
            lo = pts.min(0)
            d = (pts.max(0) - lo) // cs + 1
            host = np.full(tuple(d), -1, np.int64)
            c = (pts - lo) // cs
            host[c[:, 0], c[:, 1], c[:, 2]] = 0
            box = ([int(v) for v in lo], [int(v) for v in d], torch.from_numpy(host.reshape(-1)).to(dev))
        tr, keys = self._key_box(*box)   # (`keys` stays alive until the launch below has been made)
        if self._camera_table is None:
            self._camera_table = torch.zeros_like(w.device_tensors["chunk_table"])
        origin = (C.c_int64 * 3)(*[int(v) for v in w.origin])
        dims = (C.c_int32 * 3)(*[int(v) for v in w.dims])
        pos = (C.c_double * 3)(*_xyz(self.pos))
        with torch.cuda.device(dev):
            nat.check(L.vrt_select_chunks(w.device_tensors["chunk_table"].data_ptr(), origin, dims, cs, pos,
                                          float(s.dist_max), int(s.chunk_lod), 1 if s.culling else 0, C.byref(tr),
                                          self._camera_table.data_ptr(), torch.cuda.current_stream().cuda_stream),
                      "vrt_select_chunks")
        # the largest resolution this selection can have written, from the very position and settings it was made with:
        # the table outlives camera moves (the reference gates chunk_update by chunk_rate but moves cam.pos every frame,
        # init.py:391, 464), and a bound taken from a later, closer position would understate it
        self._camera_table_max_res = self._max_selected_resolution(w)
        return self._camera_table

    # ------------------------------------------------------------------ device plumbing
    def _require_device(self):
        if self._device is None:
            raise RuntimeError("python_raytracer_amd needs a ROCm GPU: torch.cuda.is_available() is False and "
                               "there is no CPU fallback")
        return self._device

    def _ensure_scene(self):
        dev = self._require_device()
        if self._scene is None or self._scene_dirty:
            sc, mats = PackedScene.from_chunks(self._chunks, self._settings().chunk_size)
            self._scene = sc.to(dev)
            self._materials = mats
            self._scene_dirty = False
        return self._scene

    def _c_settings(self, seed_nonce=None):
        s = self._settings()
        PackedScene.check_chunk_size(int(s.chunk_size))
        if seed_nonce is None:
            seed_nonce = 0 if s.static else random.getrandbits(63) | 1
        return nat.VrtSettings(int(s.width), int(s.height), int(s.samples), int(s.chunk_size), int(s.chunk_radius),
                               1 if self._has_background() else 0, seed_nonce, float(s.proportions),
                               float(s.shutter), float(s.falloff), float(s.dof), float(s.dist_min),
                               float(s.dist_max), float(s.max_light), float(s.max_bounces), float(s.lod_bounces),
                               float(s.lod_samples), float(s.lod_random), float(s.lod_edge))

    def _c_camera(self):
        cam = nat.VrtCamera()
        cam.pos[:] = _xyz(self.pos)
        cam.rot[:] = [float(self.rot.x), float(self.rot.y), float(self.rot.z), float(self.rot.w)]
        cam.lens = float(self.lens)
        return cam

    def _c_scene(self, sc):
        t = sc.device_tensors
        cs = nat.VrtScene()
        cs.origin[:] = [int(v) for v in sc.origin]
        cs.dims[:] = [int(v) for v in sc.dims]
        cs.chunk_size = sc.chunk_size
        cs.n_slots = sc.n_slots
        cs.n_materials = len(sc.materials)
        selected = self._camera_table is not None and sc is self._world   # chunk_update() chose this world's chunks
        cs.d_chunk_table = (self._camera_table if selected else t["chunk_table"]).data_ptr()
        cs.d_voxels = t["voxels"].data_ptr()
        cs.d_materials = t["materials"].data_ptr()
        cs.d_occupancy = t["occupancy"].data_ptr() if t.get("occupancy") is not None else None
        cs.d_world_tables = t["world_tables"].data_ptr() if t.get("world_tables") is not None else None
        if selected:
            cs.max_resolution = int(self._camera_table_max_res)   # (as of the chunk_update() that wrote the table)
            # (vrt_select_chunks keeps every block where it is: a table-order world stays one)
            cs.flags = nat.SCENE_LAYOUT_DENSE if sc.dense else 0
        else:
            cs.max_resolution = int(getattr(sc, "max_resolution", 0))
            # (VRT_SCENE_TABLE_IS_IDENTITY: the march computes its table entries; VRT_SCENE_LAYOUT_DENSE: it looks ahead
            # across chunk borders -- include/vrt.h)
            cs.flags = sc.layout_flags()
        return cs

    def _max_selected_resolution(self, world):
        """Upper bound of the resolutions vrt_select_chunks can have written for this camera: the reference picks
        lod = min(trunc(dist(chunk centre, camera) / (dist_max / (1 + chunk_lod))), chunk_lod) (init.py:448-449), and no
        chunk of the world box is farther from the camera than its farthest corner chunk.  The kernel variant follows
        from it (resolution 1 only / <= 2 / any): with the reference's defaults (chunk_lod 2, dist_max 192) and the
        default scene no chunk reaches LOD 2, so the frame runs the resolution <= 2 kernel, not the generic one."""
        s = self._settings()
        cs_ = int(s.chunk_size)
        lod_max = int(s.chunk_lod)
        if lod_max == 0:
            return 1
        cam = _xyz(self.pos)
        far2 = 0.0
        for a in range(3):
            lo = int(world.origin[a]) + int(s.chunk_radius)                       # centre of the first / last chunk
            hi = int(world.origin[a]) + (int(world.dims[a]) - 1) * cs_ + int(s.chunk_radius)
            d = max(abs(lo - cam[a]), abs(hi - cam[a]))
            far2 += d * d
        q = math.sqrt(far2) / (float(s.dist_max) / (1 + lod_max))
        # (the kernel's distance is math.dist's, bit for bit (vrt_dist3), while far2 sums the squares naively, and the farthest
        # corner's centre may be no chunk's: the factor guards the bound against those last roundings, an ulp or two each)
        lod = min(int(math.trunc(q * (1 + 1e-12))), lod_max)
        return lod + 1

    def _velocity_bound(self, rot=None):
        """Upper bound of |vel|_inf of a ray of a camera with rotation `rot` ((x, y, z, w); default: this camera's).  After a hit the velocity is Chebyshev-normalised and a reflection
        scales a component by |1 - 2 ior| <= 1 (init.py:84, 108), but the primary direction is
        rot.multiply(lens quaternion).vec_forward() (lib.py:353-358, 372-376) and the reference's quaternion product is
        not the Hamilton product: it does not preserve the norm, so for a rotated camera the primary velocity can be
        longer than 1 (1.65 seen).  With r = M(rot) o, |o| = 1: |vx|, |vy| <= |r|^2 and |vz| <= max(1, 2 |r|^2 - 1)."""
        qx, qy, qz, qw = [float(v) for v in (rot if rot is not None else (self.rot.x, self.rot.y, self.rot.z, self.rot.w))]
        m = np.array([[qw, qz, -qy, qx], [qz, qw, qx, qy], [qy, -qx, qw, qz], [qx, -qy, -qz, qw]])
        s2 = float(np.linalg.norm(m, 2)) ** 2
        return max(1.0, s2, 2.0 * s2 - 1.0)

    def _box_radius(self, rot=None):
        """Chunk cells on either side of a camera's own that every ray stays inside: a ray moves at most dist_max (plus one
        void-skip step of at most 1 + chunk_size / 2) times _velocity_bound(rot) in the max-norm."""
        s = self._settings()
        cs = int(s.chunk_size)
        return int(math.ceil((float(s.dist_max) + 1.0 + cs / 2.0) * self._velocity_bound(rot) / cs)) + 1

    def _box_around(self, pos, r):
        """(origin, dims) of the box of `r` chunk cells on either side of the one that holds `pos` (x, y, z)."""
        cs = int(self._settings().chunk_size)
        return [(int(math.floor(v / cs)) - r) * cs for v in pos], [2 * r + 1] * 3

    def _key_box(self, origin=None, dims=None, keys=None, reset=0):
        """(vrt_traversed, keys) for the box of `dims` chunk cells whose cell (0, 0, 0) is the chunk at `origin` (world
        coordinates); without an origin: no box.  `keys`: the caller's int64 tensor, one key per cell, used as it is unless
        `reset`; None: allocated here, and the launch that clears its counters sets every key to "never visited"."""
        tr = nat.VrtTraversed()
        if origin is None:
            return tr, None
        if keys is None:
            keys = self._torch.empty((dims[0] * dims[1] * dims[2],), dtype=self._torch.int64, device=self._device)
            reset = 1
        tr.origin[:] = origin
        tr.dims[:] = dims
        tr.reset = reset
        tr.d_keys = keys.data_ptr()
        return tr, keys

    def _trav_box(self, want):
        """Box of chunk cells around the camera that every ray stays inside (_box_radius)."""
        if not want:
            return self._key_box()
        r = self._box_radius()
        if (2 * r + 1) ** 3 > (1 << 28):
            s = self._settings()
            raise nat.VrtError("the traversed-chunk box would need %d^3 cells (dist_max %r, chunk_size %d, camera "
                               "rotation %r)" % (2 * r + 1, s.dist_max, int(s.chunk_size), self.rot))
        return self._key_box(*self._box_around(_xyz(self.pos), r))

    def upload_pixels(self, pixels):
        """Validate and upload an [n, 2] (x, y) pixel list once; pass the result as `pixels=` to render()."""
        s = self._settings()
        arr = np.ascontiguousarray(np.asarray(pixels, np.int32).reshape(-1, 2))
        if len(arr) and (arr.min() < 0 or arr[:, 0].max() >= s.width or arr[:, 1].max() >= s.height):
            raise ValueError("pixel outside the %dx%d window" % (s.width, s.height))
        return DevicePixels(self._torch.from_numpy(arr).to(self._require_device()), arr)

    def _pixels_tensor(self, thread, pixels):
        if isinstance(pixels, DevicePixels):
            return pixels
        if pixels is not None:
            return self.upload_pixels(pixels)
        plist = self._settings().pixels[thread]
        dp = self._cached_pixels(self._pixel_cache.get(thread), plist)
        if dp is None:
            arr = plist.array if hasattr(plist, "array") else np.asarray(list(plist), np.int32).reshape(-1, 2)
            dp = self.upload_pixels(arr)
            self._pixel_cache[thread] = (plist, dp)
        return dp

    @staticmethod
    def _cached_pixels(entry, plist):
        """The DevicePixels of a _pixel_cache entry (the list it was uploaded from, the upload) if `plist` is that very
        list, unchanged in length; else None.  The entry holds the list itself: finalize_settings replaces
        settings.pixels, and an id() kept without the object can come back for a new list of the same length (a 64 x 16
        window resized to 16 x 64), whose frame would then be rendered from the old window's pixels."""
        if entry is None or entry[0] is not plist or len(entry[1].array) != len(plist):
            return None
        return entry[1]

    def _plan_for(self, dp, st):
        """Build (once per pixel list and sample settings) the tile plan of `dp`."""
        torch = self._torch
        L = nat.lib()
        key = (int(st.width), int(st.height), int(st.samples), float(st.lod_edge), len(dp.array))
        if dp.plan is not None and dp.plan_key == key:
            return dp
        n_px = len(dp.array)
        pb, sb = C.c_int64(0), C.c_int64(0)
        rc = L.vrt_plan_bytes(C.byref(st), n_px, C.byref(pb), C.byref(sb))
        if rc != 0:
            raise nat.VrtError("this window is too large for the GPU path: width * height * samples must stay below "
                               "2**32 (%s)" % L.vrt_status_string(rc).decode())
        plan = torch.empty(pb.value, dtype=torch.uint8, device=self._device)
        scratch = torch.empty(sb.value, dtype=torch.uint8, device=self._device)
        stream = torch.cuda.current_stream().cuda_stream
        nat.check(L.vrt_plan_build(C.byref(st), dp.tensor.data_ptr(), n_px, plan.data_ptr(), plan.numel(),
                                   scratch.data_ptr(), scratch.numel(), stream), "vrt_plan_build")
        hdr = plan[:64].cpu().numpy().view(np.uint64)
        if int(hdr[0]) != nat.PLAN_MAGIC or int(hdr[1]) != n_px:
            raise nat.VrtError("tile plan header is corrupt")
        self._retire_table(dp, dp.plan)   # (frames on other streams that read the cached tables read the old plan too)
        dp.plan, dp.plan_key, dp.n_distinct = plan, key, int(hdr[3])
        dp.full_frame = bool(hdr[6])   # the list is the whole window (in the reference's x-major order): the plan's own check
        del scratch
        return dp

    def _draw_table_for(self, dp, st, fast_draws):
        """The frame-invariant draw table of a static-seed run (reference init.py:136-139): built once per (pixel
        list, draws per seed, seed nonce) and then reused by every frame.  Only used when `cache_draws` is set."""
        torch = self._torch
        L = nat.lib()
        key = (dp.plan_key, int(fast_draws), int(st.seed_nonce))
        if dp.draw_table is not None and dp.draw_key == key:
            return dp.draw_table
        tb = C.c_int64(0)
        nat.check(L.vrt_draw_table_bytes(dp.n_distinct, fast_draws, C.byref(tb)), "vrt_draw_table_bytes")
        self._retire_table(dp, dp.draw_table)
        dp.draw_table = None
        table = torch.empty(tb.value, dtype=torch.uint8, device=self._device)
        stream = torch.cuda.current_stream().cuda_stream
        nat.check(L.vrt_draw_table_build(C.byref(st), dp.tensor.data_ptr(), len(dp.array), dp.plan.data_ptr(),
                                         dp.n_distinct, fast_draws, table.data_ptr(), table.numel(), stream),
                  "vrt_draw_table_build")
        dp.draw_table, dp.draw_key = table, key
        self._retire_table(dp, dp.ray_table)
        dp.ray_table = dp.ray_key = None
        self._table_built(dp)
        return table

    def _ray_table_for(self, dp, st, fast_draws, draw_table):
        """The frame-invariant ray table of a static-seed run (lens quaternion + life per ray slot, reference
        init.py:41-43, 56, 139): a function of the draws, the lens and the settings below, not of the camera's position
        or rotation."""
        torch = self._torch
        L = nat.lib()
        key = (dp.draw_key, float(self.lens), float(st.proportions), float(st.dof), float(st.lod_samples),
               float(st.lod_random), float(st.dist_min), float(st.dist_max))
        if dp.ray_table is not None and dp.ray_key == key:
            return dp.ray_table
        tb = C.c_int64(0)
        nat.check(L.vrt_ray_table_bytes(C.byref(st), len(dp.array), C.byref(tb)), "vrt_ray_table_bytes")
        self._retire_table(dp, dp.ray_table)
        dp.ray_table = None
        table = torch.empty(tb.value, dtype=torch.uint8, device=self._device)
        stream = torch.cuda.current_stream().cuda_stream
        nat.check(L.vrt_ray_table_build(C.byref(st), float(self.lens), dp.tensor.data_ptr(), len(dp.array),
                                        dp.plan.data_ptr(), draw_table.data_ptr(), fast_draws, table.data_ptr(),
                                        table.numel(), stream), "vrt_ray_table_build")
        dp.ray_table, dp.ray_key = table, key
        self._table_built(dp)
        return table

    def _retire_table(self, dp, old):
        """A cached table is about to be dropped while frames on other streams may still read it: tell the caching
        allocator about every stream that was ordered behind its build (they are the ones that can have read it), so
        that the block is not handed out again before those streams have passed their last use."""
        if old is None:
            return
        torch = self._torch
        for s in dp.table_streams:
            old.record_stream(torch.cuda.ExternalStream(s, device=self._device))

    def _table_built(self, dp):
        """A cached table of `dp` was just launched on the current stream: remember an event behind it.  Frames on other
        streams wait for it before they read the table (the tables outlive the frame that built them)."""
        torch = self._torch
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream())
        dp.table_events = [ev] if dp.ray_table is None else dp.table_events[-1:] + [ev]
        dp.table_streams = {int(torch.cuda.current_stream().cuda_stream)}

    def _order_after_table_builds(self, dp):
        """Make the current stream wait for the builds of dp's cached tables unless it is already ordered behind them
        (it built them, or it has waited before).  Not done while the stream is being captured into a graph: a capture
        follows warm-up frames on the capturing stream, which have waited already."""
        torch = self._torch
        cur = torch.cuda.current_stream()
        if int(cur.cuda_stream) in dp.table_streams or torch.cuda.is_current_stream_capturing():
            return
        for ev in dp.table_events:
            cur.wait_event(ev)
        dp.table_streams.add(int(cur.cuda_stream))

    def _tables_for(self, dp, st, fast_draws):
        """(draw table, ray table) of `dp` for a static-seed run, built or cached, with the current stream ordered behind
        their builds."""
        table = self._draw_table_for(dp, st, fast_draws)
        self._order_after_table_builds(dp)   # (the ray table's build reads the draw table)
        rtab = self._ray_table_for(dp, st, fast_draws, table)
        self._order_after_table_builds(dp)
        return table, rtab

    def _frame_setup(self, thread, pixels, seed_nonce=0):
        """What every frame entry point starts from: (pixel list with its plan, C settings, C scene, max samples per pixel,
        pixels).  The plan of a new pixel list is built on the stream that is current."""
        dev = self._require_device()
        sc = self._ensure_scene()
        st = self._c_settings(seed_nonce)
        with self._torch.cuda.device(dev):
            dp = self._plan_for(self._pixels_tensor(thread, pixels), st)
        return dp, st, self._c_scene(sc), nat.lib().vrt_max_samples(C.byref(st)), int(dp.array.shape[0])

    def _on_stream(self, stream):
        """Context of a call that takes `stream=`: that torch stream is current inside; None: the current one stays."""
        torch = self._torch
        return torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream())

    def _get_workspace(self, nbytes):
        """Scratch buffer of the frame being rendered: one per stream, so that frames submitted on different streams
        (two frames in flight: the second starts while the first one's last waves drain) never share it."""
        torch = self._torch
        with torch.cuda.device(self._device):
            key = int(torch.cuda.current_stream().cuda_stream)
        ws = self._workspace.get(key)
        if ws is None or ws.numel() < nbytes:
            ws = self._workspace[key] = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=self._device)
        return ws

    # ------------------------------------------------------------------ rendering
    def render(self, thread=0, pixels=None, want_image=True, want_f32=True, want_ray_rgba=False, want_rays=False,
               want_traversed=True, seed_nonce=None, check=True):
        """Run Camera.tile's pixel loop (reference init.py:126-150) on the GPU for settings.pixels[thread] (or an
        explicit [n, 2] pixel array).  Returns a RenderResult holding device tensors; nothing is copied to the
        host except the 16-word statistics block (when `check`).
        A captured graph holds the raw pointers of the plan and the cached tables it was captured with: replaying it after a
        change that rebuilds them (the lens, the window, the sample or distance settings) is not supported -- capture again."""
        torch = self._torch
        L = nat.lib()
        dp, st, csc, smax, n_px = self._frame_setup(thread, pixels, seed_nonce)
        dev = self._device
        s = self._settings()
        d_px, arr = dp.tensor, dp.array
        cam = self._c_camera()
        nb = C.c_int64(0)
        used_draws = self.fast_draws
        cached = bool(self.cache_draws and s.static and int(st.seed_nonce) == 0)
        # a non-static frame seeds every ray slot on its own (include/vrt.h, vrt_settings.seed_nonce)
        n_rows = dp.n_distinct if int(st.seed_nonce) == 0 else n_px * smax
        # cached tables are passed to vrt_render_tile and need no room in the workspace (VRT_WS_* bits)
        nat.check(L.vrt_workspace_bytes(C.byref(st), n_px, n_rows, used_draws, 3 if cached else 0, C.byref(nb)),
                  "vrt_workspace_bytes")
        _ensure_pow_memo(torch, dev, s.falloff)
        ws = self._get_workspace(nb.value)
        res = RenderResult()
        res.max_samples = smax
        res.pixels = arr
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream().cuda_stream
            if want_f32:
                res.rgba_f32 = torch.empty((n_px, 4), dtype=torch.float32, device=dev)
            if want_image:
                # pixels of other threads stay transparent (init.py:128); a thread that owns the whole window writes them all
                res.image_u8 = (torch.empty if dp.full_frame else torch.zeros)((int(s.height), int(s.width), 4), dtype=torch.uint8, device=dev)
            if want_ray_rgba:
                res.ray_rgba = torch.empty(n_px * smax, dtype=torch.int32, device=dev)
            d_rays = None
            if want_rays:
                d_rays = torch.zeros(n_px * smax * nat.RAY_BYTES, dtype=torch.uint8, device=dev)
            stats = torch.empty(nat.NSTATS, dtype=torch.int64, device=dev)   # (the library clears it)
            tr, keys = self._trav_box(want_traversed)
            table = rtab = None
            if cached:
                table, rtab = self._tables_for(dp, st, used_draws)
            rc = L.vrt_render_tile(C.byref(csc), C.byref(st), C.byref(cam), d_px.data_ptr(), n_px, dp.plan.data_ptr(),
                                   n_rows, used_draws, table.data_ptr() if table is not None else None,
                                   rtab.data_ptr() if rtab is not None else None, ws.data_ptr(), ws.numel(),
                                   res.rgba_f32.data_ptr() if want_f32 else None,
                                   res.image_u8.data_ptr() if want_image else None,
                                   res.ray_rgba.data_ptr() if want_ray_rgba else None,
                                   d_rays.data_ptr() if want_rays else None, stats.data_ptr(),
                                   C.byref(tr) if want_traversed else None, stream)
            nat.check(rc, "vrt_render_tile")
            res.traversed_keys = keys
            res.trav_origin = [int(v) for v in tr.origin]
            res.trav_dims = [int(v) for v in tr.dims]
            res._stats_dev = stats
            if check or want_rays:
                res.stats = stats.cpu().numpy()
                self.last_stats = res.stats
                retry, draws64 = _check_stats(res.stats, used_draws, "frame")
                if draws64:
                    self.fast_draws = 64
                if retry:
                    return self.render(thread, pixels=dp, want_image=want_image, want_f32=want_f32,
                                       want_ray_rgba=want_ray_rgba, want_rays=want_rays,
                                       want_traversed=want_traversed, seed_nonce=int(st.seed_nonce), check=check)
            if want_rays:
                raw = d_rays.cpu().numpy()
                res.rays = raw.view(np.dtype(nat.RAY_FIELDS, align=True))
        return res

    # ------------------------------------------------------------------ many views of one scene in one launch
    @staticmethod
    def _pose_records(poses, lens):
        """[V, 8] float64 vrt_camera records (pos, rot, lens) of `poses`: a sequence of (pos, rot) pairs, a [V, 7] array
        (x, y, z, qx, qy, qz, qw) or a [V, 8] array of vrt_camera records, whose lens column must equal `lens` -- the
        ray table was built for one lens, and the library cannot check records that are already on the device."""
        if isinstance(poses, np.ndarray):
            arr = np.asarray(poses, np.float64)
        else:
            rows = []
            for p in poses:
                pos, rot = p
                pos = _xyz(pos) if hasattr(pos, "x") else [float(v) for v in pos]
                rot = [float(rot.x), float(rot.y), float(rot.z), float(rot.w)] if hasattr(rot, "x") else [float(v) for v in rot]
                if len(pos) != 3 or len(rot) != 4:
                    raise ValueError("a pose is (pos[3], rot[4])")
                rows.append(pos + rot)
            arr = np.asarray(rows, np.float64).reshape(-1, 7)
        if arr.ndim != 2 or arr.shape[1] not in (7, 8):
            raise ValueError("poses must be a sequence of (pos, rot) or a [V, 7] array (or [V, 8] vrt_camera records)")
        if arr.shape[0] == 0:
            raise ValueError("render_views() needs at least one pose")
        rec = np.empty((arr.shape[0], 8), np.float64)
        rec[:, :7] = arr[:, :7]
        rec[:, 7] = float(lens)
        if arr.shape[1] == 8 and not np.array_equal(arr[:, 7], rec[:, 7]):
            raise ValueError("every view of a batch must have the camera's lens (%r): the ray table is built for one lens"
                             % float(lens))
        return rec

    def _check_pose_range(self, rec, s):
        """vrt_render_tile's range rule for a camera (|rot| <= 1e3, |pos| + reach < 2^28), which the library applies to
        host records only: the cameras of a batch are checked here, before they are uploaded.  (A restatement of the rule in
        fill_params, csrc/vrt_kernels.hip: keep the two alike.)"""
        if not np.all(np.isfinite(rec)) or np.abs(rec[:, 3:7]).max() > 1e3:
            raise ValueError("a pose of the batch is not finite or its rotation exceeds 1e3")
        q2 = (rec[:, 3:7] ** 2).sum(1)
        reach = (abs(float(s.dist_max)) + abs(float(s.dist_min)) + 2.0 * int(s.chunk_size) + 2.0) * (8 * q2 + 1)
        if not np.all(np.abs(rec[:, :3]).max(1) + reach < 2.0 ** 28):
            raise ValueError("a pose of the batch lies outside the range the march supports: |pos| + reach must stay below 2**28")

    def _device_poses(self, rec, who, verb):
        """The device copy of the pose records `rec`.  Their upload is a host-to-device copy, which a stream capture cannot
        hold: the last batch's device copy is kept (self._views_cams) and reused for equal poses, whichever of the batch
        calls made it (a capture follows a warm-up batch with the poses it captures)."""
        torch = self._torch
        ckey = rec.tobytes()
        if self._views_cams is None or self._views_cams[0] != ckey:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("%s() inside a stream capture needs the poses of the batch %s just before "
                                   "it (their upload cannot be captured)" % (who, verb))
            self._views_cams = (ckey, torch.from_numpy(rec).to(self._device))
        return self._views_cams[1]

    def _view_boxes(self, rec):
        """(origins, dims) of the traversed boxes of a batch: every view's box by _trav_box's rule for its pose; the velocity
        bound depends on the rotation, so all of them get the largest dimensions of the batch (the library wants equal dims
        and one allocation of keys)."""
        r = max(self._box_radius(q) for q in rec[:, 3:7])
        n, n_views = 2 * r + 1, int(rec.shape[0])
        if n ** 3 > (1 << 28) or n ** 3 * n_views >= (1 << 32):
            s = self._settings()
            raise nat.VrtError("the traversed-chunk boxes would need %d x %d^3 cells (dist_max %r, chunk_size %d)"
                               % (n_views, n, s.dist_max, int(s.chunk_size)))
        return [self._box_around(p, r)[0] for p in rec[:, :3]], [n, n, n]

    def render_views(self, poses, thread=0, pixels=None, want_image=True, want_f32=True, want_ray_rgba=False,
                     want_traversed=True, check=True):
        """Camera.render for many camera poses of one scene with one march launch per batch instead of per view (plus the
        batch's clear, set-up, two re-trace and resolve launches; vrt_render_views): what a small
        window needs, whose own launch leaves the GPU nearly empty -- stereo pairs, cube faces, a camera path, many
        agents' viewpoints.  poses: a sequence of (pos, rot) or a [V, 7] array; lens and settings are the camera's own.
        Returns one RenderResult per view, bit-identical to render() at that pose: their tensors are views into the
        batch's, each carries its own traversed box (so traversed() and chunk_update() work per view), and `stats` is the
        batch's shared block (words 0-11: the sum over the views).  Static settings and cached tables only.

        Inside a stream capture the records' upload (a host-to-device copy) cannot be captured: the device copy of the
        last batch's records is kept (self._views_cams) and reused for equal poses, so a capture must follow an eager
        batch with the same poses, and the graph replays those poses only."""
        torch = self._torch
        L = nat.lib()
        s = self._settings()
        if not s.static:
            raise ValueError("render_views() needs settings.static: a batch reuses the cached draw and ray tables, which "
                             "a non-static run re-seeds every frame")
        if not self.cache_draws:
            raise ValueError("render_views() needs cache_draws: a batch reuses the cached draw and ray tables")
        rec = self._pose_records(poses, self.lens)
        self._check_pose_range(rec, s)
        n_views = int(rec.shape[0])
        dp, st, csc, smax, n_px = self._frame_setup(thread, pixels)
        dev = self._device
        d_px, arr = dp.tensor, dp.array
        slots = n_px * smax
        if n_views * slots >= (1 << 32) - 1:
            raise nat.VrtError("the batch is too large: views * pixels * samples must stay below 2**32 (%d * %d)"
                               % (n_views, slots))
        used_draws = self.fast_draws
        nb = C.c_int64(0)
        nat.check(L.vrt_views_workspace_bytes(C.byref(st), n_views, n_px, C.byref(nb)), "vrt_views_workspace_bytes")
        _ensure_pow_memo(torch, dev, s.falloff)
        ws = self._get_workspace(nb.value)
        H, W = int(s.height), int(s.width)
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream().cuda_stream
            f32 = torch.empty((n_views, n_px, 4), dtype=torch.float32, device=dev) if want_f32 else None
            img = (torch.empty if dp.full_frame else torch.zeros)((n_views, H, W, 4), dtype=torch.uint8, device=dev) \
                if want_image else None
            rr = torch.empty((n_views, slots), dtype=torch.int32, device=dev) if want_ray_rgba else None
            stats = torch.empty(nat.NSTATS, dtype=torch.int64, device=dev)   # (the library clears it)
            cams = self._device_poses(rec, "render_views", "rendered")
            trs = keys = None
            if want_traversed:
                origins, dims = self._view_boxes(rec)
                keys = torch.empty((n_views, dims[0] * dims[1] * dims[2]), dtype=torch.int64, device=dev)
                # (the library takes an array of structs: its elements are copies of _key_box's)
                trs = (nat.VrtTraversed * n_views)(*[self._key_box(o, dims, keys[v], 1)[0] for v, o in enumerate(origins)])
            table, rtab = self._tables_for(dp, st, used_draws)
            rc = L.vrt_render_views(C.byref(csc), C.byref(st), cams.data_ptr(), n_views, d_px.data_ptr(), n_px,
                                    dp.plan.data_ptr(), dp.n_distinct, used_draws, table.data_ptr(), rtab.data_ptr(),
                                    ws.data_ptr(), ws.numel(), f32.data_ptr() if want_f32 else None,
                                    img.data_ptr() if want_image else None, rr.data_ptr() if want_ray_rgba else None,
                                    None, stats.data_ptr(), trs if want_traversed else None, stream)
            nat.check(rc, "vrt_render_views")
            hstats = None
            if check:
                hstats = stats.cpu().numpy()
                self.last_stats = hstats
                retry, draws64 = _check_stats(hstats, used_draws, "batch")
                if draws64:
                    self.fast_draws = 64
                if retry:
                    return self.render_views(rec[:, :7], thread, pixels=dp, want_image=want_image, want_f32=want_f32,
                                             want_ray_rgba=want_ray_rgba, want_traversed=want_traversed, check=check)
            out = []
            for v in range(n_views):
                res = RenderResult()
                res.max_samples = smax
                res.pixels = arr
                res.rgba_f32 = f32[v] if want_f32 else None
                res.image_u8 = img[v] if want_image else None
                res.ray_rgba = rr[v] if want_ray_rgba else None
                if want_traversed:
                    res.traversed_keys = keys[v]
                    res.trav_origin = [int(x) for x in trs[v].origin]
                    res.trav_dims = [int(x) for x in trs[v].dims]
                else:
                    res.trav_origin, res.trav_dims = [0, 0, 0], [0, 0, 0]
                res._stats_dev = stats
                res.stats = hstats
                out.append(res)
        return out

    # ------------------------------------------------------------------ first hit: what a pixel sees
    def _first_hit_tables(self, dp, st):
        """The plan and the ray table a first-hit pass reads (the lens jitter and the life of every ray are the static-seed
        frame's).  Returns (ray table, retire): with cache_draws unset the tables were built for this call and `retire()`
        drops them again once the pass has been launched."""
        rtab = self._tables_for(dp, st, self.fast_draws)[1]

        def retire():
            if self.cache_draws:
                return
            for t in (dp.draw_table, dp.ray_table):
                self._retire_table(dp, t)
            dp.draw_table = dp.draw_key = dp.ray_table = dp.ray_key = None
        return rtab, retire

    def first_hit(self, thread=0, pixels=None, all_samples=False, stream=None):
        """What every pixel of settings.pixels[thread] (or of an explicit pixel list) sees: the primary rays of render() --
        the same lens jitter, the same life -- followed to their first voxel and no further (vrt_first_hit: no shading, no
        draws, no traversed list).  Returns a HitResult of device tensors: one record per pixel (its first sample), or with
        all_samples one per ray slot p * max_samples + s, unused sample slots marked material -1.  Nothing is copied to
        the host and nothing synchronises; `stream` (a torch stream) defaults to the current one."""
        torch = self._torch
        L = nat.lib()
        dev = self._require_device()
        s = self._settings()
        self._ensure_scene()   # (a changed scene is uploaded on the caller's stream, as render() does, not on `stream`)
        with torch.cuda.device(dev), self._on_stream(stream):
            dp, st, csc, smax, n_px = self._frame_setup(thread, pixels)
            cam = self._c_camera()
            samples = smax if all_samples else 1
            rtab, retire = self._first_hit_tables(dp, st)
            records = torch.empty(max(n_px * samples, 1) * nat.HIT_BYTES, dtype=torch.uint8, device=dev)
            stats = torch.empty(nat.NSTATS, dtype=torch.int64, device=dev)   # (the library clears it)
            rc = L.vrt_first_hit(C.byref(csc), C.byref(st), C.byref(cam), dp.tensor.data_ptr(), n_px, dp.plan.data_ptr(),
                                 dp.n_distinct, rtab.data_ptr(), 0 if all_samples else 1, records.data_ptr(), stats.data_ptr(),
                                 torch.cuda.current_stream().cuda_stream)
            retire()
            nat.check(rc, "vrt_first_hit")
        return HitResult(records[: n_px * samples * nat.HIT_BYTES], dp.array, samples, smax, int(s.height), int(s.width), stats)

    def first_hit_views(self, poses, thread=0, pixels=None, all_samples=False, stream=None):
        """first_hit() for many camera poses of one scene in one launch (vrt_first_hit_views): depth or material-id images
        for stereo pairs, cube faces, a camera path, many agents.  poses: as render_views takes them; lens and settings are
        the camera's own.  Returns one HitResult per view -- views into the batch's record buffer, bit-identical to first_hit()
        at that pose; their `stats` is the batch's shared block.  Inside a stream capture the poses must be those of the
        batch made just before it (their upload cannot be captured: render_views)."""
        torch = self._torch
        L = nat.lib()
        s = self._settings()
        rec = self._pose_records(poses, self.lens)
        self._check_pose_range(rec, s)
        n_views = int(rec.shape[0])
        dev = self._require_device()
        self._ensure_scene()   # (on the caller's stream: first_hit)
        with torch.cuda.device(dev), self._on_stream(stream):
            dp, st, csc, smax, n_px = self._frame_setup(thread, pixels)
            if n_views * n_px * smax >= (1 << 32) - 1:
                raise nat.VrtError("the batch is too large: views * pixels * samples must stay below 2**32 (%d * %d)"
                                   % (n_views, n_px * smax))
            samples = smax if all_samples else 1
            cams = self._device_poses(rec, "first_hit_views", "made")
            nb = C.c_int64(0)
            nat.check(L.vrt_first_hit_views_workspace_bytes(n_views, C.byref(nb)), "vrt_first_hit_views_workspace_bytes")
            ws = self._get_workspace(nb.value)
            rtab, retire = self._first_hit_tables(dp, st)
            per_view = n_px * samples * nat.HIT_BYTES
            records = torch.empty(max(n_views * per_view, 1), dtype=torch.uint8, device=dev)
            stats = torch.empty(nat.NSTATS, dtype=torch.int64, device=dev)   # (the library clears it)
            rc = L.vrt_first_hit_views(C.byref(csc), C.byref(st), cams.data_ptr(), n_views, dp.tensor.data_ptr(), n_px,
                                       dp.plan.data_ptr(), dp.n_distinct, rtab.data_ptr(), 0 if all_samples else 1,
                                       ws.data_ptr(), ws.numel(), records.data_ptr(), stats.data_ptr(),
                                       torch.cuda.current_stream().cuda_stream)
            retire()
            nat.check(rc, "vrt_first_hit_views")
        return [HitResult(records[v * per_view:(v + 1) * per_view], dp.array, samples, smax, int(s.height), int(s.width), stats)
                for v in range(n_views)]

    # ------------------------------------------------------------------ explicit rays: the first voxel along any ray
    def _cast_records(self, origins, velocities, lives, default_life, who="cast_rays"):
        """[n, 8] float64 device tensor of vrt_cast_ray records from what cast_rays (or shade_rays: `who`) was given."""
        torch = self._torch
        dev = self._require_device()
        if velocities is None:
            # ready records, used as they are
            if not isinstance(origins, torch.Tensor) or origins.dtype != torch.float64 or not origins.is_cuda:
                raise ValueError(who + "(records): the records must be one float64 CUDA tensor [n, 8]")
            if origins.dim() != 2 or origins.shape[1] != 8 or not origins.is_contiguous() or origins.data_ptr() % 64:
                raise ValueError(who + "(records): the records must be a contiguous, 64-byte aligned [n, 8] tensor")
            if origins.device != dev:
                raise ValueError(who + "(records): the records are on %s, the camera renders on %s" % (origins.device, dev))
            if lives is not None:
                raise ValueError(who + "(records): ready records carry their own lives")
            return origins
        org = _floats(origins, "origins", who, ("n", 3), dev)
        vel = _floats(velocities, "velocities", who, ("n", 3), dev)
        n = int(org.shape[0])
        if int(vel.shape[0]) != n:
            raise ValueError(who + ": %d origins but %d velocities" % (n, int(vel.shape[0])))
        rec = torch.zeros((n, 8), dtype=torch.float64, device=dev)
        rec[:, 0:3] = org
        rec[:, 3:6] = vel
        rec[:, 6] = float(default_life) if lives is None else _floats(lives, "lives", who, (n,), dev, any_dtype=True)
        return rec

    def cast_rays(self, origins, velocities=None, lives=None, max_life=None, stream=None):
        """The first voxel along explicit rays (vrt_cast_rays): ray k starts at origins[k], advances by velocities[k] per
        unit of step and lives for lives[k] -- the reference's loop (init.py:66-116) from exactly that state up to the first
        non-empty voxel, bit for bit what the renderer's ray would do from there.  The rays go against the scene this
        camera currently renders (the packed scene of first_hit(), LODs included).  No traversed list, no bounces, no
        material filter.
        origins, velocities: [n, 3], numpy or torch; or pass ONE [n, 8] float64 CUDA tensor of ready vrt_cast_ray records
        (origin, vel, life, reserved), which is used without a copy.  lives: [n], default dist_max - dist_min.
        max_life: the bound on how long a lane may march, default settings.dist_max.
        A ray is REJECTED on the device -- material -2, every other field 0, counted in stats[9] -- when a value is not
        finite, when life > max_life, when |vel| > 2**25 on an axis, or unless
        |origin| + (max(life, 0) + 2 * chunk_size + 2) * max(1, |vel|_inf) < 2**28 on every axis.
        Returns a CastResult of device tensors; nothing is copied to the host and nothing synchronises (with tensors
        already on the device the call can be captured into a graph)."""
        torch = self._torch
        L = nat.lib()
        dev = self._require_device()
        s = self._settings()
        max_life = _max_life(max_life, s.dist_max, "cast_rays")
        sc = self._ensure_scene()
        st = self._c_settings(0)
        with torch.cuda.device(dev), self._on_stream(stream):
            rec = self._cast_records(origins, velocities, lives, float(s.dist_max) - float(s.dist_min))
            n = int(rec.shape[0])
            if n == 0:
                raise ValueError("cast_rays: no rays")
            if n >= 1 << 32:
                raise ValueError("cast_rays: 2**32 rays and more need several calls")
            csc = self._c_scene(sc)
            records = torch.empty(n * nat.HIT_BYTES, dtype=torch.uint8, device=dev)
            stats = torch.empty(nat.NSTATS, dtype=torch.int64, device=dev)   # (the library clears it)
            rc = L.vrt_cast_rays(C.byref(csc), C.byref(st), rec.data_ptr(), n, max_life, records.data_ptr(), stats.data_ptr(),
                                 torch.cuda.current_stream().cuda_stream)
            nat.check(rc, "vrt_cast_rays")
        return CastResult(records, stats)

    # ------------------------------------------------------------------ explicit rays: colour and end state along any ray
    def _shade_box(self, want):
        """The traversed box of shade_rays: False / None none; True the camera's own (_trav_box: around cam.pos, sized for
        dist_max); or (origin, dims) -- world coordinates of cell (0, 0, 0), multiples of chunk_size, and cells per axis."""
        if want is None or want is False or want is True:
            return self._trav_box(bool(want))
        origin, dims = want
        origin, dims = [int(v) for v in origin], [int(v) for v in dims]
        cs = int(self._settings().chunk_size)
        if len(origin) != 3 or len(dims) != 3 or any(o % cs for o in origin) or any(d <= 0 for d in dims):
            raise ValueError("shade_rays: want_traversed=(origin, dims) takes an origin in multiples of chunk_size and positive "
                             "dims, not %r" % (want,))
        if dims[0] * dims[1] * dims[2] > (1 << 28):
            raise ValueError("shade_rays: the traversed box %r has more than 2**28 cells" % (dims,))
        return self._key_box(origin, dims)

    def _shaded_setup(self, who, max_life, seeds, draws, n_draws):
        """What shade_rays and path_rays (`who`) check and prepare before they enter their stream: (max_life, n_draws, the
        scene, C settings).  The pow memo of the camera's falloff is made here, outside any stream capture."""
        torch = self._torch
        dev = self._require_device()
        s = self._settings()
        max_life = _max_life(max_life, s.dist_max, who)
        if seeds is not None and draws is not None:
            raise ValueError(who + ": pass seeds or draws, not both")
        if seeds is not None:
            n_draws = 32 if n_draws is None else int(n_draws)
            if not 2 <= n_draws <= 4096:
                raise ValueError(who + ": n_draws must lie in 2..4096, not %r" % n_draws)
        sc = self._ensure_scene()
        st = self._c_settings(0)
        if not torch.cuda.is_current_stream_capturing():
            _ensure_pow_memo(torch, dev, s.falloff)
        return max_life, n_draws, sc, st

    def _shaded_inputs(self, who, origins, velocities, lives, seeds, draws, n_draws):
        """The device inputs of shade_rays and path_rays (`who`), made on the current stream: (vrt_cast_ray records [n, 8], n,
        draws [n, n_draws] or None, n_draws, the stream's handle).  seeds: the rows are made on the device (vrt_rng_draws)."""
        torch = self._torch
        dev = self._device
        s = self._settings()
        rec = self._cast_records(origins, velocities, lives, float(s.dist_max) - float(s.dist_min), who)
        n = int(rec.shape[0])
        if n == 0:
            raise ValueError(who + ": no rays")
        if n >= (1 << 32) - 1:
            raise ValueError(who + ": 2**32 - 1 rays and more need several calls")
        cur = torch.cuda.current_stream().cuda_stream
        if seeds is not None:
            sd = _seeds(seeds, n, who, dev)
            dd = torch.empty((n, n_draws), dtype=torch.float64, device=dev)
            nat.check(nat.lib().vrt_rng_draws(sd.data_ptr(), n, n_draws, dd.data_ptr(), cur), "vrt_rng_draws")
        elif draws is not None:
            dd = _floats(draws, "draws", who, (n, "n_draws" if n_draws is None else int(n_draws)), dev).contiguous()
            n_draws = int(dd.shape[1])
        else:
            dd, n_draws = None, 0
        return rec, n, dd, n_draws, cur

    def shade_rays(self, origins, velocities=None, lives=None, *, seeds=None, draws=None, n_draws=None, max_life=None,
                   want_records=True, want_traversed=False, stream=None):
        """Colour and end state along explicit rays (vrt_shade_rays): ray k starts at origins[k] with velocity velocities[k]
        and life lives[k] -- the state of init.py:50-59 -- and runs the whole of Camera.trace's loop from there (hits,
        lib.material, reflection, lib.material_background if the camera has a background, the alpha): bit for bit what the
        renderer's ray gives from that state.  The rays go against the scene this camera currently renders; the camera's own
        pose, lens, dist_min / dist_max, dof and lod settings play no part.
        origins, velocities, lives, max_life: as cast_rays takes them (numpy or torch, or ONE ready [n, 8] float64 CUDA
        tensor), with the same rejection rule.
        seeds: [n] integers in [0, 2**63): ray k's draws are random.seed(seeds[k]) followed by random.random() repeatedly,
        n_draws of them (default 32, 2..4096), made on the device (vrt_rng_draws).  numpy seeds are range-checked; a torch
        tensor is taken as it is (checking it would synchronise): a negative value there is read as its unsigned 64-bit
        pattern.  draws: [n, n_draws] float64, used as
        given.  Neither: no draws -- a ray that meets a rough material runs out at once.  A ray that needs more draws than it
        has is not completed: rgba 0, record s = -3 (exhausted_mask()), counted in stats[10].
        want_traversed: True for the camera's own box (around cam.pos, sized for dist_max), or (origin, dims) for a box of
        the caller's -- origin: world coordinates of cell (0, 0, 0), multiples of chunk_size; dims: cells per axis, at most
        2**28 in all; visits outside it are counted in stats[11] -- a map view or a mirror
        sees chunks the camera's rays do not, and with culling on the next chunk_update() would drop them.
        Returns a ShadeResult of device tensors; nothing is copied to the host and nothing synchronises (with tensors already
        on the device the call can be captured into a graph)."""
        torch = self._torch
        L = nat.lib()
        dev = self._require_device()
        max_life, n_draws, sc, st = self._shaded_setup("shade_rays", max_life, seeds, draws, n_draws)
        with torch.cuda.device(dev), self._on_stream(stream):
            rec, n, dd, n_draws, cur = self._shaded_inputs("shade_rays", origins, velocities, lives, seeds, draws, n_draws)
            csc = self._c_scene(sc)
            tr, keys = self._shade_box(want_traversed)
            rgba = torch.empty(n, dtype=torch.uint32, device=dev)
            records = torch.empty(n * nat.RAY_BYTES, dtype=torch.uint8, device=dev) if want_records else None
            stats = torch.empty(nat.NSTATS, dtype=torch.int64, device=dev)   # (the library clears it)
            nb = C.c_int64(0)
            nat.check(L.vrt_shade_workspace_bytes(n, C.byref(nb)), "vrt_shade_workspace_bytes")
            # (a workspace of the call's own, kept by the result: it holds the launch-wide ray counter, and a captured call
            # keeps its pointer -- the camera's per-stream workspace is replaced when a later frame needs a larger one)
            ws = torch.empty(nb.value, dtype=torch.uint8, device=dev)
            rc = L.vrt_shade_rays(C.byref(csc), C.byref(st), rec.data_ptr(), n, max_life,
                                  dd.data_ptr() if n_draws else None, n_draws, ws.data_ptr(), ws.numel(), rgba.data_ptr(),
                                  records.data_ptr() if want_records else None, stats.data_ptr(),
                                  C.byref(tr) if keys is not None else None, cur)
            nat.check(rc, "vrt_shade_rays")
        trav = (keys, [int(v) for v in tr.origin], [int(v) for v in tr.dims]) if keys is not None else None
        res = ShadeResult(rgba, records, stats, trav)
        res._workspace = ws
        return res

    # ------------------------------------------------------------------ explicit rays: every voxel a ray shades
    def path_rays(self, origins, velocities=None, lives=None, *, seeds=None, draws=None, n_draws=None, max_hits=8, max_life=None,
                  want_rgba=True, stream=None):
        """Every voxel explicit rays shade, not only the first (vrt_path_rays): shade_rays's rays, loop, draws and rejection
        rule, with the ray's state -- step, pos, cell, material -- recorded in front of every lib.material: what stands behind
        a pane of glass, what a mirror shows, the returns of a range sensor, the voxels that lit a probe.
        origins, velocities, lives, seeds, draws, n_draws, max_life: as shade_rays takes them.
        max_hits: records kept per ray, 1..64 (and n * max_hits < 2**31); `counts` holds all hits of a ray and may exceed it.
        A rejected ray has count -2, one whose draws ran out count -3; both have every slot unused and rgba 0.
        Returns a PathResult of device tensors, whose `records` DeviceWorld.owners takes as they are; rgba and stats[0..10]
        are bit for bit shade_rays's.  Nothing is copied to the host and nothing synchronises (with tensors already on the
        device the call can be captured into a graph)."""
        torch = self._torch
        L = nat.lib()
        dev = self._require_device()
        max_hits = int(max_hits)
        if not 1 <= max_hits <= nat.PATH_MAX_HITS:
            raise ValueError("path_rays: max_hits must lie in 1..%d, not %r" % (nat.PATH_MAX_HITS, max_hits))
        max_life, n_draws, sc, st = self._shaded_setup("path_rays", max_life, seeds, draws, n_draws)
        with torch.cuda.device(dev), self._on_stream(stream):
            rec, n, dd, n_draws, cur = self._shaded_inputs("path_rays", origins, velocities, lives, seeds, draws, n_draws)
            if n * max_hits >= 1 << 31:
                raise ValueError("path_rays: %d rays of %d records each: n * max_hits must stay below 2**31" % (n, max_hits))
            csc = self._c_scene(sc)
            records = torch.empty(n * max_hits * nat.HIT_BYTES, dtype=torch.uint8, device=dev)
            counts = torch.empty(n, dtype=torch.int32, device=dev)
            rgba = torch.empty(n, dtype=torch.uint32, device=dev) if want_rgba else None
            stats = torch.empty(nat.NSTATS, dtype=torch.int64, device=dev)   # (the library clears it)
            nb = C.c_int64(0)
            nat.check(L.vrt_path_workspace_bytes(n, C.byref(nb)), "vrt_path_workspace_bytes")
            ws = torch.empty(nb.value, dtype=torch.uint8, device=dev)   # (the call's own, kept by the result: shade_rays)
            rc = L.vrt_path_rays(C.byref(csc), C.byref(st), rec.data_ptr(), n, max_life, dd.data_ptr() if n_draws else None,
                                 n_draws, max_hits, ws.data_ptr(), ws.numel(), records.data_ptr(), counts.data_ptr(),
                                 rgba.data_ptr() if want_rgba else None, stats.data_ptr(), cur)
            nat.check(rc, "vrt_path_rays")
        res = PathResult(records, counts, rgba, stats, max_hits)
        res._workspace = ws
        return res

    def pixel_rays(self, thread=0, pixels=None, all_samples=False, stream=None):
        """The primary rays of render() as explicit rays (vrt_pixel_rays): (rays, used) -- rays a [n, 8] float64 CUDA tensor of
        vrt_cast_ray records that cast_rays, shade_rays and path_rays take as they are, one per pixel of settings.pixels[thread]
        (or of an explicit pixel list; its first sample), or with all_samples one per ray slot p * max_samples + s; used a
        bool [n] tensor, false for an unused sample slot, whose record is eight NaNs (rejected by every explicit-ray call).
        Record k is the start state first_hit() and render() give that ray -- the same lens jitter, the same life, bit for
        bit.  Nothing is copied to the host and nothing synchronises; `stream` defaults to the current one."""
        torch = self._torch
        L = nat.lib()
        dev = self._require_device()
        self._ensure_scene()   # (on the caller's stream: first_hit)
        with torch.cuda.device(dev), self._on_stream(stream):
            dp, st, csc, smax, n_px = self._frame_setup(thread, pixels)
            cam = self._c_camera()
            samples = smax if all_samples else 1
            rtab, retire = self._first_hit_tables(dp, st)
            rays = torch.empty((max(n_px * samples, 1), 8), dtype=torch.float64, device=dev)[: n_px * samples]
            stats = torch.empty(nat.NSTATS, dtype=torch.int64, device=dev)   # (the library clears it)
            rc = L.vrt_pixel_rays(C.byref(csc), C.byref(st), C.byref(cam), dp.tensor.data_ptr(), n_px, dp.plan.data_ptr(),
                                  dp.n_distinct, rtab.data_ptr(), 0 if all_samples else 1, rays.data_ptr(), stats.data_ptr(),
                                  torch.cuda.current_stream().cuda_stream)
            retire()
            nat.check(rc, "vrt_pixel_rays")
            used = rays[:, 6] == rays[:, 6]   # (an unused slot is NaN throughout)
        return rays, used

    # ------------------------------------------------------------------ hit records: how the surface lies there
    def surfaces(self, hits, rays, stream=None):
        """How the surface lies at hit records (vrt_hit_surfaces): per record the ray's velocity after the reference's
        reflection (init.py:84, 92-111), its position one step on, the neighbours that reflection asked and found, and a
        geometric normal -- where a mirror, portal or deferred-reflection pass goes on from a hit, and the normal image of a
        G-buffer.  For a material of roughness 0 velocity and position are bit for bit the renderer's ray one step after the
        hit; for a rough one they are the answer for the unjittered velocity.
        hits: a HitResult (first_hit), a CastResult (cast_rays), PathResult.hit(0), or a uint8 tensor of 48-byte vrt_hit
        records on this camera's device.  rays: the rays that reached them -- what pixel_rays returned (the tensor, or the
        (rays, used) pair) or what cast_rays was given: ONE [n, 8] float64 CUDA tensor of vrt_cast_ray records, or a tuple
        (origins, velocities); only the velocities are read.
        The records go against the scene this camera currently renders, with the LODs of its last chunk_update(), as
        DeviceWorld.owners(hits, camera) resolves them.
        Returns a SurfaceResult of device tensors; nothing is copied to the host and nothing synchronises (with tensors
        already on the device the call can be captured into a graph)."""
        torch = self._torch
        dev = self._require_device()
        records = getattr(hits, "records", hits)
        if not isinstance(records, torch.Tensor) or records.dtype != torch.uint8:
            raise ValueError("surfaces(): hits must be a HitResult, a CastResult or a uint8 tensor of vrt_hit records")
        if records.device != dev:
            raise ValueError("surfaces(): the hit records are on %s, the camera renders on %s" % (records.device, dev))
        if records.numel() % nat.HIT_BYTES:
            raise ValueError("surfaces(): %d bytes are no whole number of %d-byte vrt_hit records" % (records.numel(), nat.HIT_BYTES))
        n = records.numel() // nat.HIT_BYTES
        if n >= 1 << 32:
            raise ValueError("surfaces: 2**32 records and more need several calls")
        if isinstance(rays, tuple) and len(rays) == 2 and isinstance(rays[1], torch.Tensor) and rays[1].dtype == torch.bool:
            rays = rays[0]   # (pixel_rays's (rays, used))
        if isinstance(rays, tuple) and len(rays) != 2:
            raise ValueError("surfaces(): rays must be one [n, 8] tensor of vrt_cast_ray records or (origins, velocities)")
        n_rays = len(rays[0]) if isinstance(rays, tuple) else (int(rays.shape[0]) if hasattr(rays, "shape") and len(rays.shape) else -1)
        if n_rays != n:   # (before anything is launched)
            raise ValueError("surfaces(): %d hit records but %d rays" % (n, n_rays))
        sc = self._ensure_scene()
        with torch.cuda.device(dev), self._on_stream(stream):
            origins, velocities = rays if isinstance(rays, tuple) else (rays, None)
            rec = self._cast_records(origins, velocities, None, 0.0, "surfaces")
            if not records.is_contiguous():   # (PathResult.hit(0) of rows longer than one record)
                records = records.contiguous()
            records = records.reshape(-1)
            if records.data_ptr() % 8:
                raise ValueError("surfaces(): the hit records must be 8-byte aligned")
            csc = self._c_scene(sc)
            out = torch.empty(max(n, 1) * nat.SURFACE_BYTES, dtype=torch.uint8, device=dev)
            stats = torch.empty(nat.NSTATS, dtype=torch.int64, device=dev)   # (the library clears it)
            rc = nat.lib().vrt_hit_surfaces(C.byref(csc), records.data_ptr() if n else None, rec.data_ptr() if n else None, n,
                                            out.data_ptr(), stats.data_ptr(), torch.cuda.current_stream().cuda_stream)
            nat.check(rc, "vrt_hit_surfaces")
        return SurfaceResult(out[: n * nat.SURFACE_BYTES], stats)

    def line_of_sight(self, a, b, stream=None):
        """torch.bool [n]: can point a[k] see point b[k]?  One cast per pair: vel = (b - a) / max|b - a| -- the reference's
        Chebyshev normalize (lib.py:310-314), left as it is where the maximum is 0 or 1 -- and life = max|b - a|; true
        where that ray found no voxel.  This is the renderer's own sampling: unit steps along the dominant axis, one voxel
        looked up per step (larger steps through coarser and empty chunks), so a thin diagonal gap is open or closed
        exactly as it is in the image, and a voxel at b itself (a step the life no longer covers) does not block.
        Raises ValueError when the cast rejected a pair (see cast_rays); that check synchronises."""
        torch = self._torch
        dev = self._require_device()
        with torch.cuda.device(dev), self._on_stream(stream):
            pa, pb = (_floats(v, name, "line_of_sight", ("n", 3), dev) for name, v in (("a", a), ("b", b)))
            if pa.shape != pb.shape:
                raise ValueError("line_of_sight: %d points a but %d points b" % (int(pa.shape[0]), int(pb.shape[0])))
            if int(pa.shape[0]) == 0:
                raise ValueError("line_of_sight: no pairs")
            d = pb - pa
            ref = d.abs().amax(dim=1)
            keep = (ref == 0) | (ref == 1)            # lib.py:312: `if ref and ref != 1`
            vel = torch.where(keep[:, None], d, d / torch.where(keep, torch.ones_like(ref), ref)[:, None])
            rec = torch.zeros((int(pa.shape[0]), 8), dtype=torch.float64, device=dev)
            rec[:, 0:3] = pa
            rec[:, 3:6] = vel
            rec[:, 6] = ref
            # (the bound on a lane's march follows the longest pair, not dist_max; a pair that is not finite is rejected below)
            bound = float(torch.where(torch.isfinite(ref), ref, torch.zeros_like(ref)).max())
            res = self.cast_rays(rec, max_life=min(max(bound, 1.0), float(1 << 28)), stream=stream)
            bad = res.rejected_mask()
            if bool(bad.any()):
                raise ValueError("line_of_sight: %d of %d pairs were rejected (not finite, or out of the range "
                                 "|a| + (max|b - a| + 2 * chunk_size + 2) < 2**28)" % (int(bad.sum()), int(bad.numel())))
        return res.material == 0

    def pick(self, x, y, world):
        """The voxel under the cursor: what pixel (x, y) sees, as something to act on.  Runs first_hit() on that one pixel
        (its first sample) and world.owners() on the record; `world` is the DeviceWorld whose scene this camera renders.
        Returns None where the pixel sees nothing, else (Object, local, voxel, depth): the Object instance of world.order,
        the index (x, y, z) into its sprite's model array -- the voxel a sprite edit would change --, the world voxel, and
        the ray's step at the hit.  Copies the two records to the host, so it SYNCHRONISES; for many pixels use first_hit()
        and owners() themselves.  Raises RuntimeError if no object of `world` accounts for the hit (another world's)."""
        hit = self.first_hit(pixels=[[int(x), int(y)]])
        own = world.owners(hit, self).numpy()[0]
        if int(own["object"]) == nat.OWNER_NONE:
            return None
        if int(own["object"]) < 0:
            raise RuntimeError("pick(%d, %d): no object of this world accounts for the voxel the pixel sees" % (x, y))
        return (world.order[int(own["object"])], tuple(int(v) for v in own["local"]), tuple(int(v) for v in own["voxel"]),
                float(hit.numpy()["step"][0]))

    def tile(self, thread, t=0):
        """Reference signature and return triple (init.py:126-150): RGBA8 bytes of the full window (pixels of other
        threads transparent), the traversed chunk list, and the thread index."""
        r = self.render(thread, want_image=True, want_f32=False, want_traversed=True)
        image = r.image_u8.cpu().numpy().tobytes()
        return image, r.traversed(int(self._settings().chunk_size)), thread

    def tile_f32(self, thread=0):
        """[H, W, 4] float32 image of per-pixel sample means (non-owned pixels 0) on the device."""
        torch = self._torch
        s = self._settings()
        r = self.render(thread, want_image=False, want_f32=True, want_traversed=False)
        img = torch.zeros((int(s.height), int(s.width), 4), dtype=torch.float32, device=self._device)
        px = torch.from_numpy(r.pixels.astype(np.int64)).to(self._device)
        img[px[:, 1], px[:, 0]] = r.rgba_f32
        return img

    # ------------------------------------------------------------------ single ray (reference init.py:37-121)
    def trace(self, dir_x, dir_y, detail):
        """Trace one ray and return its end state as a `store` like the reference.  The ray consumes draws from
        Python's global `random` stream exactly as the reference's trace would (the stream is advanced by the
        number of draws the ray used)."""
        rays = self.trace_many([dir_x], [dir_y], [detail], rng=random)
        return rays[0]

    def trace_many(self, dir_x, dir_y, detail, draws=None, rng=None, _n_rng_draws=113):
        """Explicit rays.  draws: [n, n_draws] array of the random.random() values each ray may consume, or `rng`
        (a random-like module/object) to draw them from for a single ray."""
        torch = self._torch
        L = nat.lib()
        dev = self._require_device()
        sc = self._ensure_scene()
        _ensure_pow_memo(torch, dev, self._settings().falloff)
        n = len(dir_x)
        state = None
        if draws is None:
            if rng is None or n != 1:
                raise ValueError("pass `draws` for more than one ray")
            state = rng.getstate()
            draws = np.array([[rng.random() for _ in range(_n_rng_draws)]], np.float64)
        draws = np.ascontiguousarray(np.asarray(draws, np.float64).reshape(n, -1))
        st = self._c_settings(0)
        cam = self._c_camera()
        csc = self._c_scene(sc)
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream().cuda_stream
            dx = torch.tensor(np.asarray(dir_x, np.float64), device=dev)
            dy = torch.tensor(np.asarray(dir_y, np.float64), device=dev)
            dt = torch.tensor(np.asarray(detail, np.float64), device=dev)
            dd = torch.from_numpy(draws).to(dev)
            d_rays = torch.zeros(n * nat.RAY_BYTES, dtype=torch.uint8, device=dev)
            stats = torch.zeros(nat.NSTATS, dtype=torch.int64, device=dev)
            tr, keys = self._trav_box(n == 1)
            nb = C.c_int64(0)
            nat.check(L.vrt_trace_workspace_bytes(n, C.byref(nb)), "vrt_trace_workspace_bytes")
            ws = self._get_workspace(nb.value)
            rc = L.vrt_trace_rays(C.byref(csc), C.byref(st), C.byref(cam), dx.data_ptr(), dy.data_ptr(),
                                  dt.data_ptr(), dd.data_ptr(), draws.shape[1], n, ws.data_ptr(), ws.numel(),
                                  d_rays.data_ptr(), stats.data_ptr(), C.byref(tr) if n == 1 else None, stream)
            nat.check(rc, "vrt_trace_rays")
            hstats = stats.cpu().numpy()
            rec = d_rays.cpu().numpy().view(np.dtype(nat.RAY_FIELDS, align=True))
        if hstats[nat.S_RNG_EXHAUSTED]:
            if state is not None and _n_rng_draws < 4096:  # a ray with very many rough hits: offer it more of the stream
                rng.setstate(state)
                return self.trace_many(dir_x, dir_y, detail, rng=rng, _n_rng_draws=4096)
            raise nat.VrtError("ray consumed more random draws than were supplied (%d)" % draws.shape[1])
        if state is not None:
            rng.setstate(state)
            for _ in range(int(rec["counters"][0][5])):
                rng.random()
        out = []
        for i in range(n):
            r = rec[i]
            ray = store(color=rgb(int(r["color"][0]), int(r["color"][1]), int(r["color"][2])),
                        energy=float(r["energy"]), pos=vec3(*[float(v) for v in r["pos"]]),
                        vel=vec3(*[float(v) for v in r["vel"]]), step=float(r["step"]), life=float(r["life"]),
                        bounces=float(r["bounces"]), traversed=[])
            if n == 1:
                ray.traversed = _traversed_positions(keys, list(tr.origin), list(tr.dims), int(self._settings().chunk_size))
            out.append(ray)
        self.last_trace_records = rec
        return out
