"""What the Camera's calls return: device tensors (torch) plus a 16-word statistics block that reaches the host on request."""
import numpy as np

from . import _native as nat


def _traversed_positions(keys, origin, dims, chunk_size):
    """Visited chunk positions of a traversed box (include/vrt.h, vrt_traversed: `keys` one int64 per chunk cell, -1 never
    visited; cell (0, 0, 0) is the chunk at `origin`) in the reference's order, which is the order of the keys: the
    order-preserving union over rays in call order (reference init.py:72-73, 143; lib.py:404-409).  [] without keys."""
    import torch
    if keys is None:
        return []
    idx = torch.nonzero(keys != -1).flatten()
    if idx.numel() == 0:
        return []
    idx = idx[torch.argsort(keys[idx])].cpu().numpy()
    cz = idx % dims[2]
    cy = (idx // dims[2]) % dims[1]
    cx = idx // (dims[2] * dims[1])
    return [(float(origin[0] + a * chunk_size), float(origin[1] + b * chunk_size), float(origin[2] + c * chunk_size))
            for a, b, c in zip(cx.tolist(), cy.tolist(), cz.tolist())]


class RenderResult:
    """Device-side outputs of one tile render (torch tensors) plus host statistics."""

    def __init__(self):
        self.rgba_f32 = None     # [n_px, 4] float32: per-pixel mean of [r, g, b, alpha] (before Surface.set_at)
        self.image_u8 = None     # [H, W, 4] uint8 full-window RGBA, non-owned pixels 0
        self.ray_rgba = None     # [n_px * max_samples] int32 packed per-sample r|g<<8|b<<16|a<<24
        self.rays = None         # numpy structured array of per-ray end states (only if requested)
        self.stats = None        # numpy int64[16]
        self.traversed_keys = None
        self.trav_origin = None
        self.trav_dims = None
        self.max_samples = 1
        self.pixels = None

    def counters(self):
        return {k: int(self.stats[i]) for i, k in enumerate(nat.COUNTER_NAMES)}

    def traversed(self, chunk_size):
        """Visited chunk positions in the reference's order (order-preserving union over rays in call order,
        reference init.py:72-73, 143; lib.py:404-409)."""
        return _traversed_positions(self.traversed_keys, self.trav_origin, self.trav_dims, chunk_size)


class _LazyStats:
    """`stats` of a call that does not synchronise: the device block `_stats_dev` (numpy int64[16] once read), copied to the
    host on first use -- a synchronisation -- and kept.  What the words count is in each class's own docstring."""
    _stats = None

    @property
    def stats(self):
        if self._stats is None:
            self._stats = self._stats_dev.cpu().numpy()
        return self._stats


class _HitRecords(_LazyStats):
    """`step`, `pos`, `cell` and `material`: views of one buffer of 48-byte vrt_hit records (include/vrt.h)."""

    def __init__(self, records, stats_dev):
        import torch
        n = records.numel() // nat.HIT_BYTES
        f64 = records.view(torch.float64).view(n, nat.HIT_BYTES // 8)
        i32 = records.view(torch.int32).view(n, nat.HIT_BYTES // 4)
        self.records = records           # uint8 [n * 48]
        self.step = f64[:, 0]            # float64 [n]: ray.step at the first voxel, or >= the ray's life for a miss
        self.pos = f64[:, 1:4]           # float64 [n, 3]: ray.pos at that moment
        self.cell = i32[:, 8:11]         # int32 [n, 3]: floor(pos)
        self.material = i32[:, 11]       # int32 [n]: 1..255 the material found, 0 none; < 0: see the class
        self._stats_dev = stats_dev

    def numpy(self):
        """The records as a numpy structured array (fields step, pos, cell, material)."""
        return np.ascontiguousarray(self.records.cpu().numpy()).view(np.dtype(nat.HIT_FIELDS)).reshape(-1)


class HitResult(_HitRecords):
    """Device-side records of a first-hit pass (Camera.first_hit / first_hit_views): what every primary ray of the frame sees.
    `step`, `pos`, `cell` and `material` are views of one buffer of 48-byte vrt_hit records (include/vrt.h), one per ray
    slot p * max_samples + s (`samples` == max_samples) or one per pixel (`samples` == 1: every pixel's first sample);
    material -1 marks an unused sample slot.
    `stats`: numpy int64[16], copied from the device on first use (a synchronisation): word 8 = rays traced, word 4 = rays
    that found a voxel.  A batch's views share one block: the batch's totals."""

    def __init__(self, records, pixels, samples, max_samples, height, width, stats_dev):
        super().__init__(records, stats_dev)
        self.pixels = pixels             # numpy [n_px, 2] (x, y)
        self.samples = samples
        self.max_samples = max_samples
        self.height, self.width = height, width

    def _scatter(self, values, fill, dtype):
        import torch
        img = torch.full((self.height, self.width), fill, dtype=dtype, device=self.records.device)
        px = torch.from_numpy(self.pixels.astype(np.int64)).to(self.records.device)
        img[px[:, 1], px[:, 0]] = values[:: self.samples]
        return img

    def depth_image(self):
        """[height, width] float64: sample 0's step where it found a voxel, inf where it found none and at pixels that
        are not listed."""
        import torch
        inf = torch.full_like(self.step, float("inf"))
        return self._scatter(torch.where(self.material > 0, self.step, inf), float("inf"), torch.float64)

    def material_image(self):
        """[height, width] int32: the material id sample 0 found (0: none); -1 at pixels that are not listed."""
        import torch
        return self._scatter(self.material, -1, torch.int32)


class CastResult(_HitRecords):
    """Device-side records of Camera.cast_rays: what every explicit ray found.  `step`, `pos`, `cell` and `material` are
    views of one buffer of 48-byte vrt_hit records (include/vrt.h), record k for ray k; material -2: the ray was rejected.
    `stats`: numpy int64[16], copied from the device on first use (a synchronisation): word 8 = rays marched, word 4 = rays
    that found a voxel, word 9 = rays rejected."""

    def hit_mask(self):
        """torch.bool [n]: the ray found a voxel within its life."""
        return self.material > 0

    def rejected_mask(self):
        """torch.bool [n]: the ray was rejected on the device (not finite, life > max_life, |vel| > 2**25, or out of
        range: include/vrt.h, vrt_cast_ray) and was not marched."""
        return self.material == nat.HIT_REJECTED


class PathResult(_LazyStats):
    """Device-side outputs of Camera.path_rays: every voxel each explicit ray shaded.  `records` is one flat uint8 buffer of
    n * max_hits 48-byte vrt_hit records (include/vrt.h), row k the hits of ray k in the order it met them, unused slots
    marked material -1 with every other field 0 -- DeviceWorld.owners takes the buffer as it is and answers OWNER_NONE for
    those.  `counts` (int32 [n]) holds ALL hits of a ray, which may exceed max_hits (the row then holds the first max_hits);
    -2 a rejected ray, -3 one whose draws ran out.  `rgba` (uint32 [n], or None) is packed r | g << 8 | b << 16 | alpha << 24.
    `stats`: numpy int64[16], copied from the device on first use (a synchronisation): words 0..10 as ShadeResult's, 12
    completed rays with more hits than max_hits, 13 hit records written for completed rays."""

    def __init__(self, records, counts, rgba, stats_dev, max_hits):
        self.records = records           # uint8 [n * max_hits * 48]
        self.counts = counts             # int32 [n]
        self.rgba = rgba                 # uint32 [n], or None
        self.max_hits = int(max_hits)
        self._stats_dev = stats_dev

    def numpy(self):
        """The records as a numpy structured array [n, max_hits] (fields step, pos, cell, material)."""
        return self.records.cpu().numpy().view(np.dtype(nat.HIT_FIELDS)).reshape(-1, self.max_hits)

    def truncated_mask(self):
        """torch.bool [n]: the ray was completed and shaded more voxels than its row holds."""
        return self.counts > self.max_hits

    def rejected_mask(self):
        """torch.bool [n]: the ray was rejected on the device (cast_rays's rule) and was not marched."""
        return self.counts == nat.PATH_REJECTED

    def exhausted_mask(self):
        """torch.bool [n]: the ray needed more draws than it was given and was not completed: repeat it with a longer row."""
        return self.counts == nat.PATH_EXHAUSTED

    def hit(self, j):
        """A CastResult view (no copy) of every ray's j-th record: `material` > 0 where the ray shaded at least j + 1 voxels,
        -1 where it did not (a rejected ray's material is -1 here too, not -2: see rejected_mask())."""
        import torch
        j = int(j)
        if not 0 <= j < self.max_hits:
            raise IndexError("hit(%d): the rows hold %d records" % (j, self.max_hits))
        n = self.records.numel() // (nat.HIT_BYTES * self.max_hits)
        f64 = self.records.view(torch.float64).view(n, self.max_hits, nat.HIT_BYTES // 8)[:, j]
        i32 = self.records.view(torch.int32).view(n, self.max_hits, nat.HIT_BYTES // 4)[:, j]
        out = CastResult.__new__(CastResult)
        out.records = self.records.view(n, self.max_hits * nat.HIT_BYTES)[:, j * nat.HIT_BYTES:(j + 1) * nat.HIT_BYTES]
        out.step, out.pos, out.cell, out.material = f64[:, 0], f64[:, 1:4], i32[:, 8:11], i32[:, 11]
        out._stats_dev = self._stats_dev
        return out


class ShadeResult(_LazyStats):
    """Device-side outputs of Camera.shade_rays: what colour and energy arrived along every explicit ray.  `rgba` is packed
    r | g << 8 | b << 16 | alpha << 24, entry k for ray k; `records` (or None) one buffer of 152-byte vrt_ray records
    (include/vrt.h), whose `s` field is 0 for a completed ray, -2 for a rejected one and -3 for one whose draws ran out.
    `stats`: numpy int64[16], copied from the device on first use (a synchronisation): words 0..7 event sums over completed
    rays, 8 completed rays, 9 rejected, 10 rays whose draws ran out, 11 chunk visits outside the traversed box."""

    def __init__(self, rgba, records, stats_dev, trav=None):
        self.rgba = rgba                 # uint32 [n]
        self.records = records           # uint8 [n * 152], or None
        self._stats_dev = stats_dev
        self.traversed_keys, self.trav_origin, self.trav_dims = trav if trav is not None else (None, None, None)

    def _s(self, what):
        import torch
        if self.records is None:
            raise ValueError("%s needs the records (shade_rays(..., want_records=True))" % what)
        n = self.records.numel() // nat.RAY_BYTES
        return self.records.view(torch.int32).view(n, nat.RAY_BYTES // 4)[:, 2]

    def numpy(self):
        """The records as a numpy structured array of vrt_ray (fields x, y, s, color, alpha, ntrav, counters, detail,
        energy, step, life, bounces, pos, vel)."""
        if self.records is None:
            raise ValueError("numpy() needs the records (shade_rays(..., want_records=True))")
        return self.records.cpu().numpy().view(np.dtype(nat.RAY_FIELDS, align=True))

    def rejected_mask(self):
        """torch.bool [n]: the ray was rejected on the device (cast_rays's rule) and was not marched."""
        return self._s("rejected_mask()") == nat.RAY_REJECTED

    def exhausted_mask(self):
        """torch.bool [n]: the ray needed more draws than it was given and was not completed: repeat it with a longer row."""
        return self._s("exhausted_mask()") == nat.RAY_EXHAUSTED

    def image(self, height, width):
        """[height, width, 4] uint8 RGBA from n == height * width rays in row-major order (ray y * width + x is pixel (x, y))."""
        import torch
        height, width = int(height), int(width)
        if height <= 0 or width <= 0 or height * width != int(self.rgba.numel()):
            raise ValueError("image(%d, %d): %d rays are not %d x %d pixels" % (height, width, int(self.rgba.numel()), height, width))
        return self.rgba.view(torch.uint8).view(height, width, 4)

    def traversed(self, chunk_size):
        """Visited chunk positions inside the box the call was given, in the reference's order (the order-preserving union
        over the rays in array order); [] without a box."""
        return _traversed_positions(self.traversed_keys, self.trav_origin, self.trav_dims, chunk_size)


class SurfaceResult(_LazyStats):
    """Device-side records of Camera.surfaces(): views of one buffer of 64-byte vrt_surface records (include/vrt.h), record k
    for hit record k -- how the surface lies there.
    `stats`: numpy int64[16], copied from the device on first use (a synchronisation): word 8 = records with a material
    examined, word 4 = resolved (status 0), word 9 = orphans (no chunk of the scene accounts for them), word 10 = records two
    chunks explain differently, of which the first was taken, word 11 = records the device refused, word 12 = resolved records
    with no open incoming side (normal 0)."""

    def __init__(self, records, stats_dev):
        import torch
        n = records.numel() // nat.SURFACE_BYTES
        f64 = records.view(torch.float64).view(n, nat.SURFACE_BYTES // 8)
        i8 = records.view(torch.int8).view(n, nat.SURFACE_BYTES)
        u8 = records.view(n, nat.SURFACE_BYTES)
        self.records = records           # uint8 [n * 64]
        self.vel = f64[:, 0:3]           # float64 [n, 3]: the velocity after the hit (of the unjittered ray: include/vrt.h)
        self.next = f64[:, 3:6]          # float64 [n, 3]: pos + vel * resolution, the ray's position one step on
        self.normal = i8[:, 48:51]       # int8 [n, 3]: one component -1 or +1; all 0: enclosed, or no surface
        self.status = i8[:, 51]          # int8 [n]: 0 a surface, -1 no hit, -2 orphan, -3 invalid input
        self.neighbour = u8[:, 52:55]    # uint8 [n, 3]: the material the reflection test found per axis (0: none)
        self.resolution = u8[:, 55]      # uint8 [n]: resolution of the chunk the ray stood in
        self.reflect = u8[:, 56]         # uint8 [n]: bit a: axis a is reflected
        self.side = u8[:, 57]            # uint8 [n]: bit a: the neighbour asked on axis a lies at +1
        self.fetched = u8[:, 58]         # uint8 [n]: bit a: that neighbour came through chunk_get
        self.open = u8[:, 59]            # uint8 [n]: bit a: the incoming-side neighbour of the normal rule is empty
        self._stats_dev = stats_dev

    def numpy(self):
        """The records as a numpy structured array (fields of vrt_surface)."""
        return np.ascontiguousarray(self.records.cpu().numpy()).view(np.dtype(nat.SURFACE_FIELDS)).reshape(-1)

    def surface_mask(self):
        """torch.bool [n]: the record describes a surface (status 0)."""
        return self.status == nat.SURFACE_OK

    def reflect_mask(self):
        """torch.bool [n, 3]: axis a of record k is reflected (always false where there is no surface)."""
        import torch
        bits = torch.tensor([1, 2, 4], dtype=torch.uint8, device=self.records.device)
        return (self.reflect[:, None] & bits[None, :]) != 0

    def normal_image(self, hit_result):
        """[height, width, 3] int8 normal image of the HitResult these surfaces were made from: the normal sample 0 of every
        pixel sees; 0 where it sees no surface and at pixels that are not listed."""
        import torch
        if hit_result.records.numel() // nat.HIT_BYTES != self.status.numel():
            raise ValueError("normal_image(): these surfaces were not made from that HitResult")
        return torch.stack([hit_result._scatter(self.normal[:, a], 0, torch.int8) for a in range(3)], dim=-1)

    def rays(self, lives):
        """The continuation rays as explicit rays: a [n, 8] float64 CUDA tensor of vrt_cast_ray records with origin = next,
        vel = vel and life = lives (a number, or [n]), which cast_rays, shade_rays and path_rays take as it is.  Records with
        status < 0 are eight NaNs, which every explicit-ray call rejects.  The doubles are copied, never computed with.
        A continuation starts with no current chunk: a ray that lands exactly on its old chunk's inclusive upper face re-snaps
        into the chunk above there, where the renderer's ray would have stayed in the old one."""
        import torch
        n = self.status.numel()
        dev = self.records.device
        rec = torch.empty((max(n, 1), 8), dtype=torch.float64, device=dev)[:n]
        rec[:, 0:3] = self.next
        rec[:, 3:6] = self.vel
        if isinstance(lives, torch.Tensor):
            if lives.numel() != n:
                raise ValueError("rays(): %d lives for %d records" % (lives.numel(), n))
            rec[:, 6] = lives.to(device=dev, dtype=torch.float64).reshape(n)
        elif np.ndim(lives) == 0:
            rec[:, 6] = float(lives)
        else:
            host = np.ascontiguousarray(lives, np.float64).reshape(-1)
            if host.size != n:
                raise ValueError("rays(): %d lives for %d records" % (host.size, n))
            rec[:, 6] = torch.from_numpy(host).to(dev)
        rec[:, 7] = 0.0
        # (a select, which neither computes with a double nor synchronises as an assignment through a mask would)
        return torch.where((self.status < 0)[:, None], torch.full_like(rec, float("nan")), rec)


class PhysicsResult(_LazyStats):
    """What DeviceWorld.tick() did.  `moved`: the Objects whose position changed, in physics order.  `records`: the body
    records as read back, a numpy structured array of vrt_body (include/vrt.h), one per object.  `counters`: its `out` fields
    alone (steps, blocked_steps, contacts, transfers, moved, status: 0 stepped, -1 skipped, -3 refused) -- the array
    world.tick() returns for the same tick.  `kernel_ms`: the kernel's time if it was asked for, else None.
    `stats`: numpy int64[16], copied from the device on first use: word 8 = bodies stepped, 9 = refused, 10 = steps, 11 = blocked
    steps, 12 = contacts, 13 = transfers, 14 = bodies the iteration cap ended; of a tick with rng also 15 = random.random() calls,
    which `draws` returns (0 for a tick without rng, which makes none), and 7 = 1 if the device found the generator's index out
    of range and did nothing."""

    def __init__(self, records, moved, stats_dev, kernel_ms=None):
        from .world import PHYSICS_COUNTER_FIELDS
        self.records, self.moved, self.kernel_ms = records, moved, kernel_ms
        self.counters = np.zeros(len(records), np.dtype(PHYSICS_COUNTER_FIELDS))
        for name, *_ in PHYSICS_COUNTER_FIELDS:
            self.counters[name] = records[name]
        self._stats_dev = stats_dev

    @property
    def draws(self):
        """The random.random() calls of the tick (word 15 of `stats`)."""
        return int(self.stats[nat.S_PHYSICS_DRAWS])


class ContactRecords:
    """The contact log of one run (world.Contacts is the request): `records`, a numpy structured array of
    _native.CONTACT_FIELDS with the byte layout of vrt_contact (include/vrt.h) -- tick, mover, other, step, voxel (the world
    voxel of `other` that was met; the mover's is voxel - dir), dir, mat_other, mat_mover -- in the reference's order, at most
    `capacity` rows.  `total`: all records the filters passed; `lost`: max(0, total - capacity), those that were counted and not
    stored.  `materials`: the list `mat_other` and `mat_mover` index; entry 0 is None.  Host and device number the materials
    alike for a DeviceWorld that meets the sprites for the first time; otherwise compare through `materials`."""

    def __init__(self, records, total, capacity, materials, objects=None):
        self.records, self.total, self.capacity = records, int(total), int(capacity)
        self.lost = max(0, self.total - self.capacity)
        self.materials = list(materials)
        self._objects = list(objects) if objects is not None else None

    def __len__(self):
        return len(self.records)

    def _index(self, who):
        if isinstance(who, (int, np.integer)):
            return int(who)
        where = [k for k, o in enumerate(self._objects or ()) if o is who]
        if not where:
            raise ValueError("ContactRecords: not an index and not one of the run's objects: %r" % (who,))
        return where[0]

    def of(self, mover=None, other=None):
        """The rows whose mover and whose other are the given ones (an Object of the run or an index; None: any)."""
        keep = np.ones(len(self.records), bool)
        if mover is not None:
            keep &= self.records["mover"] == self._index(mover)
        if other is not None:
            keep &= self.records["other"] == self._index(other)
        return self.records[keep]

    def first(self, mover, other=None):
        """The earliest such row, or None."""
        rows = self.of(mover, other)
        return rows[0] if len(rows) else None

    def pairs(self):
        """One row per (tick, mover, step, other): the first record of each, with `count`, the stored records it stands for --
        what turns a "voxels" log into touches with their sizes.  A structured array of CONTACT_FIELDS + count."""
        out = np.zeros(len(self.records), np.dtype(nat.CONTACT_FIELDS + [("count", "<i8")]))
        n, last = 0, None
        for r in self.records:
            key = (int(r["tick"]), int(r["mover"]), int(r["step"]), int(r["other"]))
            if key != last:
                for name, *_ in nat.CONTACT_FIELDS:
                    out[n][name] = r[name]
                n, last = n + 1, key
            out[n - 1]["count"] += 1
        return out[:n]


class RunResult(_LazyStats):
    """What DeviceWorld.run() did.  `records`: the body records after the last tick, a numpy structured array of vrt_body
    (include/vrt.h), one per object; their `out` fields are the last tick's (`counters`, as PhysicsResult's), and pad[0] says
    whether any tick moved the body (1) or changed its visibility (2).  `moved`: the Objects whose position changed during the
    run, in physics order.  `ticks_run`: the ticks done, always the ticks asked for; `launches`: the device launches they took
    (more than one where the work budget ended a launch early).  `kernel_ms`: the launches' summed time if it was asked for.
    `stats`: numpy int64[16], copied from the device on first use, summed over the launches: word 8 = body turns stepped,
    9 = refusals (a body counts once per tick that refused it), 10 = steps, 11 = blocked steps, 12 = contacts, 13 = transfers,
    14 = step loops the iteration cap ended, 5 = work units counted, 6 = ticks done.
    `trace`: None, or with trace=True a numpy structured array [ticks][n] of _native.BODY_SAMPLE_FIELDS -- every body after
    every tick -- copied from the device on first use.
    With clock= (the sprites animated): pad[0] of a record also says whether some tick's anim_update changed the frame at that
    body's turn (4); `frames`: {Sprite: its frame after the run} for every animated sprite (None without clock); `anim`: None,
    or with trace=True a numpy structured array [ticks][n] of _native.ANIM_SAMPLE_FIELDS -- every body's weight after every
    tick, its sprite's frame (-1: not animated) and whether the body made the switch at that tick.
    With rng= (the reference's random draws made on the device): `draws`: the random.random() calls of the run, an int (None
    without rng); `draws_per_tick`: a numpy uint64 array [ticks_run], each tick's (None without rng); word 15 of `stats` is
    the total as well.
    With contacts= (the contact log): `contacts`: the run's ContactRecords (None without contacts=).
    With impulses= (scripted accelerations): `impulses_applied`, `impulses_skipped`: the entries the device added to a
    velocity and those it refused to, ints (None without impulses=); words 0 and 1 of `stats` as well."""

    def __init__(self, records, moved, stats_dev, ticks_run, launches, trace_dev, trace_shape, kernel_ms=None, frames=None,
                 anim_dev=None, draws_per_tick=None, contacts=None, impulses=False):
        from .world import PHYSICS_COUNTER_FIELDS
        self.records, self.moved, self.kernel_ms = records, moved, kernel_ms
        self.ticks_run, self.launches = ticks_run, launches
        self.counters = np.zeros(len(records), np.dtype(PHYSICS_COUNTER_FIELDS))
        for name, *_ in PHYSICS_COUNTER_FIELDS:
            self.counters[name] = records[name]
        self._stats_dev = stats_dev
        self._trace_dev, self._trace_shape, self._trace = trace_dev, trace_shape, None
        self.frames, self._anim_dev, self._anim = frames, anim_dev, None
        self.draws_per_tick = draws_per_tick
        self.draws = int(draws_per_tick.sum()) if draws_per_tick is not None else None
        self.contacts = contacts
        self._impulses = bool(impulses)

    @property
    def impulses_applied(self):
        return int(self.stats[nat.S_PHYSICS_IMPULSES]) if self._impulses else None

    @property
    def impulses_skipped(self):
        return int(self.stats[nat.S_PHYSICS_IMPULSES_BAD]) if self._impulses else None

    @property
    def anim(self):
        if self._anim is None and self._anim_dev is not None:
            self._anim = self._anim_dev.cpu().numpy().view(np.dtype(nat.ANIM_SAMPLE_FIELDS)).reshape(self._trace_shape)
            self._anim_dev = None
        return self._anim

    @property
    def trace(self):
        if self._trace is None and self._trace_dev is not None:
            self._trace = self._trace_dev.cpu().numpy().view(np.dtype(nat.BODY_SAMPLE_FIELDS)).reshape(self._trace_shape)
            self._trace_dev = None
        return self._trace


class BatchRunResult(_LazyStats):
    """What DeviceWorld.run_many() did: K variants of one world, each stepped as run() steps a twin, none written into the
    caller's objects.  `records`: [K][n] vrt_body (include/vrt.h) after the last tick, as RunResult.records per variant, pad[0]
    included; `counters`: their `out` fields, [K][n].  `ticks_run`: [K] ticks each variant has behind it, always the ticks asked
    for; `launches`: the device launches the batch took (more than one where the work budget ended some run's share early).
    `kernel_ms`: the launches' summed time if it was asked for.
    `stats`: numpy int64[K][16], copied from the device on first use, summed over the launches: RunResult's words per variant
    (8 = body turns stepped, 9 = refusals, 10 = steps, 11 = blocked steps, 12 = contacts, 13 = transfers, 14 = capped step
    loops, 5 = work units, 6 = ticks done).
    `trace`: None, or with trace=True a numpy structured array [K][ticks][n] of _native.BODY_SAMPLE_FIELDS, copied from the
    device on first use.
    final(k): where variant k ends.  apply(k, objects): commit variant k to the objects.
    With rng= (the reference's random draws made on the device, a generator per variant): `draws`: numpy uint64 [K], the
    random.random() calls of each variant (word 15 of its `stats` as well); `draws_per_tick`: numpy uint64 [K][ticks];
    rng_state(k): the state variant k's generator ends in; apply(k, objects, rng=g) also sets g to it.  `draws` and
    `draws_per_tick` are None for a batch without rng=, and so is what rng_state(k) returns.
    With contacts= (a contact log per variant): contacts(k): variant k's ContactRecords; `contacts_total`: numpy uint64 [K],
    the records each variant's filters passed; `contacts_lost`: numpy uint64 [K], those beyond the capacity, counted and not
    stored.  All three are None for a batch without contacts=.
    With impulses= or the "impulses" key of a variant (scripted accelerations): `impulses_applied`, `impulses_skipped`: numpy
    uint64 [K], the entries each variant added to a velocity and those the device refused to (words 0 and 1 of its `stats`);
    None for a batch without impulses.  The final records hold what the impulses did: apply(k, objects) needs nothing more."""

    def __init__(self, records, start, changes, stats_dev, ticks_run, launches, trace_dev, trace_shape, kernel_ms=None,
                 draws_per_tick=None, rng_words=None, rng_start=None, contact_log=None, impulses=False):
        from .world import PHYSICS_COUNTER_FIELDS
        self.records, self.kernel_ms = records, kernel_ms
        self.ticks_run, self.launches = ticks_run, launches
        self.counters = np.zeros(records.shape, np.dtype(PHYSICS_COUNTER_FIELDS))
        for name, *_ in PHYSICS_COUNTER_FIELDS:
            self.counters[name] = records[name]
        self._start, self._changes = start, changes
        self._stats_dev = stats_dev
        self._trace_dev, self._trace_shape, self._trace = trace_dev, trace_shape, None
        self.draws_per_tick = draws_per_tick
        self.draws = draws_per_tick.sum(axis=1, dtype=np.uint64) if draws_per_tick is not None else None
        self._rng_words, self._rng_start = rng_words, rng_start
        # (contact_log: the [K][capacity] records as read back, the K counts, the capacity, the materials and the objects)
        self._contact_log = contact_log
        self._impulses = bool(impulses)
        self.contacts_total = self.contacts_lost = None
        if contact_log is not None:
            self.contacts_total = contact_log[1]
            self.contacts_lost = np.maximum(contact_log[1], np.uint64(contact_log[2])) - np.uint64(contact_log[2])

    @property
    def impulses_applied(self):
        return self.stats[:, nat.S_PHYSICS_IMPULSES].astype(np.uint64) if self._impulses else None

    @property
    def impulses_skipped(self):
        return self.stats[:, nat.S_PHYSICS_IMPULSES_BAD].astype(np.uint64) if self._impulses else None

    def contacts(self, k):
        """Variant k's contact log, as run(contacts=) on its twin returns it.  None for a batch without contacts=."""
        if self._contact_log is None:
            return None
        rows, counts, capacity, materials, objects = self._contact_log
        total = int(counts[k])
        return ContactRecords(rows[k][:min(total, capacity)].copy(), total, capacity, materials, objects)

    def rng_state(self, k):
        """The state variant k's generator ends in, as run(rng=) would have left it: the tuple random.Random.setstate takes,
        with the version and gauss_next of the generator variant k was handed.  None for a batch without rng=."""
        if self._rng_words is None:
            return None
        version, _, gauss_next = self._rng_start[k]
        return version, tuple(self._rng_words[k].tolist()), gauss_next

    @property
    def trace(self):
        if self._trace is None and self._trace_dev is not None:
            self._trace = self._trace_dev.cpu().numpy().view(np.dtype(nat.BODY_SAMPLE_FIELDS)).reshape(self._trace_shape)
            self._trace_dev = None
        return self._trace

    def final(self, k):
        """(pos [n][3], vel [n][3]) of variant k after its last tick, float64 copies."""
        return self.records[k]["pos"].copy(), self.records[k]["vel"].copy()

    def apply(self, k, objects, rng=None):
        """Write variant k's outcome into `objects` -- the objects run_many() was given, unchanged since -- exactly as run()
        writes its own into a twin that had the variant applied: first the variant itself (Object.move, the velocity), then
        pos, vel, mins, maxs, visible, cam_pos and redraw from the records.  Returns the Objects whose position changed
        during the run, in physics order (RunResult.moved).  update(objects) follows, as after run().
        rng: a random.Random (anything else: TypeError); if the batch drew, it is set to rng_state(k), where run(rng=) on
        the variant's twin would have left variant k's generator.  A batch without rng= leaves it alone."""
        from .world import _write_back_run
        objects = list(objects)
        if len(objects) != self.records.shape[1]:
            raise ValueError("apply(): %d objects for records of %d" % (len(objects), self.records.shape[1]))
        if rng is not None:
            import random
            if not isinstance(rng, random.Random):
                raise TypeError("apply(): rng must be a random.Random, not %r" % (rng,))
            if self._rng_words is not None:
                rng.setstate(self.rng_state(k))
        for at, pos, vel in self._changes[k]:
            if pos is not None:
                objects[at].move(pos)
            if vel is not None:
                objects[at].vel = type(vel)(vel.x, vel.y, vel.z)
        return _write_back_run(objects, self.records[k], self._start[k])
