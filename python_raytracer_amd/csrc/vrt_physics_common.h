// vrt_physics_common.h -- what the two object-physics units share (vrt_physics.hip: vrt_physics_tick, the tick that makes no
// draws; vrt_physics_draws.hip: vrt_physics_tick_draws, the tick that makes the reference's): the kernel's arguments, the state of
// the body whose turn it is, the model lookup with its quarter-turn addressing, the refusal rules and the ordered compaction.
// Device helpers only, all forced inline; included after <hip/hip_runtime.h> and include/vrt.h.
#pragma once

#define VRT_PHYS_BLOCK 1024
#define VRT_PHYS_WAVES (VRT_PHYS_BLOCK / 64)

static_assert(sizeof(vrt_body) == 192 && sizeof(vrt_object) == 64 && sizeof(vrt_physics_params) == 40, "record sizes of include/vrt.h");

struct PhysParams {
    vrt_body* bodies;
    const uint8_t* models;
    const uint8_t* remap;
    const double* matphys;
    unsigned long long* stats;
    int64_t models_bytes;
    int32_t n, remap_bytes, n_materials;
    vrt_physics_params p;
};

// the state of the body whose turn it is; lane 0 writes it, every lane reads it after a barrier
struct PhysSelf {
    double pos[3], vel[3], va[3];  // va: vel_apply of data.py:499
    double weight, friction, elasticity;
    int32_t mins[3], maxs[3], half[3];
    int32_t dir[3];                // vel_dir of data.py:501
    int32_t lo[3], ext[3];         // the slab: first voxel and voxels per axis (data.py:506-517)
    int64_t rim;
    int32_t run, done, blocked;
    int32_t steps, blocked_steps, contacts, transfers, moved;
};

// Sprite.pos_rotated (data.py:338-371): where a model rotated in quarter turns is read for local position (x, y, z); a turn about
// an axis whose two other extents differ is ignored
__device__ __forceinline__ void physics_rotate(const vrt_object& o, int& x, int& y, int& z) {
    const int ex = o.size[0] - 1, ey = o.size[1] - 1, ez = o.size[2] - 1;
    const int ax = o.turns[0], ay = o.turns[1], az = o.turns[2];
    int a, b, c;
    if (ax && o.size[1] == o.size[2]) {
        a = x;
        b = ax == 1 ? ez - z : (ax == 2 ? ey - y : z);
        c = ax == 1 ? y : (ax == 2 ? ez - z : ey - y);
        x = a, y = b, z = c;
    }
    if (ay && o.size[0] == o.size[2]) {
        a = ay == 1 ? z : (ay == 2 ? ex - x : ez - z);
        b = y;
        c = ay == 1 ? ex - x : (ay == 2 ? ez - z : x);
        x = a, y = b, z = c;
    }
    if (az && o.size[0] == o.size[1]) {
        a = az == 1 ? ey - y : (az == 2 ? ex - x : y);
        b = az == 1 ? x : (az == 2 ? ey - y : ex - x);
        c = z;
        x = a, y = b, z = c;
    }
}

// Sprite.get_voxel for object `o` at local position (x, y, z) = world voxel - mins: the world material id, 0 = no voxel.
// Positions outside the model hold nothing (a missing key of Frame.get_voxel) -- but for the plane at x = size.x, which the
// reference's import fills (data.py:287) and its inclusive box test reaches: `rim` is that plane's offset, -1 if it is empty.
// Every index is checked before it is used; the ranges [model, model + size.x * size.y * size.z) and [rim, rim + size.y * size.z)
// were checked against models_bytes when the body was validated.
__device__ __forceinline__ int physics_material(const PhysParams& P, const vrt_object& o, int64_t rim, int x, int y, int z) {
    physics_rotate(o, x, y, z);
    if (x < 0 || y < 0 || z < 0 || x > o.size[0] || y >= o.size[1] || z >= o.size[2]) return 0;
    if (x == o.size[0] && rim < 0) return 0;
    const int local = x == o.size[0] ? P.models[rim + (int64_t)y * o.size[2] + z] : P.models[o.model + ((int64_t)x * o.size[1] + y) * o.size[2] + z];
    if (!local) return 0;
    const int64_t at = (int64_t)o.remap + local;
    if (at >= P.remap_bytes) return 0;
    const int g = P.remap[at];
    return g <= P.n_materials ? g : 0;
}

// vrt.h's refusal rules for one body
__device__ __forceinline__ bool physics_valid(const PhysParams& P, const vrt_body& b) {
    const double lim = (double)(1 << 28);
    bool good = true;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        // (a NaN fails every comparison)
        good = good & (__builtin_fabs(b.pos[a]) < lim) & (__builtin_fabs(b.vel[a]) <= (double)VRT_PHYSICS_MAX_VEL);
        good = good & (b.half[a] >= 0) & (b.half[a] <= VRT_PHYSICS_MAX_HALF);
        const int64_t mn = b.object.mins[a], mx = b.object.maxs[a];
        good = good & (mn > -(1ll << 29)) & (mx < (1ll << 29)) & (mx - mn >= 0) & (mx - mn <= 2 * VRT_PHYSICS_MAX_HALF + 1);
    }
    good = good & (__builtin_fabs(b.weight) < __builtin_inf());
    if (b.has_sprite) {
        int64_t vol = 1;
#pragma unroll
        for (int a = 0; a < 3; a++) {
            good = good & (b.object.size[a] >= 0) & (b.object.size[a] <= 32768);
            vol *= good ? b.object.size[a] : 0;
        }
        good = good & (b.object.model >= 0) & (vol <= P.models_bytes) & (b.object.model <= P.models_bytes - vol);
        good = good & (b.object.remap >= 0) & (b.object.remap <= P.remap_bytes);
        const int64_t plane = good ? (int64_t)b.object.size[1] * b.object.size[2] : 0;
        good = good & (b.rim >= -1) & (b.rim < 0 || (plane <= P.models_bytes && b.rim <= P.models_bytes - plane));
    }
    return good;
}

__device__ __forceinline__ int physics_ceil(double v) { return (int)__builtin_ceil(v); }
__device__ __forceinline__ int physics_floor(double v) { return (int)__builtin_floor(v); }

// Rank of this lane among the set lanes of `mask`, and the ordered offset of its wave among the workgroup's waves: the
// compaction keeps thread order, which is the reference's loop order.  s_wave: one count per wave.  Two barriers.
__device__ __forceinline__ int physics_slot(bool flag, int* s_wave) {
    const unsigned long long mask = __ballot(flag);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) s_wave[wave] = __popcll(mask);
    __syncthreads();
    int off = 0;
    for (int w = 0; w < wave; w++) off += s_wave[w];
    return off + __popcll(mask & ((1ull << lane) - 1ull));
}

// What both entry points refuse before any HIP call (include/vrt.h)
static inline bool physics_args_ok(const vrt_body* d_bodies, int32_t n_bodies, const uint8_t* d_models, int64_t models_bytes,
                                   const uint8_t* d_remap, int32_t remap_bytes, const double* d_matphys, int32_t n_materials,
                                   const vrt_physics_params* params, const uint64_t* d_stats) {
    if (!d_stats || !params || ((uintptr_t)d_stats & 7) != 0 || n_bodies < 0 || n_bodies > (1 << 20)) return false;
    if (models_bytes < 0 || remap_bytes < 0 || n_materials < 0 || n_materials > 255) return false;
    if ((models_bytes > 0 && !d_models) || (remap_bytes > 0 && !d_remap)) return false;
    if (n_bodies > 0 && (!d_bodies || !d_matphys || ((uintptr_t)d_bodies & 7) != 0 || ((uintptr_t)d_matphys & 7) != 0)) return false;
    const double v[5] = {params->gravity, params->friction, params->friction_air, params->min_velocity, params->max_velocity};
    for (int a = 0; a < 5; a++)
        if (!(__builtin_fabs(v[a]) < __builtin_inf())) return false;
    return true;
}
