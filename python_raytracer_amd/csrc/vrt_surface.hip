// vrt_surface.hip -- MI355X (gfx950) surface pass for hit records (vrt_hit_surfaces, include/vrt.h): how the surface lies
// at a hit -- the ray's velocity after the reference's reflection (init.py:84, 92-111), its position one step on
// (init.py:114-116), what the three neighbour lookups found, and the project's geometric normal.
//
// A translation unit of its own, linked into the same library as vrt_kernels.hip and built with the same flags.  It shares no
// code with that file: the three device helpers it needs -- the bricked voxel offset, Python's floor division for the LOD
// snap, and owner_candidate's rule for the chunk a ray stood in -- are restated here, and tests/test_gpu_surfaces.py holds the
// restatement to tests/surface_ref.py and to shade_kernel's own end state bit for bit.
//
// Arithmetic is binary64 in the reference's evaluation order; build with -ffp-contract=off.
// gfx950 only: 64-wide waves are assumed.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/vrt.h"

#pragma clang fp contract(off)

#define VRT_BLOCK 256
// waves per SIMD surface_kernel is compiled for (the second argument of its __launch_bounds__; 5 spills 4 VGPRs and gained
// nothing when measured) and the most workgroups of a launch (measured: 1024 and 2048 within 3 % of each other);
// -D overrides both for tools/build_variant.sh
#ifndef VRT_SURFACE_WAVES
#define VRT_SURFACE_WAVES 4
#endif
#ifndef VRT_SURFACE_GRID
#define VRT_SURFACE_GRID 2048
#endif

static_assert(sizeof(vrt_surface) == 64 && sizeof(vrt_hit) == 48 && sizeof(vrt_cast_ray) == 64, "record sizes of include/vrt.h");

struct SurfaceParams {
    const vrt_hit* hits;
    const vrt_cast_ray* rays;
    vrt_surface* out;
    int64_t n;
    const uint32_t* table;
    const uint8_t* voxels;
    const double* materials;
    unsigned long long* stats;
    int32_t n_slots, n_materials, cs, cs_shift;
    int32_t origin[3], dims[3];
};

// 16 bytes moved as one: the hit records are 8-byte aligned only, which a global 16-byte access allows
struct __attribute__((aligned(8))) Word16 {
    uint64_t a, b;
};

// byte offset of voxel (lx, ly, lz) inside a chunk's block: 8^3 bricks [bx][by][bz] of 8 micro-bricks [mx][my][mz] of 4^3
// voxels [x][y][z] (include/vrt.h, vrt_scene; vrt_voxel_offset)
__device__ __forceinline__ int64_t surface_voxel_offset(int cs, int lx, int ly, int lz) {
    const int nb = cs >> 3;
    const int brick = (((lx >> 3) * nb) + (ly >> 3)) * nb + (lz >> 3);
    const int micro = ((((lx >> 2) & 1) * 2) + ((ly >> 2) & 1)) * 2 + ((lz >> 2) & 1);
    const int vox = (((lx & 3) * 4) + (ly & 3)) * 4 + (lz & 3);
    return (int64_t)brick * 512 + micro * 64 + vox;
}

// (c // r) * r for one coordinate, Python's floor division, without a branch: |f| < 2^29 and 1 <= r <= 255, so the binary64
// quotient is either exact or at least 2^-8 away from a whole number, and its floor is the floor of f / r
__device__ __forceinline__ int surface_snap(int f, int r) {
    return (int)__builtin_floor((double)f / (double)r) * r;
}

// N independent probes, in phases so that their memory accesses overlap: the table words of the chunk cells k[a] together,
// then the voxel bytes.  byte[a]: what Frame.get_voxel gives for world cell q[a] in chunk cell k[a] -- the voxel at
// (q // r') * r' with that chunk's own r' -- and 0 if the probe is not asked, the cell lies outside the table or is not listed,
// or that voxel lies outside the chunk.  res[a]: r' of a listed chunk, else 0.  Every index is checked before it is used.
template <int N>
__device__ __forceinline__ void surface_probes(const SurfaceParams& P, const bool (&ask)[N], const int (&k)[N][3], const int (&q)[N][3],
                                               unsigned (&byte)[N], int (&res)[N]) {
    uint32_t entry[N];
    bool in[N];
#pragma unroll
    for (int a = 0; a < N; a++) {
        // (& and not &&: flags, not branches -- a branch between two loads would make the second wait for the first)
        in[a] = ask[a] & ((unsigned)k[a][0] < (unsigned)P.dims[0]) & ((unsigned)k[a][1] < (unsigned)P.dims[1]) &
                ((unsigned)k[a][2] < (unsigned)P.dims[2]);
        const int64_t cell = in[a] ? ((int64_t)k[a][0] * P.dims[1] + k[a][1]) * P.dims[2] + k[a][2] : 0;
        entry[a] = P.table[cell];  // (cell 0 exists: the load needs no branch)
    }
    const uint8_t* at[N];
    bool ok[N];
#pragma unroll
    for (int a = 0; a < N; a++) {
        const int slot = (int)(entry[a] & 0xffffffu) - 1, r = (int)(entry[a] >> 24);
        const bool listed = in[a] & (slot >= 0) & (slot < P.n_slots) & (r >= 1);
        res[a] = listed ? r : 0;
        const int rr = listed ? r : 1;
        const int lx = surface_snap(q[a][0], rr) - (P.origin[0] + (k[a][0] << P.cs_shift)),
                  ly = surface_snap(q[a][1], rr) - (P.origin[1] + (k[a][1] << P.cs_shift)),
                  lz = surface_snap(q[a][2], rr) - (P.origin[2] + (k[a][2] << P.cs_shift));
        ok[a] = listed & ((unsigned)lx < (unsigned)P.cs) & ((unsigned)ly < (unsigned)P.cs) & ((unsigned)lz < (unsigned)P.cs);
        // (a probe that reads no voxel reads the table's first byte instead and drops it: loads without a branch between
        // them, so they leave together)
        at[a] = ok[a] ? P.voxels + (((int64_t)slot << (3 * P.cs_shift)) + surface_voxel_offset(P.cs, lx, ly, lz))
                      : reinterpret_cast<const uint8_t*>(P.table);
    }
    unsigned got[N];
#pragma unroll
    for (int a = 0; a < N; a++) got[a] = *at[a];
#pragma unroll
    for (int a = 0; a < N; a++) byte[a] = ok[a] ? got[a] : 0u;
}

// owner_candidate's question for chunk cell (kx, ky, kz): does the table list it, does (cell // r) * r lie inside it, and does
// the voxel there hold `material`?  r: its resolution if so.
__device__ __forceinline__ bool surface_candidate(const SurfaceParams& P, int kx, int ky, int kz, const int (&f)[3], int material, int& r) {
    if ((unsigned)kx >= (unsigned)P.dims[0] || (unsigned)ky >= (unsigned)P.dims[1] || (unsigned)kz >= (unsigned)P.dims[2]) return false;
    const uint32_t entry = P.table[((int64_t)kx * P.dims[1] + ky) * P.dims[2] + kz];
    const int slot = (int)(entry & 0xffffffu) - 1;
    r = (int)(entry >> 24);
    if (slot < 0 || slot >= P.n_slots || r < 1) return false;
    const int lx = surface_snap(f[0], r) - (P.origin[0] + (kx << P.cs_shift)), ly = surface_snap(f[1], r) - (P.origin[1] + (ky << P.cs_shift)),
              lz = surface_snap(f[2], r) - (P.origin[2] + (kz << P.cs_shift));
    if ((unsigned)lx >= (unsigned)P.cs || (unsigned)ly >= (unsigned)P.cs || (unsigned)lz >= (unsigned)P.cs) return false;
    return (int)P.voxels[((int64_t)slot << (3 * P.cs_shift)) + surface_voxel_offset(P.cs, lx, ly, lz)] == material;
}

// What the reflection of init.py:92-111 gives for a ray that stood in chunk cell (kx, ky, kz)
struct SurfaceReflection {
    double v[3];
    unsigned neighbour;  // byte a: the material found on axis a
    unsigned reflect, side, fetched;
};

__device__ __forceinline__ SurfaceReflection surface_reflect(const SurfaceParams& P, const double* s_ior, int kx, int ky, int kz,
                                                             const double (&pos)[3], const int (&f)[3], const double (&v)[3], double ior) {
    SurfaceReflection R = {{v[0], v[1], v[2]}, 0u, 0u, 0u, 0u};
    if (ior == 0.0) return R;
    const double direction = (ior - 0.5) * 2;
    const int kc[3] = {kx, ky, kz};
    double cmin[3], cmax[3];
    bool pin[3];  // the ray's own coordinate lies in the chunk's inclusive box
#pragma unroll
    for (int a = 0; a < 3; a++) {
        cmin[a] = (double)(P.origin[a] + (kc[a] << P.cs_shift));
        cmax[a] = cmin[a] + (double)P.cs;
        pin[a] = (pos[a] >= cmin[a]) & (pos[a] <= cmax[a]);
    }
    const bool ask[3] = {true, true, true};
    int k[3][3], q[3][3];
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const bool up = v[a] < direction;
        const double p = up ? pos[a] + 1 : pos[a] - 1;
        R.side |= (unsigned)up << a;
        // init.py:100-102: the current chunk while the point lies inside its inclusive box, else Camera.chunk_get, which
        // snaps every coordinate of the point
        const bool inside = (p >= cmin[a]) & (p <= cmax[a]) & pin[(a + 1) % 3] & pin[(a + 2) % 3];
        R.fetched |= (unsigned)!inside << a;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            q[a][c] = c == a ? (int)__builtin_floor(p) : f[c];
            k[a][c] = inside ? kc[c] : (q[a][c] - P.origin[c]) >> P.cs_shift;
        }
    }
    unsigned byte[3];
    int res[3];
    surface_probes<3>(P, ask, k, q, byte, res);
    double nior[3];
#pragma unroll
    for (int a = 0; a < 3; a++) nior[a] = s_ior[byte[a]];
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const bool solid = (byte[a] != 0u) & (nior[a] == ior);
        R.neighbour |= byte[a] << (8 * a);
        R.reflect |= (unsigned)!solid << a;
        R.v[a] = solid ? v[a] : v[a] - v[a] * ior * 2;
    }
    return R;
}

__global__ void __launch_bounds__(VRT_BLOCK) surface_begin_kernel(uint32_t* stats) {
    if (threadIdx.x < 2 * VRT_NSTATS) stats[threadIdx.x] = 0u;
}

// One lane per record at a time; a workgroup strides over the launch's records.
__global__ void __launch_bounds__(VRT_BLOCK, VRT_SURFACE_WAVES) surface_kernel(SurfaceParams P) {
    // ior by material id; NaN for id 0 and ids the scene has no material for: such a neighbour never counts as solid
    __shared__ double s_ior[256];
    __shared__ unsigned s_count[6];  // the workgroup's records examined, resolved, orphaned, ambiguous, refused, enclosed
    if (threadIdx.x < 6) s_count[threadIdx.x] = 0u;
    {
        const int id = threadIdx.x;
        s_ior[id] = (id >= 1 && id <= P.n_materials) ? P.materials[(id - 1) * 8 + 5] : __builtin_nan("");
    }
    __syncthreads();
    // the wave's counts: summed over its records, added to the workgroup's once at the end
    unsigned n_exam = 0, n_found = 0, n_orphan = 0, n_amb = 0, n_inv = 0, n_enc = 0;
    for (int64_t base = (int64_t)blockIdx.x * VRT_BLOCK; base < P.n; base += (int64_t)gridDim.x * VRT_BLOCK) {
        const int64_t i = base + threadIdx.x;
        const bool live = i < P.n;
        int material = 0;
        int f[3] = {0, 0, 0};
        double pos[3] = {0, 0, 0}, v[3] = {0, 0, 0};
        if (live) {
            const Word16* h = reinterpret_cast<const Word16*>(P.hits + i);
            const Word16 h0 = h[0], h1 = h[1], h2 = h[2];
            const Word16* rr = reinterpret_cast<const Word16*>(P.rays + i);
            const Word16 r1 = rr[1], r2 = rr[2];  // origin[2] vel[0] | vel[1] vel[2]
            material = (int)(h2.b >> 32);
            pos[0] = __longlong_as_double((long long)h0.b), pos[1] = __longlong_as_double((long long)h1.a),
            pos[2] = __longlong_as_double((long long)h1.b);
            f[0] = (int)(uint32_t)h2.a, f[1] = (int)(h2.a >> 32), f[2] = (int)(uint32_t)h2.b;
            v[0] = __longlong_as_double((long long)r1.b), v[1] = __longlong_as_double((long long)r2.a),
            v[2] = __longlong_as_double((long long)r2.b);
        }
        const bool examined = material > 0;
        bool invalid = false;
        if (examined) {
            const double lim = (double)(1 << 28);
            bool good = material <= P.n_materials;
#pragma unroll
            for (int a = 0; a < 3; a++) {
                // (a NaN fails the first comparison, an infinity the second or third)
                good = good & (__builtin_fabs(pos[a]) < lim) & (__builtin_fabs(v[a]) < __builtin_inf()) & ((double)f[a] == __builtin_floor(pos[a]));
            }
            invalid = !good;
        }
        const bool work = examined && !invalid;
        const double ior = work ? s_ior[material] : 0.0;
        double ref = 0.0;
        if (work) {
            // Chebyshev normalize (lib.py:310-314)
            ref = __builtin_fmax(__builtin_fabs(v[0]), __builtin_fmax(__builtin_fabs(v[1]), __builtin_fabs(v[2])));
            if (ref != 0.0 && ref != 1.0) v[0] /= ref, v[1] /= ref, v[2] /= ref;
        }
        // ---- the normal: the incoming-side neighbour cell of every axis the ray moves on; it does not depend on the ray's chunk.
        // The fourth probe of the batch is the first candidate for that chunk, the one containing `cell`: nearly always the one taken
        unsigned open = 0, byte0 = 0;
        int normal_axis = -1, normal_sign = 0, res0 = 0;
        if (work) {
            bool ask[4];
            int k[4][3], q[4][3];
#pragma unroll
            for (int a = 0; a < 3; a++) {
                ask[a] = v[a] != 0.0;
                const int sgn = v[a] > 0.0 ? 1 : -1;
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    q[a][c] = c == a ? f[c] - sgn : f[c];
                    k[a][c] = (q[a][c] - P.origin[c]) >> P.cs_shift;
                }
            }
            ask[3] = true;
#pragma unroll
            for (int c = 0; c < 3; c++) q[3][c] = f[c], k[3][c] = (f[c] - P.origin[c]) >> P.cs_shift;
            unsigned byte[4];
            int res[4];
            surface_probes<4>(P, ask, k, q, byte, res);
            byte0 = byte[3], res0 = res[3];
            double best = 0.0;
#pragma unroll
            for (int a = 0; a < 3; a++) {
                if (ask[a] && byte[a] == 0u) {
                    open |= 1u << a;
                    if (__builtin_fabs(v[a]) > best) best = __builtin_fabs(v[a]), normal_axis = a, normal_sign = v[a] > 0.0 ? -1 : 1;
                }
            }
        }
        // ---- the chunk the ray stood in: vrt_hit_owners's candidates in their order, the first that counts; a later one that
        // counts and reflects differently makes the record ambiguous
        bool found = false, ambiguous = false;
        int resolution = 0;
        SurfaceReflection R = {{0, 0, 0}, 0u, 0u, 0u, 0u};
        if (work) {
            const int cm = P.cs - 1;
            unsigned low = 0;  // bit a: pos[a] is a whole multiple of chunk_size, so the ray may still have stood in the chunk below
#pragma unroll
            for (int a = 0; a < 3; a++) low |= (unsigned)(pos[a] == (double)f[a] && (f[a] & cm) == 0) << a;
            const int base[3] = {(f[0] - P.origin[0]) >> P.cs_shift, (f[1] - P.origin[1]) >> P.cs_shift, (f[2] - P.origin[2]) >> P.cs_shift};
#pragma nounroll
            for (int m = 0; m < 8; m++) {
                if (m & ~low) continue;
                const int kx = base[0] - (m & 1), ky = base[1] - ((m >> 1) & 1), kz = base[2] - ((m >> 2) & 1);
                int r = res0;
                if (m == 0) {
                    if ((int)byte0 != material) continue;  // (0 unless the chunk is listed and holds the snapped voxel: material > 0)
                } else {
                    if (!surface_candidate(P, kx, ky, kz, f, material, r)) continue;
                }
                const SurfaceReflection G = surface_reflect(P, s_ior, kx, ky, kz, pos, f, v, ior);
                if (!found) {
                    found = true, resolution = r, R = G;
                } else {
                    // (compared as bit patterns: a reflected -0.0 is another velocity than 0.0)
                    ambiguous = ambiguous || __double_as_longlong(G.v[0]) != __double_as_longlong(R.v[0]) ||
                                __double_as_longlong(G.v[1]) != __double_as_longlong(R.v[1]) ||
                                __double_as_longlong(G.v[2]) != __double_as_longlong(R.v[2]) || G.reflect != R.reflect || G.neighbour != R.neighbour;
                }
            }
        }
        const bool orphan = work && !found;
        const bool enclosed = found && normal_axis < 0;
        if (live) {
            Word16 w0 = {0, 0}, w1 = {0, 0}, w2 = {0, 0}, w3 = {0, 0};
            const int status = !examined ? VRT_SURFACE_NONE : (invalid ? VRT_SURFACE_INVALID : (orphan ? VRT_SURFACE_ORPHAN : 0));
            w3.a = (uint64_t)(uint8_t)status << 24;
            if (found) {
                const double rd = (double)resolution;
                const double nx = pos[0] + R.v[0] * rd, ny = pos[1] + R.v[1] * rd, nz = pos[2] + R.v[2] * rd;
                w0.a = (uint64_t)__double_as_longlong(R.v[0]), w0.b = (uint64_t)__double_as_longlong(R.v[1]);
                w1.a = (uint64_t)__double_as_longlong(R.v[2]), w1.b = (uint64_t)__double_as_longlong(nx);
                w2.a = (uint64_t)__double_as_longlong(ny), w2.b = (uint64_t)__double_as_longlong(nz);
                if (normal_axis >= 0) w3.a |= (uint64_t)(uint8_t)normal_sign << (8 * normal_axis);
                w3.a |= (uint64_t)(R.neighbour & 0xffffffu) << 32 | (uint64_t)(uint8_t)resolution << 56;
                w3.b = (uint64_t)R.reflect | (uint64_t)R.side << 8 | (uint64_t)R.fetched << 16 | (uint64_t)open << 24;
            }
            Word16* o = reinterpret_cast<Word16*>(P.out + i);
            o[0] = w0, o[1] = w1, o[2] = w2, o[3] = w3;
        }
        n_exam += (unsigned)__popcll(__ballot(examined)), n_found += (unsigned)__popcll(__ballot(found));
        n_orphan += (unsigned)__popcll(__ballot(orphan)), n_amb += (unsigned)__popcll(__ballot(ambiguous));
        n_inv += (unsigned)__popcll(__ballot(invalid)), n_enc += (unsigned)__popcll(__ballot(enclosed));
    }
    // by wave ballot into the workgroup's six words in LDS, then one atomic per workgroup and word: the statistics words share
    // one cache line, and with an atomic per wave and word on it the pass spent most of its time queueing there (2.07 M records:
    // 0.41 ms with a wave per 64 records, 0.15 ms with 2048 striding workgroups, 0.10 ms with these -- DESIGN.md section 4h)
    if ((threadIdx.x & 63) == 0) {
        atomicAdd(&s_count[0], n_exam), atomicAdd(&s_count[1], n_found), atomicAdd(&s_count[2], n_orphan);
        atomicAdd(&s_count[3], n_amb), atomicAdd(&s_count[4], n_inv), atomicAdd(&s_count[5], n_enc);
    }
    __syncthreads();
    if (threadIdx.x < 6 && s_count[threadIdx.x]) {
        const int word[6] = {VRT_S_SURFACE_EXAMINED, VRT_S_SURFACE_RESOLVED, VRT_S_SURFACE_ORPHANS, VRT_S_SURFACE_AMBIGUOUS, VRT_S_SURFACE_INVALID,
                             VRT_S_SURFACE_ENCLOSED};
        atomicAdd(&P.stats[word[threadIdx.x]], (unsigned long long)s_count[threadIdx.x]);
    }
}

extern "C" int vrt_hit_surfaces(const vrt_scene* sc, const vrt_hit* d_hits, const vrt_cast_ray* d_rays, int64_t n, vrt_surface* d_surfaces,
                                uint64_t* d_stats, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    // (every check comes before any HIP call)
    if (!sc || !d_stats || n < 0 || n >= (1ll << 32)) return VRT_ERR_ARG;
    if (n > 0 && (!d_hits || !d_rays || !d_surfaces || ((uintptr_t)d_hits & 7) != 0 || ((uintptr_t)d_rays & 63) != 0 ||
                  ((uintptr_t)d_surfaces & 63) != 0))
        return VRT_ERR_ARG;
    const int cs = sc->chunk_size;
    if (cs < 8 || cs > 256 || (cs & (cs - 1))) return VRT_ERR_ARG;
    if (!sc->d_chunk_table || sc->n_slots < 0 || sc->n_slots >= (1 << 24) || (sc->n_slots > 0 && !sc->d_voxels)) return VRT_ERR_ARG;
    if (sc->n_materials < 0 || sc->n_materials > 255 || (sc->n_materials > 0 && (!sc->d_materials || ((uintptr_t)sc->d_materials & 7) != 0)))
        return VRT_ERR_ARG;
    SurfaceParams P;
    int64_t cells = 1;
    for (int a = 0; a < 3; a++) {
        if (sc->dims[a] <= 0 || (sc->origin[a] % cs) != 0) return VRT_ERR_ARG;
        if (sc->origin[a] < -(1ll << 28) || sc->origin[a] + (int64_t)sc->dims[a] * cs > (1ll << 28)) return VRT_ERR_ARG;
        P.origin[a] = (int32_t)sc->origin[a];
        P.dims[a] = sc->dims[a];
        cells *= sc->dims[a];
    }
    if (cells >= (1ll << 31)) return VRT_ERR_ARG;
    int shift = 0;
    while ((1 << shift) < cs) shift++;
    P.cs = cs;
    P.cs_shift = shift;
    P.n_slots = sc->n_slots;
    P.n_materials = sc->n_materials;
    P.table = sc->d_chunk_table;
    P.voxels = sc->d_voxels;
    P.materials = sc->d_materials;
    P.stats = (unsigned long long*)d_stats;
    // (a kernel, not hipMemsetAsync: vrt_kernels.hip, clear_words_kernel)
    hipLaunchKernelGGL(surface_begin_kernel, dim3(1), dim3(VRT_BLOCK), 0, stream, (uint32_t*)d_stats);
    const int64_t per_launch = (int64_t)1 << 28;
    for (int64_t r0 = 0; r0 < n; r0 += per_launch) {
        P.n = n - r0 < per_launch ? n - r0 : per_launch;
        P.hits = d_hits + r0;
        P.rays = d_rays + r0;
        P.out = d_surfaces + r0;
        // at most VRT_SURFACE_GRID workgroups, each striding over the launch's records and adding to the statistics once
        const int64_t blocks = (P.n + VRT_BLOCK - 1) / VRT_BLOCK;
        hipLaunchKernelGGL(surface_kernel, dim3((unsigned)(blocks < VRT_SURFACE_GRID ? blocks : VRT_SURFACE_GRID)), dim3(VRT_BLOCK), 0, stream, P);
    }
    if (hipGetLastError() != hipSuccess) return VRT_ERR_HIP;
    return VRT_OK;
}
