// vrt_chunk_lists.hip -- MI355X (gfx950) per-chunk object lists (vrt_chunk_lists_build, include/vrt.h) and the two passes that
// read them instead of the whole object array: vrt_voxelize_lists and vrt_hit_owners_lists.  The lists are the reference's
// Window.chunks_objects (init.py:398-444) as two device arrays: for every chunk of the world box the objects whose box meets it,
// in merge order.
//
// A translation unit of its own, linked into the same library as vrt_kernels.hip and built with the same flags.  It shares no
// code with that file.  The helpers of the voxelisation and of the owner pass that the list-driven kernels need are RESTATED
// here; the originals are in vrt_kernels.hip: voxel_offset under "shared helpers", rotate_index next to voxelize_kernel,
// owner_probe, owner_snap and owner_candidate next to owner_kernel.  tests/test_gpu_chunk_lists.py holds every restatement to the
// original, byte for byte, through the results of the two pairs of entry points.
//
// gfx950 only: 64-wide waves are assumed.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/vrt.h"

#define VRT_BLOCK 256
#define VRT_LISTS_SCAN_BLOCK 1024
#define VRT_LISTS_SCAN_PER_THREAD 4
#define VRT_LISTS_TILE 128                // object records a voxelize_lists workgroup stages in LDS at a time: 8 KiB
#define VRT_LISTS_SENTINEL 0xffffffffu    // d_offsets[n_chunks] of lists that did not fit (n_items_cap < 2^31: never an offset)

static_assert(sizeof(vrt_object) == 64 && sizeof(vrt_hit) == 48 && sizeof(vrt_owner) == 32, "record sizes of include/vrt.h");

// ---------------------------------------------------------------------------------------------
// restated helpers (originals: vrt_kernels.hip)
// ---------------------------------------------------------------------------------------------
__device__ static __forceinline__ int64_t voxel_offset(int cs, int lx, int ly, int lz) {
    int nb = cs >> 3;
    int brick = (((lx >> 3) * nb) + (ly >> 3)) * nb + (lz >> 3);
    int micro = ((((lx >> 2) & 1) * 2) + ((ly >> 2) & 1)) * 2 + ((lz >> 2) & 1);
    int vox = (((lx & 3) * 4) + (ly & 3)) * 4 + (lz & 3);
    return (int64_t)brick * 512 + micro * 64 + vox;
}

// Sprite.pos_rotated (data.py:338-371): where a model rotated in quarter turns is read for local position (x, y, z)
__device__ static __forceinline__ void rotate_index(const vrt_object& o, int& x, int& y, int& z) {
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

// voxelize_kernel's question for one object: the model byte object `o` holds at world voxel (wx, wy, wz), 0 = none
__device__ static __forceinline__ int owner_probe(const vrt_object& o, const uint8_t* models, int wx, int wy, int wz, int& x, int& y,
                                                  int& z) {
    if (wx < o.mins[0] || wy < o.mins[1] || wz < o.mins[2] || wx >= o.maxs[0] || wy >= o.maxs[1] || wz >= o.maxs[2]) return 0;
    x = wx - o.mins[0], y = wy - o.mins[1], z = wz - o.mins[2];
    rotate_index(o, x, y, z);
    if (x < 0 || y < 0 || z < 0 || x >= o.size[0] || y >= o.size[1] || z >= o.size[2]) return 0;
    return models[o.model + ((int64_t)x * o.size[1] + y) * o.size[2] + z];
}

// (c // r) * r for one coordinate, Python's floor division
__device__ static __forceinline__ int owner_snap(int f, int r) {
    if (r == 1) return f;
    if (r == 2) return f & ~1;
    int q = f / r;
    if (f - q * r < 0) q--;
    return q * r;
}

// the lists as a kernel sees them: the box in 32-bit words (the entry points check the range), the capacity, the two arrays
struct ListsView {
    const uint32_t* offsets;
    const int32_t* items;
    int32_t origin[3], dims[3];
    int32_t cs_shift, n_chunks;
    uint32_t cap;
};

struct ListsOwnerParams {
    const vrt_hit* hits;
    vrt_owner* owners;
    int64_t n;
    const vrt_object* objects;
    const uint8_t* models;
    const uint8_t* remap;
    const uint32_t* table;
    const uint8_t* voxels;
    unsigned long long* stats;
    int32_t n_objects, n_slots, cs, cs_shift;
    int32_t origin[3], dims[3];
    ListsView L;
};
struct ListsOwnerFound {
    int object, lx, ly, lz;
};

// Candidate chunk `m` of a record (bit a of m: the chunk one below the containing one on axis a): if the camera table lists
// it, the voxel (cell // r) * r lies inside it and holds `material`, returns its resolution and the voxel; else 0.
__device__ static __forceinline__ int owner_candidate(const ListsOwnerParams& P, int m, int fx, int fy, int fz, int material, int& cx,
                                                      int& cy, int& cz) {
    const int kx = ((fx - P.origin[0]) >> P.cs_shift) - (m & 1), ky = ((fy - P.origin[1]) >> P.cs_shift) - ((m >> 1) & 1),
              kz = ((fz - P.origin[2]) >> P.cs_shift) - ((m >> 2) & 1);
    if ((unsigned)kx >= (unsigned)P.dims[0] || (unsigned)ky >= (unsigned)P.dims[1] || (unsigned)kz >= (unsigned)P.dims[2]) return 0;
    const uint32_t entry = P.table[((int64_t)kx * P.dims[1] + ky) * P.dims[2] + kz];
    const int slot = (int)(entry & 0xffffffu) - 1, r = (int)(entry >> 24);
    if (slot < 0 || slot >= P.n_slots || r < 1) return 0;
    cx = owner_snap(fx, r), cy = owner_snap(fy, r), cz = owner_snap(fz, r);
    const int lx = cx - (P.origin[0] + (kx << P.cs_shift)), ly = cy - (P.origin[1] + (ky << P.cs_shift)),
              lz = cz - (P.origin[2] + (kz << P.cs_shift));
    if ((unsigned)lx >= (unsigned)P.cs || (unsigned)ly >= (unsigned)P.cs || (unsigned)lz >= (unsigned)P.cs) return 0;
    const int byte = P.voxels[((int64_t)slot << (3 * P.cs_shift)) + voxel_offset(P.cs, lx, ly, lz)];
    return byte == material ? r : 0;
}

// ---------------------------------------------------------------------------------------------
// what every consumer does with a chunk's two offsets (the memory-safety half of the contract, include/vrt.h)
// ---------------------------------------------------------------------------------------------
// The range [lo, hi) of chunk `c`'s list.  `whole`: the lists did not fit (the sentinel) -- the range is every object, and an
// index of the range is the object itself; else an index of the range is a slot of `items`.  Both offsets are clamped to the
// capacity and an inverted pair is empty, so lists that were built for other arrays still index inside `items`.
__device__ static __forceinline__ void lists_range(const ListsView& L, int c, int n_objects, bool& whole, uint32_t& lo, uint32_t& hi) {
    whole = L.offsets[L.n_chunks] == VRT_LISTS_SENTINEL;
    if (whole) {
        lo = 0u, hi = (uint32_t)n_objects;
        return;
    }
    lo = L.offsets[c], hi = L.offsets[c + 1];
    lo = lo < L.cap ? lo : L.cap;
    hi = hi < L.cap ? hi : L.cap;
    hi = hi > lo ? hi : lo;
}

// ---------------------------------------------------------------------------------------------
// the build: count, scan, fill
// ---------------------------------------------------------------------------------------------
// One wave per chunk.  The lanes take the objects 64 at a time, a ballot marks those whose box meets the chunk's, and the
// population count below a lane is its place among them: ascending object index without atomics or a sort, the same bytes at
// every run.  FILL = false counts into offsets[chunk + 1] (lists_scan_kernel sums them in place); FILL = true writes the items.
template <bool FILL>
__global__ void __launch_bounds__(VRT_BLOCK) lists_wave_kernel(const vrt_object* __restrict__ objects, int n_objects, ListsView L,
                                                               uint32_t* __restrict__ offsets, int32_t* __restrict__ items) {
    const int chunk = (int)(((int64_t)blockIdx.x * VRT_BLOCK + threadIdx.x) >> 6), lane = threadIdx.x & 63;
    if (chunk >= L.n_chunks) return;  // (whole waves leave: `chunk` is the same in a wave's lanes)
    uint32_t at = 0;
    if (FILL) {
        if (offsets[L.n_chunks] == VRT_LISTS_SENTINEL) return;  // the lists did not fit: nothing is written
        at = offsets[chunk];
    }
    const int dy = L.dims[1], dz = L.dims[2];
    const int cx = chunk / (dy * dz), cy = (chunk / dz) % dy, cz = chunk % dz;
    const int cs = 1 << L.cs_shift;
    const int x0 = L.origin[0] + (cx << L.cs_shift), y0 = L.origin[1] + (cy << L.cs_shift), z0 = L.origin[2] + (cz << L.cs_shift);
    uint32_t count = 0;
    for (int base = 0; base < n_objects; base += 64) {
        const int k = base + lane;
        bool meet = false;
        if (k < n_objects) {
            const vrt_object& o = objects[k];
            // half-open boxes: [mins, maxs) meets [x0, x0 + cs); an empty box meets nothing
            meet = o.mins[0] < x0 + cs && o.maxs[0] > x0 && o.mins[1] < y0 + cs && o.maxs[1] > y0 && o.mins[2] < z0 + cs && o.maxs[2] > z0 &&
                   o.mins[0] < o.maxs[0] && o.mins[1] < o.maxs[1] && o.mins[2] < o.maxs[2];
        }
        const unsigned long long mask = __ballot(meet);
        if (FILL && meet) {
            const uint32_t slot = at + count + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
            if (slot < L.cap) items[slot] = k;  // (the scan saw the total fit; the guard keeps the write inside whatever happens)
        }
        count += (uint32_t)__popcll(mask);
    }
    if (!FILL && lane == 0) offsets[chunk + 1] = count;
}

// One workgroup sums the counts in place: offsets[c + 1] becomes the sum of the counts of the chunks 0..c, offsets[0] = 0.  The
// running total is 64 bits wide; a total above the capacity sets the two statistics words and the sentinel.  Also clears the
// statistics, so the build needs no other launch.
__global__ void __launch_bounds__(VRT_LISTS_SCAN_BLOCK) lists_scan_kernel(uint32_t* __restrict__ offsets, int n_chunks, uint32_t cap,
                                                                          unsigned long long* __restrict__ stats) {
    __shared__ unsigned long long s_wave[VRT_LISTS_SCAN_BLOCK / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned long long carry = 0;  // the same in every thread
    for (int base = 0; base < n_chunks; base += VRT_LISTS_SCAN_BLOCK * VRT_LISTS_SCAN_PER_THREAD) {
        const int first = base + tid * VRT_LISTS_SCAN_PER_THREAD;
        uint32_t v[VRT_LISTS_SCAN_PER_THREAD];
        unsigned long long mine = 0;
#pragma unroll
        for (int j = 0; j < VRT_LISTS_SCAN_PER_THREAD; j++) {
            v[j] = first + j < n_chunks ? offsets[1 + first + j] : 0u;
            mine += v[j];
        }
        // inclusive sums across the wave, then across the waves
        unsigned long long incl = mine;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned long long up = __shfl_up(incl, d, 64);
            if (lane >= d) incl += up;
        }
        if (lane == 63) s_wave[wave] = incl;
        __syncthreads();
        unsigned long long before = carry, total = 0;
        for (int w = 0; w < VRT_LISTS_SCAN_BLOCK / 64; w++) {
            if (w < wave) before += s_wave[w];
            total += s_wave[w];
        }
        unsigned long long run = before + incl - mine;
#pragma unroll
        for (int j = 0; j < VRT_LISTS_SCAN_PER_THREAD; j++) {
            run += v[j];
            if (first + j < n_chunks) offsets[1 + first + j] = (uint32_t)run;  // (wraps only when the total overflows the capacity)
        }
        carry += total;
        __syncthreads();  // (s_wave is written again)
    }
    if (tid < VRT_NSTATS) stats[tid] = tid == VRT_S_LISTS_ITEMS ? carry : (tid == VRT_S_LISTS_OVERFLOW ? (unsigned long long)(carry > cap) : 0ull);
    if (tid == 0) {
        offsets[0] = 0u;
        if (carry > cap) offsets[n_chunks] = VRT_LISTS_SENTINEL;
    }
}

// ---------------------------------------------------------------------------------------------
// voxelisation from the lists
// ---------------------------------------------------------------------------------------------
// voxelize_kernel with the object loop over the chunk's list only.  One workgroup per chunk; the list's records are staged in
// LDS, VRT_LISTS_TILE at a time, and every voxel asks the records of a tile in list order (the later object wins).  A thread
// walks the block in STORAGE order (vrt_voxel_offset's), so neighbouring lanes write neighbouring bytes; with more than one
// tile a voxel's id so far waits in its own byte of the block, which only its own thread touches.  An item outside
// [0, n_objects) becomes a record of zeros, whose empty box holds no voxel.
__global__ void __launch_bounds__(VRT_BLOCK) voxelize_lists_kernel(const vrt_object* __restrict__ objects, int n_objects,
                                                                   const uint8_t* __restrict__ models, const uint8_t* __restrict__ remap,
                                                                   ListsView L, const uint32_t* __restrict__ chunk_list,
                                                                   uint32_t* __restrict__ table, uint8_t* __restrict__ voxels) {
    __shared__ __attribute__((aligned(16))) vrt_object s_obj[VRT_LISTS_TILE];
    const int chunk = chunk_list ? (int)chunk_list[blockIdx.x] : (int)blockIdx.x;
    if ((unsigned)chunk >= (unsigned)L.n_chunks) return;  // (a chunk list made for another box)
    const int dy = L.dims[1], dz = L.dims[2], cs = 1 << L.cs_shift, nb = cs >> 3, cells = cs * cs * cs;
    const int cx = chunk / (dy * dz), cy = (chunk / dz) % dy, cz = chunk % dz;
    const int wx0 = L.origin[0] + cx * cs, wy0 = L.origin[1] + cy * cs, wz0 = L.origin[2] + cz * cs;
    uint8_t* block = voxels + (int64_t)chunk * cells;
    bool whole;
    uint32_t lo, hi;
    lists_range(L, chunk, n_objects, whole, lo, hi);
    if (lo == hi) {  // nothing meets this chunk: no object is touched (cells is a multiple of 512, the block 16-byte aligned)
        uint4* out = reinterpret_cast<uint4*>(block);
        for (int i = threadIdx.x; i < cells / 16; i += VRT_BLOCK) out[i] = uint4{0u, 0u, 0u, 0u};
        if (threadIdx.x == 0) table[chunk] = 0u;
        return;
    }
    int any = 0;
    for (uint32_t t0 = lo; t0 < hi; t0 += VRT_LISTS_TILE) {
        const int cnt = (int)(hi - t0 < VRT_LISTS_TILE ? hi - t0 : VRT_LISTS_TILE);
        if (t0 != lo) __syncthreads();  // (every thread has finished with the tile before)
        // 64-byte records as four 16-byte words each
        int4* dst = reinterpret_cast<int4*>(s_obj);
        for (int w = threadIdx.x; w < cnt * 4; w += VRT_BLOCK) {
            const int k = whole ? (int)(t0 + (uint32_t)(w >> 2)) : L.items[t0 + (uint32_t)(w >> 2)];
            dst[w] = (unsigned)k < (unsigned)n_objects ? reinterpret_cast<const int4*>(objects + k)[w & 3] : int4{0, 0, 0, 0};
        }
        __syncthreads();
        const bool first = t0 == lo, last = t0 + (uint32_t)cnt == hi;
        for (int i = threadIdx.x; i < cells; i += VRT_BLOCK) {
            // storage offset -> local position (vrt_voxel_offset backwards)
            const int brick = i >> 9, micro = (i >> 6) & 7, vox = i & 63;
            const int lx = ((brick / (nb * nb)) << 3) | ((micro >> 2) << 2) | (vox >> 4);
            const int ly = (((brick / nb) % nb) << 3) | (((micro >> 1) & 1) << 2) | ((vox >> 2) & 3);
            const int lz = ((brick % nb) << 3) | ((micro & 1) << 2) | (vox & 3);
            const int wx = wx0 + lx, wy = wy0 + ly, wz = wz0 + lz;
            int id = first ? 0 : (int)block[i];
            for (int k = 0; k < cnt; k++) {
                int x, y, z;
                const vrt_object& o = s_obj[k];
                const int local = owner_probe(o, models, wx, wy, wz, x, y, z);
                if (local) id = remap[o.remap + local];
            }
            block[i] = (uint8_t)id;
            if (last) any |= id;
        }
    }
    any = __syncthreads_or(any);
    if (threadIdx.x == 0) table[chunk] = any ? ((uint32_t)(chunk + 1) | (1u << 24)) : 0u;
}

// ---------------------------------------------------------------------------------------------
// owner pass from the lists
// ---------------------------------------------------------------------------------------------
// The list of the chunk of the LISTS' box that holds voxel (wx, wy, wz), from its last item to its first; the first object that
// has a voxel there owns it.  A voxel outside that box is in no object of the lists: -2.  Per lane: neighbouring lanes mostly
// share a chunk, but each walks on its own and leaves when it has its answer.
__device__ static __forceinline__ ListsOwnerFound lists_owner_search(const ListsOwnerParams& P, int wx, int wy, int wz, int material) {
    ListsOwnerFound f = {-2, 0, 0, 0};
    const int kx = (wx - P.L.origin[0]) >> P.L.cs_shift, ky = (wy - P.L.origin[1]) >> P.L.cs_shift, kz = (wz - P.L.origin[2]) >> P.L.cs_shift;
    if ((unsigned)kx >= (unsigned)P.L.dims[0] || (unsigned)ky >= (unsigned)P.L.dims[1] || (unsigned)kz >= (unsigned)P.L.dims[2]) return f;
    bool whole;
    uint32_t lo, hi;
    lists_range(P.L, (kx * P.L.dims[1] + ky) * P.L.dims[2] + kz, P.n_objects, whole, lo, hi);
    for (uint32_t j = hi; j > lo; j--) {
        const int k = whole ? (int)(j - 1u) : P.L.items[j - 1u];
        if ((unsigned)k >= (unsigned)P.n_objects) continue;  // (lists of a longer object array)
        const vrt_object& o = P.objects[k];
        int x, y, z;
        const int local = owner_probe(o, P.models, wx, wy, wz, x, y, z);
        if (local) {
            if (P.remap[o.remap + local] == material) f = ListsOwnerFound{k, x, y, z};
            break;
        }
    }
    return f;
}

// owner_kernel with the search above: one lane per record, the candidate rule and the four statistics words unchanged
__global__ void __launch_bounds__(VRT_BLOCK) owner_lists_kernel(ListsOwnerParams P) {
    const int64_t i = (int64_t)blockIdx.x * VRT_BLOCK + threadIdx.x;
    const bool live = i < P.n;
    int material = 0, fx = 0, fy = 0, fz = 0;
    unsigned low = 0;  // bit a: pos[a] is a whole multiple of chunk_size, so the ray may still have stood in the chunk below
    if (live) {
        const vrt_hit& h = P.hits[i];
        material = h.material;
        if (material > 0) {
            fx = h.cell[0], fy = h.cell[1], fz = h.cell[2];
            const int cm = P.cs - 1;
            low = (unsigned)(h.pos[0] == (double)fx && (fx & cm) == 0) | (unsigned)(h.pos[1] == (double)fy && (fy & cm) == 0) << 1 |
                  (unsigned)(h.pos[2] == (double)fz && (fz & cm) == 0) << 2;
        }
    }
    const bool examined = material > 0;
    // the first candidate that counts, in the order 0 (the containing chunk), x, y, xy, z, xz, yz, xyz; `later`: the others that count
    int res = 0, cx = 0, cy = 0, cz = 0;
    unsigned later = 0;
    if (examined) {
        for (int m = 0; m < 8; m++) {
            if (m & ~low) continue;
            int tx, ty, tz;
            const int r = owner_candidate(P, m, fx, fy, fz, material, tx, ty, tz);
            if (!r) continue;
            if (!res) res = r, cx = tx, cy = ty, cz = tz;
            else later |= 1u << m;
        }
    }
    ListsOwnerFound f = {-2, 0, 0, 0};
    if (res) f = lists_owner_search(P, cx, cy, cz, material);
    // two chunks explain this record (rare): the first was taken, and the record is counted if another resolves differently
    bool ambiguous = false;
    if (later) {
        for (int m = 1; m < 8; m++) {
            if (!((later >> m) & 1u)) continue;
            int tx, ty, tz;
            owner_candidate(P, m, fx, fy, fz, material, tx, ty, tz);
            const ListsOwnerFound g = lists_owner_search(P, tx, ty, tz, material);
            ambiguous |= g.object != f.object || g.lx != f.lx || g.ly != f.ly || g.lz != f.lz;
        }
    }
    if (live) {
        int4 a = {-1, 0, 0, 0}, b = {0, 0, 0, 0};
        if (examined) {
            a.x = f.object;
            if (f.object >= 0) a = int4{f.object, res, cx, cy}, b = int4{cz, f.lx, f.ly, f.lz};
        }
        int4* out = reinterpret_cast<int4*>(P.owners + i);
        out[0] = a;
        out[1] = b;
    }
    const unsigned n_exam = (unsigned)__popcll(__ballot(examined)), n_own = (unsigned)__popcll(__ballot(examined && f.object >= 0)),
                   n_amb = (unsigned)__popcll(__ballot(ambiguous));
    if ((threadIdx.x & 63) == 0) {
        if (n_exam) atomicAdd(&P.stats[VRT_S_OWNER_EXAMINED], (unsigned long long)n_exam);
        if (n_own) atomicAdd(&P.stats[VRT_S_OWNER_RESOLVED], (unsigned long long)n_own);
        if (n_exam - n_own) atomicAdd(&P.stats[VRT_S_OWNER_ORPHANS], (unsigned long long)(n_exam - n_own));
        if (n_amb) atomicAdd(&P.stats[VRT_S_OWNER_AMBIGUOUS], (unsigned long long)n_amb);
    }
}

// (the statistics are cleared by a kernel, as everywhere in the library: a captured memset node of so small a buffer was seen
// to replay a stale pattern)
__global__ void __launch_bounds__(64) lists_clear_stats_kernel(unsigned long long* stats) {
    if (threadIdx.x < VRT_NSTATS) stats[threadIdx.x] = 0ull;
}

// ---------------------------------------------------------------------------------------------
// entry points
// ---------------------------------------------------------------------------------------------
// What all three refuse about the lists before any HIP call; fills the kernels' view of them
static bool lists_view(const vrt_chunk_lists* lists, ListsView& V) {
    if (!lists || !lists->d_offsets || ((uintptr_t)lists->d_offsets & 3) != 0 || ((uintptr_t)lists->d_items & 3) != 0) return false;
    const int cs = lists->chunk_size;
    if (cs < 8 || cs > 256 || (cs & (cs - 1))) return false;
    if (lists->n_items_cap < 0 || lists->n_items_cap >= (1ll << 31) || (lists->n_items_cap > 0 && !lists->d_items)) return false;
    int64_t n = 1;
    for (int a = 0; a < 3; a++) {
        if (lists->dims[a] < 1 || n * lists->dims[a] > (1 << 24) - 2) return false;
        n *= lists->dims[a];
        if (lists->origin[a] % cs) return false;
        if (lists->origin[a] < -(1ll << 30) || lists->origin[a] + (int64_t)lists->dims[a] * cs > (1ll << 30)) return false;
        V.origin[a] = (int32_t)lists->origin[a];
        V.dims[a] = lists->dims[a];
    }
    int shift = 0;
    while ((1 << shift) < cs) shift++;
    V.cs_shift = shift;
    V.n_chunks = (int32_t)n;
    V.cap = (uint32_t)lists->n_items_cap;
    V.offsets = lists->d_offsets;
    V.items = lists->d_items;
    return true;
}

extern "C" int vrt_chunk_lists_build(const vrt_object* d_objects, int32_t n_objects, const vrt_chunk_lists* lists, uint64_t* d_stats,
                                     void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    // (every check comes before any HIP call)
    ListsView V;
    if (!lists_view(lists, V) || !d_stats || ((uintptr_t)d_stats & 7) != 0 || n_objects < 0) return VRT_ERR_ARG;
    if (n_objects > 0 && (!d_objects || ((uintptr_t)d_objects & 15) != 0)) return VRT_ERR_ARG;
    const unsigned blocks = (unsigned)(((int64_t)V.n_chunks * 64 + VRT_BLOCK - 1) / VRT_BLOCK);
    hipLaunchKernelGGL(lists_wave_kernel<false>, dim3(blocks), dim3(VRT_BLOCK), 0, stream, d_objects, (int)n_objects, V, lists->d_offsets,
                       lists->d_items);
    hipLaunchKernelGGL(lists_scan_kernel, dim3(1), dim3(VRT_LISTS_SCAN_BLOCK), 0, stream, lists->d_offsets, (int)V.n_chunks, V.cap,
                       (unsigned long long*)d_stats);
    hipLaunchKernelGGL(lists_wave_kernel<true>, dim3(blocks), dim3(VRT_BLOCK), 0, stream, d_objects, (int)n_objects, V, lists->d_offsets,
                       lists->d_items);
    if (hipGetLastError() != hipSuccess) return VRT_ERR_HIP;
    return VRT_OK;
}

extern "C" int vrt_voxelize_lists(const vrt_object* d_objects, int32_t n_objects, const uint8_t* d_models, const uint8_t* d_remap,
                                  const int64_t* origin, const int32_t* dims, int32_t cs, const uint32_t* d_chunk_list, int64_t n_list,
                                  uint32_t* d_world_table, uint8_t* d_voxels, const vrt_chunk_lists* lists, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    // (every check comes before any HIP call: vrt_voxelize's, then the lists')
    if (n_objects < 0 || !origin || !dims || !d_world_table || !d_voxels || ((uintptr_t)d_voxels & 15) != 0) return VRT_ERR_ARG;
    if (n_objects > 0 && (!d_objects || !d_models || !d_remap || ((uintptr_t)d_objects & 15) != 0)) return VRT_ERR_ARG;
    if (cs < 8 || cs > 256 || (cs & (cs - 1))) return VRT_ERR_ARG;
    if (dims[0] < 1 || dims[1] < 1 || dims[2] < 1) return VRT_ERR_ARG;
    const int64_t n = (int64_t)dims[0] * dims[1] * dims[2];
    if (n > (1 << 24) - 2) return VRT_ERR_ARG;
    if (n_list < 0 || n_list > n || (n_list > 0 && !d_chunk_list)) return VRT_ERR_ARG;
    for (int a = 0; a < 3; a++) {
        if (origin[a] % cs) return VRT_ERR_ARG;
        if (origin[a] < -(1ll << 30) || origin[a] + (int64_t)dims[a] * cs > (1ll << 30)) return VRT_ERR_ARG;
    }
    ListsView V;
    if (!lists_view(lists, V) || lists->chunk_size != cs) return VRT_ERR_ARG;
    for (int a = 0; a < 3; a++)
        if (lists->origin[a] != origin[a] || lists->dims[a] != dims[a]) return VRT_ERR_ARG;
    const int64_t blocks = d_chunk_list ? n_list : n;
    if (blocks == 0) return VRT_OK;
    hipLaunchKernelGGL(voxelize_lists_kernel, dim3((unsigned)blocks), dim3(VRT_BLOCK), 0, stream, d_objects, (int)n_objects, d_models,
                       d_remap, V, d_chunk_list, d_world_table, d_voxels);
    if (hipGetLastError() != hipSuccess) return VRT_ERR_HIP;
    return VRT_OK;
}

extern "C" int vrt_hit_owners_lists(const vrt_scene* sc, const vrt_hit* d_hits, int64_t n_hits, const vrt_object* d_objects,
                                    int32_t n_objects, const uint8_t* d_models, const uint8_t* d_remap, vrt_owner* d_owners,
                                    const vrt_chunk_lists* lists, uint64_t* d_stats, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    // (every check comes before any HIP call: vrt_hit_owners', then the lists')
    if (!sc || !d_stats || n_hits < 0 || n_hits >= (1ll << 32) || n_objects < 0) return VRT_ERR_ARG;
    if (n_hits > 0 && (!d_hits || !d_owners || ((uintptr_t)d_hits & 7) != 0 || ((uintptr_t)d_owners & 15) != 0)) return VRT_ERR_ARG;
    if (n_objects > 0 && (!d_objects || !d_models || !d_remap || ((uintptr_t)d_objects & 15) != 0)) return VRT_ERR_ARG;
    const int cs = sc->chunk_size;
    if (cs < 8 || cs > 256 || (cs & (cs - 1))) return VRT_ERR_ARG;
    if (!sc->d_chunk_table || sc->n_slots < 0 || sc->n_slots >= (1 << 24) || (sc->n_slots > 0 && !sc->d_voxels)) return VRT_ERR_ARG;
    ListsOwnerParams P;
    int64_t cells = 1;
    for (int a = 0; a < 3; a++) {
        if (sc->dims[a] <= 0 || (sc->origin[a] % cs) != 0) return VRT_ERR_ARG;
        if (sc->origin[a] < -(1ll << 28) || sc->origin[a] + (int64_t)sc->dims[a] * cs > (1ll << 28)) return VRT_ERR_ARG;
        P.origin[a] = (int32_t)sc->origin[a];
        P.dims[a] = sc->dims[a];
        cells *= sc->dims[a];
    }
    if (cells >= (1ll << 31)) return VRT_ERR_ARG;
    if (!lists_view(lists, P.L)) return VRT_ERR_ARG;
    int shift = 0;
    while ((1 << shift) < cs) shift++;
    P.cs = cs;
    P.cs_shift = shift;
    P.n_slots = sc->n_slots;
    P.table = sc->d_chunk_table;
    P.voxels = sc->d_voxels;
    P.objects = d_objects;
    P.n_objects = n_objects;
    P.models = d_models;
    P.remap = d_remap;
    P.stats = (unsigned long long*)d_stats;
    hipLaunchKernelGGL(lists_clear_stats_kernel, dim3(1), dim3(64), 0, stream, (unsigned long long*)d_stats);
    const int64_t per_launch = 1ll << 28;
    for (int64_t r0 = 0; r0 < n_hits; r0 += per_launch) {
        P.n = n_hits - r0 < per_launch ? n_hits - r0 : per_launch;
        P.hits = d_hits + r0;
        P.owners = d_owners + r0;
        hipLaunchKernelGGL(owner_lists_kernel, dim3((unsigned)((P.n + VRT_BLOCK - 1) / VRT_BLOCK)), dim3(VRT_BLOCK), 0, stream, P);
    }
    if (hipGetLastError() != hipSuccess) return VRT_ERR_HIP;
    return VRT_OK;
}
