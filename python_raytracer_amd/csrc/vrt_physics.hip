// vrt_physics.hip -- MI355X (gfx950) object physics (vrt_physics_tick, include/vrt.h): one tick of the reference's
// `for obj in objects: obj.update(cam_pos)` (init.py:469-470) with Object.update_physics (data.py:495-560) on the resident models.
//
// A translation unit of its own, linked into the same library as vrt_kernels.hip and built with the same flags.  It shares no code
// with that file: the quarter-turn addressing of the object voxel lookup (rotate_index next to voxelize_kernel) is restated in
// vrt_physics_common.h, which this unit shares with vrt_physics_draws.hip (the tick that makes the reference's random draws),
// and tests/test_gpu_physics.py holds the restatement to vrt_voxelize.
//
// The tick is a sequential chain -- body k meets what bodies 0..k-1 have just done, and a body's steps follow each other -- so
// the launch is ONE workgroup that walks the bodies in order and meets at workgroup barriers only.  There is no grid-wide
// barrier, no cooperative launch and no waiting on memory: nothing here can wait for another workgroup.  The width goes to the
// inside of a step: (bodies whose box meets the slab) x (slab voxels), 1024 tests at a time.  The friction and elasticity sums
// are the reference's bit for bit: contacts are compacted in its order (bodies -> x -> y -> z) and one lane adds them, so the
// path is latency-bound by construction.
//
// Arithmetic is binary64 in the reference's evaluation order; build with -ffp-contract=off.
// gfx950 only: 64-wide waves are assumed.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/vrt.h"

#pragma clang fp contract(off)

#include "vrt_physics_common.h"

__global__ void __launch_bounds__(VRT_PHYS_BLOCK) physics_kernel(PhysParams P) {
    __shared__ PhysSelf S;
    __shared__ vrt_object s_self;
    __shared__ int s_cand[VRT_PHYS_BLOCK];
    __shared__ double s_terms[VRT_PHYS_BLOCK][2];
    __shared__ int s_wave[VRT_PHYS_WAVES];
    __shared__ unsigned s_refused;
    const int tid = threadIdx.x;
    if (tid < VRT_NSTATS) P.stats[tid] = 0ull;
    if (tid == 0) s_refused = 0u;
    __syncthreads();
    // ---- every body is validated before the first moves: a refused body is met by none
    for (int j = tid; j < P.n; j += VRT_PHYS_BLOCK) {
        vrt_body& b = P.bodies[j];
        const bool good = physics_valid(P, b);
        b.steps = b.blocked_steps = b.contacts = b.transfers = b.moved = 0;
        b.status = good ? 0 : VRT_BODY_REFUSED;
        if (!good) atomicAdd(&s_refused, 1u);
    }
    unsigned long long n_bodies = 0, n_steps = 0, n_blocked = 0, n_contacts = 0, n_transfers = 0, n_capped = 0;  // lane 0's
    for (int k = 0; k < P.n; k++) {
        __syncthreads();  // what the body before wrote -- boxes, velocities handed on -- is there
        if (tid == 0) {
            const vrt_body& b = P.bodies[k];
            S.run = b.status == 0 && b.visible_now && b.awake && b.physics && b.has_sprite;
            if (S.run) {
#pragma unroll
                for (int a = 0; a < 3; a++) {
                    S.pos[a] = b.pos[a], S.vel[a] = b.vel[a], S.va[a] = b.vel[a];
                    S.mins[a] = b.object.mins[a], S.maxs[a] = b.object.maxs[a], S.half[a] = b.half[a];
                }
                S.weight = b.weight, S.friction = 0.0, S.elasticity = 0.0;
                S.steps = S.blocked_steps = S.contacts = S.transfers = S.moved = 0;
                s_self = b.object, S.rim = b.rim;
            } else if (b.status == 0) {
                P.bodies[k].status = VRT_BODY_SKIPPED;
            }
        }
        __syncthreads();
        if (!S.run) continue;
        for (int iter = 0;; iter++) {
            if (tid == 0) {
                const double ref = __builtin_fmax(__builtin_fabs(S.va[0]), __builtin_fmax(__builtin_fabs(S.va[1]), __builtin_fabs(S.va[2])));
                S.done = ref == 0.0 || iter >= VRT_PHYSICS_STEP_CAP;
                if (ref != 0.0 && iter >= VRT_PHYSICS_STEP_CAP) n_capped++;
                if (!S.done) {
                    // vel_dir = trunc(normalize(vel_apply)): +-1 on every axis that ties for the largest magnitude (x / x is 1)
#pragma unroll
                    for (int a = 0; a < 3; a++) {
                        const double nv = (ref != 1.0) ? S.va[a] / ref : S.va[a];
                        S.dir[a] = (nv >= 1.0) - (nv <= -1.0);
                        S.lo[a] = S.mins[a], S.ext[a] = S.maxs[a] - S.mins[a] + 1;
                    }
                    // the slab is chosen by the first axis that moves, the move is along all of vel_dir
                    const int axis = S.dir[0] ? 0 : (S.dir[1] ? 1 : 2);
                    S.lo[axis] = S.dir[axis] < 0 ? S.mins[axis] - 1 : S.maxs[axis];
                    S.ext[axis] = 2;
                    S.blocked = 0;
                }
            }
            __syncthreads();
            if (S.done) break;
            const int lo[3] = {S.lo[0], S.lo[1], S.lo[2]}, ext[3] = {S.ext[0], S.ext[1], S.ext[2]};
            const int dir[3] = {S.dir[0], S.dir[1], S.dir[2]};
            const int smin[3] = {S.mins[0], S.mins[1], S.mins[2]};
            const int64_t srim = S.rim;
            const int64_t slab = (int64_t)ext[0] * ext[1] * ext[2];
            for (int base = 0; base < P.n; base += VRT_PHYS_BLOCK) {
                // 1. the bodies this step meets, in array order (data.py:520-521)
                const int j = base + tid;
                bool meet = false;
                if (j < P.n && j != k) {
                    const vrt_body& b = P.bodies[j];
                    meet = b.status != VRT_BODY_REFUSED && b.has_sprite && (j < k ? b.visible_now : b.visible_before);
#pragma unroll
                    for (int a = 0; a < 3; a++) meet = meet && lo[a] <= b.object.maxs[a] && lo[a] + ext[a] - 1 >= b.object.mins[a];
                }
                const int n_cand = __syncthreads_count(meet);
                if (n_cand == 0) continue;
                const int slot = physics_slot(meet, s_wave);
                if (meet) s_cand[slot] = j;
                __syncthreads();
                // 2. velocity transfers to the physical ones among them, in order, contact or not (data.py:523-527)
                if (tid == 0) {
                    for (int c = 0; c < n_cand; c++) {
                        vrt_body& b = P.bodies[s_cand[c]];
                        if (!b.physics) continue;
                        const double m = __builtin_fmax(__builtin_fabs(S.va[0]), __builtin_fmax(__builtin_fabs(S.va[1]), __builtin_fabs(S.va[2])));
                        const double t = m * S.weight - b.weight;
                        double f = t < 1.0 ? t : 1.0;  // max(0, min(1, t)) as Python evaluates it
                        f = f > 0.0 ? f : 0.0;
#pragma unroll
                        for (int a = 0; a < 3; a++) {
                            const double vt = S.va[a] * f;
                            b.vel[a] = b.vel[a] + vt;
                            S.vel[a] = S.vel[a] - vt;
                            S.va[a] = S.va[a] - vt;
                        }
                        S.transfers++;
                    }
                }
                // 3. slab voxel x body, in the reference's order: bodies -> x -> y -> z (data.py:532-542)
                const int64_t total = (int64_t)n_cand * slab;
                for (int64_t first = 0; first < total; first += VRT_PHYS_BLOCK) {
                    const int64_t idx = first + tid;
                    bool contact = false;
                    double tf = 0.0, te = 0.0;
                    if (idx < total) {
                        const int c = (int)(idx / slab);
                        const int v = (int)(idx - (int64_t)c * slab);
                        const int zi = v % ext[2], yi = (v / ext[2]) % ext[1], xi = v / (ext[2] * ext[1]);
                        const int wx = lo[0] + xi, wy = lo[1] + yi, wz = lo[2] + zi;
                        const vrt_body& other = P.bodies[s_cand[c]];
                        const vrt_object& o = other.object;
                        const int g = physics_material(P, o, other.rim, wx - o.mins[0], wy - o.mins[1], wz - o.mins[2]);
                        if (g && P.matphys[g * 4] >= 1.0) {
                            const int h = physics_material(P, s_self, srim, wx - smin[0] - dir[0], wy - smin[1] - dir[1], wz - smin[2] - dir[2]);
                            if (h && P.matphys[h * 4] >= 1.0) {
                                contact = true;
                                tf = P.matphys[g * 4 + 1] * P.matphys[h * 4 + 1] * P.p.friction;
                                te = P.matphys[g * 4 + 2] * P.matphys[h * 4 + 2] * P.p.friction;
                            }
                        }
                    }
                    // 4. the contacts of this pass, compacted in order; one lane adds them as the reference does
                    const int n_hit = __syncthreads_count(contact);
                    if (n_hit == 0) continue;
                    const int at = physics_slot(contact, s_wave);
                    if (contact) s_terms[at][0] = tf, s_terms[at][1] = te;
                    __syncthreads();
                    if (tid == 0) {
                        double fr = S.friction, el = S.elasticity;
                        for (int i = 0; i < n_hit; i++) fr = fr + s_terms[i][0], el = el + s_terms[i][1];
                        S.friction = fr, S.elasticity = el;
                        S.blocked = 1;
                        S.contacts += n_hit;
                    }
                }
            }
            // the move (data.py:545-548): a blocked direction loses all its velocity, a free one moves by at most one unit
            if (tid == 0) {
                double to[3];
                bool changed = false;
#pragma unroll
                for (int a = 0; a < 3; a++) {
                    const double mag = __builtin_fabs(S.va[a]);
                    const double step = (double)dir[a] * (S.blocked ? mag : (1.0 < mag ? 1.0 : mag));
                    S.va[a] = S.va[a] - step;
                    to[a] = S.pos[a] + step;
                    changed = changed || to[a] != S.pos[a];
                }
                S.steps++;
                if (S.blocked) {
                    S.blocked_steps++;
                } else if (changed) {  // Object.move (data.py:482-488)
#pragma unroll
                    for (int a = 0; a < 3; a++) {
                        S.pos[a] = to[a];
                        S.mins[a] = physics_ceil(to[a]) - S.half[a];
                        S.maxs[a] = physics_floor(to[a]) + S.half[a];
                    }
                    S.moved = 1;
                }
            }
        }
        // gravity, elasticity, friction, the terminal and the minimum velocity (data.py:551-560), then the body goes back
        if (tid == 0) {
            vrt_body& b = P.bodies[k];
            double v[3] = {S.vel[0] - 0.0, S.vel[1] - S.weight * P.p.gravity, S.vel[2] - 0.0};
            const double sum = S.friction + P.p.friction_air;
            const double den = 1.0 + (sum > 0.0 ? sum : 0.0);
#pragma unroll
            for (int a = 0; a < 3; a++) {
                double r = v[a] - v[a] * S.elasticity;
                r = r / den;
                r = P.p.max_velocity < r ? P.p.max_velocity : r;
                r = -P.p.max_velocity > r ? -P.p.max_velocity : r;
                if (__builtin_fabs(r) < P.p.min_velocity) r = 0.0;
                b.vel[a] = r;
                b.pos[a] = S.pos[a];
                b.object.mins[a] = S.mins[a], b.object.maxs[a] = S.maxs[a];
            }
            b.steps = S.steps, b.blocked_steps = S.blocked_steps, b.contacts = S.contacts, b.transfers = S.transfers, b.moved = S.moved;
            n_bodies++, n_steps += S.steps, n_blocked += S.blocked_steps, n_contacts += S.contacts, n_transfers += S.transfers;
        }
    }
    __syncthreads();
    if (tid == 0) {
        P.stats[VRT_S_PHYSICS_BODIES] = n_bodies, P.stats[VRT_S_PHYSICS_REFUSED] = s_refused, P.stats[VRT_S_PHYSICS_STEPS] = n_steps;
        P.stats[VRT_S_PHYSICS_BLOCKED] = n_blocked, P.stats[VRT_S_PHYSICS_CONTACTS] = n_contacts;
        P.stats[VRT_S_PHYSICS_TRANSFERS] = n_transfers, P.stats[VRT_S_PHYSICS_CAPPED] = n_capped;
    }
}

extern "C" int vrt_physics_tick(vrt_body* d_bodies, int32_t n_bodies, const uint8_t* d_models, int64_t models_bytes, const uint8_t* d_remap,
                                int32_t remap_bytes, const double* d_matphys, int32_t n_materials, const vrt_physics_params* params,
                                uint64_t* d_stats, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    // (every check comes before any HIP call)
    if (!physics_args_ok(d_bodies, n_bodies, d_models, models_bytes, d_remap, remap_bytes, d_matphys, n_materials, params, d_stats))
        return VRT_ERR_ARG;
    PhysParams P;
    P.bodies = d_bodies, P.models = d_models, P.remap = d_remap, P.matphys = d_matphys;
    P.stats = (unsigned long long*)d_stats;
    P.models_bytes = models_bytes;
    P.n = n_bodies, P.remap_bytes = remap_bytes, P.n_materials = n_materials;
    P.p = *params;
    // one workgroup: the chain is sequential, and a tick that waited on another workgroup could hang
    hipLaunchKernelGGL(physics_kernel, dim3(1), dim3(VRT_PHYS_BLOCK), 0, stream, P);
    if (hipGetLastError() != hipSuccess) return VRT_ERR_HIP;
    return VRT_OK;
}
