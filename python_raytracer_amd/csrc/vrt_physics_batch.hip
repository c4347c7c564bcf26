// vrt_physics_batch.hip -- MI355X (gfx950) object physics, many runs in one launch (vrt_physics_run_batch, include/vrt.h):
// `n_runs` what-if copies of one world's bodies, each stepped for `n_ticks` ticks as vrt_physics_run steps its own, bit for bit.
//
// A run is a sequential chain and takes one workgroup of 1024 threads; runs have nothing to say to each other, so a batch is a
// grid of `n_runs` such workgroups: workgroup r owns bodies [r * n, (r + 1) * n), its row of the trace, its statistics block and
// its word of d_ticks_done, and shares the models, the remap table and the material rows, which nothing writes.
//
// A translation unit and a kernel of its own, linked into the same library and built with the same flags as the other physics
// units, whose kernels and resource reports stay as they are.  The tick is vrt_physics_run.hip's, RESTATED below statement for
// statement rather than shared, so that no existing kernel's figures can move; what the units do share lives in
// vrt_physics_common.h.  tests/test_gpu_physics_batch.py holds every run of a batch to vrt_physics_run on a twin.
//
// Workgroup barriers only: no grid barrier, no cooperative launch, no atomics on memory another workgroup reads, nothing waits on
// memory.  The launch is bounded on any input: every workgroup counts its own WORK as vrt_physics_run does and stops at the first
// tick boundary at or past the budget; how far it got goes into d_ticks_done[r], and the next launch goes on from there.
//
// Arithmetic is binary64 in the reference's evaluation order; build with -ffp-contract=off.
// gfx950 only: 64-wide waves are assumed.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/vrt.h"
#include "vrt_math.h"

#pragma clang fp contract(off)

#include "vrt_physics_common.h"

static_assert(sizeof(vrt_body_sample) == 104 && alignof(vrt_body_sample) == 8 && sizeof(vrt_physics_run_params) == 80,
              "record sizes of include/vrt.h");

__global__ void __launch_bounds__(VRT_PHYS_BLOCK) physics_batch_kernel(PhysParams P, vrt_physics_run_params R, int32_t* ticks_done,
                                                                       vrt_body_sample* trace) {
    __shared__ PhysSelf S;
    __shared__ vrt_object s_self;
    __shared__ int s_cand[VRT_PHYS_BLOCK];
    __shared__ double s_terms[VRT_PHYS_BLOCK][2];
    __shared__ int s_wave[VRT_PHYS_WAVES];
    __shared__ unsigned s_refused;
    const int tid = threadIdx.x;
    // ---- this workgroup's run: its bodies, its statistics, its rows of the trace, its word of ticks_done
    const int64_t run = blockIdx.x;
    P.bodies += run * P.n;
    P.stats += run * VRT_NSTATS;
    if (trace) trace += run * R.n_ticks * P.n;
    const int start = ticks_done[run];  // (uniform: every lane reads it before lane 0 may write it, below a barrier)
    if (tid < VRT_NSTATS) P.stats[tid] = 0ull;
    if (tid == 0) s_refused = 0u;
    __syncthreads();
    if (start < 0 || start > R.n_ticks) {  // device data: the run counts as done, nothing of it is touched
        if (tid == 0) P.stats[VRT_S_PHYSICS_BATCH_BADTICK] = 1ull;
        return;
    }
    if (start == R.n_ticks) return;  // done by an earlier launch: TICKS = 0
    if (P.n == 0) {  // nothing to do: every tick is done
        if (tid == 0) P.stats[VRT_S_PHYSICS_TICKS] = (unsigned long long)(R.n_ticks - start), ticks_done[run] = R.n_ticks;
        return;
    }
    unsigned long long n_bodies = 0, n_steps = 0, n_blocked = 0, n_contacts = 0, n_transfers = 0, n_capped = 0;  // lane 0's
    unsigned long long work = 0;  // every lane's, and the same in all of them
    const unsigned long long tiles = ((unsigned long long)P.n + VRT_PHYS_BLOCK - 1) / VRT_PHYS_BLOCK;
    int tick = start;  // absolute: the trace is indexed by it
    for (;;) {
        // ---- the camera of this tick: on the followed body as it stands now, unless this tick refuses it
        double cam[3] = {R.cam[0], R.cam[1], R.cam[2]};
        if (R.follow >= 0) {
            const vrt_body& f = P.bodies[R.follow];
            if (physics_valid(P, f)) {
#pragma unroll
                for (int a = 0; a < 3; a++) cam[a] = f.pos[a] + R.offset[a];
            }
        }
        // ---- flags and validation, before the first body moves: a refused body is met by none
        for (int j = tid; j < P.n; j += VRT_PHYS_BLOCK) {
            vrt_body& b = P.bodies[j];
            const bool good = physics_valid(P, b);
            const double dist = vrt_dist3(b.pos[0] - cam[0], b.pos[1] - cam[1], b.pos[2] - cam[2]);
            const int big = b.half[0] > b.half[1] ? (b.half[0] > b.half[2] ? b.half[0] : b.half[2]) : (b.half[1] > b.half[2] ? b.half[1] : b.half[2]);
            const int before = b.visible_now != 0;
            const int now = b.has_sprite && dist <= R.dist_max + (double)big;
            b.visible_before = before, b.visible_now = now, b.awake = dist <= R.dist_move;
            if (before != now) b.pad[0] |= 2;
            b.steps = b.blocked_steps = b.contacts = b.transfers = b.moved = 0;
            b.status = good ? 0 : VRT_BODY_REFUSED;
            if (!good) atomicAdd(&s_refused, 1u);
        }
        work += tiles;
        // ---- the tick: vrt_physics.hip's walk, restated
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
            work += 1;
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
                work += 1;
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
                    work += 1;
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
                    work += (unsigned long long)((total + VRT_PHYS_BLOCK - 1) / VRT_PHYS_BLOCK);
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
                if (S.moved) b.pad[0] |= 1;
                n_bodies++, n_steps += S.steps, n_blocked += S.blocked_steps, n_contacts += S.contacts, n_transfers += S.transfers;
            }
        }
        __syncthreads();  // the last body is back: the records are the tick's
        tick++;
        if (trace) {
            vrt_body_sample* row = trace + (int64_t)(tick - 1) * P.n;
            for (int j = tid; j < P.n; j += VRT_PHYS_BLOCK) {
                const vrt_body& b = P.bodies[j];
                vrt_body_sample& s = row[j];
#pragma unroll
                for (int a = 0; a < 3; a++) {
                    s.pos[a] = b.pos[a], s.vel[a] = b.vel[a];
                    s.mins[a] = b.object.mins[a], s.maxs[a] = b.object.maxs[a];
                }
                s.visible = b.visible_now, s.awake = b.awake;
                s.out[0] = b.steps, s.out[1] = b.blocked_steps, s.out[2] = b.contacts, s.out[3] = b.transfers;
                s.out[4] = b.moved, s.out[5] = b.status;
            }
        }
        if (tick >= R.n_ticks || work >= (unsigned long long)R.budget) break;  // (uniform: every lane counted the same)
    }
    if (tid == 0) {
        P.stats[VRT_S_PHYSICS_BODIES] = n_bodies, P.stats[VRT_S_PHYSICS_REFUSED] = s_refused, P.stats[VRT_S_PHYSICS_STEPS] = n_steps;
        P.stats[VRT_S_PHYSICS_BLOCKED] = n_blocked, P.stats[VRT_S_PHYSICS_CONTACTS] = n_contacts;
        P.stats[VRT_S_PHYSICS_TRANSFERS] = n_transfers, P.stats[VRT_S_PHYSICS_CAPPED] = n_capped;
        P.stats[VRT_S_PHYSICS_WORK] = work, P.stats[VRT_S_PHYSICS_TICKS] = (unsigned long long)(tick - start);
        ticks_done[run] = tick;
    }
}

extern "C" int vrt_physics_run_batch(vrt_body* d_bodies, int32_t n_runs, int32_t n_bodies, const uint8_t* d_models, int64_t models_bytes,
                                     const uint8_t* d_remap, int32_t remap_bytes, const double* d_matphys, int32_t n_materials,
                                     const vrt_physics_params* params, const vrt_physics_run_params* run, int32_t* d_ticks_done,
                                     vrt_body_sample* d_trace, uint64_t* d_stats, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    // (every check comes before any HIP call)
    if (!physics_args_ok(d_bodies, n_bodies, d_models, models_bytes, d_remap, remap_bytes, d_matphys, n_materials, params, d_stats))
        return VRT_ERR_ARG;
    if (!run || run->n_ticks < 1 || run->budget < 1 || run->follow < -1 || run->follow >= n_bodies) return VRT_ERR_ARG;
    const double v[8] = {run->cam[0], run->cam[1], run->cam[2], run->offset[0], run->offset[1], run->offset[2], run->dist_max, run->dist_move};
    for (int a = 0; a < 8; a++)
        if (!(__builtin_fabs(v[a]) < __builtin_inf())) return VRT_ERR_ARG;
    if (((uintptr_t)d_trace & 7) != 0) return VRT_ERR_ARG;
    if (n_runs < 1 || n_runs > VRT_PHYSICS_BATCH_MAX_RUNS || (int64_t)n_runs * n_bodies > (1 << 20)) return VRT_ERR_ARG;
    if (!d_ticks_done || ((uintptr_t)d_ticks_done & 3) != 0) return VRT_ERR_ARG;
    PhysParams P;
    P.bodies = d_bodies, P.models = d_models, P.remap = d_remap, P.matphys = d_matphys;
    P.stats = (unsigned long long*)d_stats;
    P.models_bytes = models_bytes;
    P.n = n_bodies, P.remap_bytes = remap_bytes, P.n_materials = n_materials;
    P.p = *params;
    // one workgroup per run, and none of them waits for another
    hipLaunchKernelGGL(physics_batch_kernel, dim3(n_runs), dim3(VRT_PHYS_BLOCK), 0, stream, P, *run, d_ticks_done, d_trace);
    if (hipGetLastError() != hipSuccess) return VRT_ERR_HIP;
    return VRT_OK;
}
