// vrt_physics_impulses.hip -- MI355X (gfx950) object physics, many runs in one launch WITH scripted accelerations per run
// (vrt_physics_run_batch_impulses, include/vrt.h): `n_runs` what-if copies of one world's bodies, each stepped for `n_ticks` ticks
// as vrt_physics_run_batch_contacts steps its own, bit for bit, and before each tick the run's impulses of that tick added to the
// velocities of their bodies -- Object.accelerate (data.py:491-492) between two ticks, as the reference's window calls it.
//
// Two kernels in two instances each (template <bool LOG>: with the contact log, or with every statement of the log compiled
// out -- the entry point chooses by a NULL log, which is a uniform test for the whole grid).  Their ticks are
// physics_contacts_kernel's and physics_contacts_draws_kernel's (vrt_physics_contacts.hip), RESTATED below statement for
// statement rather than shared, so that no existing kernel's figures can move: what the units share lives in
// vrt_physics_common.h and vrt_physics_contacts.h, which stay as they are.  The ownership is the batch's: workgroup r owns
// bodies [r * n, (r + 1) * n), its rows of the trace, its statistics block, its word of d_ticks_done, with draws its generator
// and its row of d_tick_draws, with a log its records and its count -- and here entries [d_first[r], d_first[r + 1]) of the list.
//
// The impulse block stands at the top of the tick loop, before the camera of the tick.  The list is DEVICE DATA and nothing of
// it is trusted.  Entry i of a run belongs to tick E[i] = the largest tick in [0, n_ticks) among entries 0..i of the run (0 if
// there is none): a non-decreasing number, so the entries of a tick are contiguous, every entry belongs to exactly one tick, and
// a launch that starts at tick s finds its place -- the first entry with a tick in [s, n_ticks) -- from s alone.  Of the entries
// that belong to tick t, those are APPLIED whose tick is t, whose body is in [0, n), is no lower than the body of any such entry
// before it in the tick, and whose three components are finite; every other one is counted as skipped.  All 1024 lanes take the
// tick's entries 1024 at a time; the lane whose entry is the first of its body in the tile adds it and goes on alone through
// the tile's following entries of the same body, so equal bodies add in list order and different bodies in parallel, with
// plain vector loads and stores and no atomics.  The state -- the place in the list, the run's upper bound, the two counts --
// lives in LDS words that lane 0 writes: nothing of it stays in a register across the tick (the drawing kernel has none to
// spare).  WORK grows by one unit per tile of entries taken and by nothing in a tick without entries, so a run with an empty
// list stops at the tick boundaries of the restated kernel, reports its words and leaves its bytes.
//
// Workgroup barriers only: no grid barrier, no cooperative launch, no atomics on memory another workgroup reads, nothing waits on
// memory.  Everything written to memory is written with vector stores from plain C++.
//
// Arithmetic is binary64 in the reference's evaluation order; build with -ffp-contract=off.
// gfx950 only: 64-wide waves are assumed.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/vrt.h"
#include "vrt_math.h"

#pragma clang fp contract(off)

#include "vrt_physics_common.h"
#include "vrt_physics_contacts.h"

static_assert(sizeof(vrt_body_sample) == 104 && alignof(vrt_body_sample) == 8 && sizeof(vrt_physics_run_params) == 80,
              "record sizes of include/vrt.h");
static_assert(sizeof(vrt_impulse) == 32 && alignof(vrt_impulse) == 8 && sizeof(vrt_impulse_list) == 24, "record sizes of include/vrt.h");

// the list as the kernels get it: all runs' entries, the rows' bounds and the number of entries the host vouches for
struct ImpulseList {
    const vrt_impulse* entries;  // [total], or NULL with total == 0
    const int32_t* first;        // [n_runs + 1]
    int32_t total;
};

// a run's place in its list; lane 0 writes it, every lane reads it after a barrier
struct ImpulseState {
    int32_t at, hi;                        // the next entry no tick has taken yet, and the end of the run's entries
    unsigned long long applied, skipped;   // lane 0's
};

__device__ __forceinline__ bool impulse_finite(const double* v) {
    // (a NaN fails the comparison)
    return __builtin_fabs(v[0]) < __builtin_inf() && __builtin_fabs(v[1]) < __builtin_inf() && __builtin_fabs(v[2]) < __builtin_inf();
}

// How many lanes, in thread order, come before the first lane whose `stop` is set: 1024 if there is none.  The same in all
// lanes.  s_wave: one word per wave.  Two barriers, the first before s_wave is written.
__device__ __forceinline__ int impulses_before(bool stop, int* s_wave) {
    const unsigned long long mask = __ballot(stop);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) s_wave[wave] = mask ? (int)__builtin_ctzll(mask) : 64;
    __syncthreads();
    int n = 0;
    for (int w = 0; w < VRT_PHYS_WAVES; w++) {
        const int f = s_wave[w];
        n += f;
        if (f < 64) break;
    }
    return n;
}

// When a launch starts on a run: its bounds from d_first, checked (a row that decreases or leaves [0, total] empties the list;
// the launch that starts the run counts it once), and its place: the first entry whose tick lies in [start, n_ticks).  Every lane
// calls it; Q is ready after it returns.
__device__ __forceinline__ void impulses_seek(const ImpulseList& I, int64_t run, int start, int n_ticks, ImpulseState& Q, int* s_wave) {
    const int tid = threadIdx.x;
    if (tid == 0) {
        int lo = I.first[run], hi = I.first[run + 1];
        unsigned long long bad = 0ull;
        if (lo < 0 || hi < lo || hi > I.total) lo = hi = 0, bad = start == 0 ? 1ull : 0ull;
        Q.at = lo, Q.hi = hi, Q.applied = 0ull, Q.skipped = bad;
    }
    __syncthreads();
    if (start == 0) return;  // (uniform) the list begins where the run does
    const int hi = Q.hi;
    int c = Q.at;
    while (c < hi) {  // (uniform)
        const int i = c + tid;
        bool stop = false;
        if (i < hi) {
            const int t = I.entries[i].tick;
            stop = t >= start && t < n_ticks;
        }
        const int n = impulses_before(stop, s_wave);
        c = n < hi - c ? c + n : hi;
        if (n < VRT_PHYS_BLOCK) break;
    }
    __syncthreads();  // every lane has read the place
    if (tid == 0) Q.at = c;
    __syncthreads();
}

// The impulses of tick `tick`, before its camera.  Every lane calls it.  Without entries left: no barrier and no work.
// Otherwise the entries that belong to the tick are taken a tile at a time; the first barrier of a tile comes before any
// velocity is written (the trace of the tick before has been read by then), the last after all of them.  s_wave, s_max: one word
// per wave each.
__device__ __forceinline__ void impulses_tick(const ImpulseList& I, const PhysParams& P, int tick, int n_ticks, ImpulseState& Q, int* s_wave,
                                              int* s_max, unsigned long long& work) {
    const int tid = threadIdx.x;
    const int hi = Q.hi;
    int c = Q.at;
    if (c >= hi) return;  // (uniform)
    const int lane = tid & 63, wave = tid >> 6;
    int carry = -1;  // the highest body of the tick's earlier tiles (uniform)
    unsigned taken = 0, applied = 0;
    for (;;) {
        const int i = c + tid;
        int t = -1, body = -1;
        bool stop = true;  // (past the run's end)
        if (i < hi) {
            t = I.entries[i].tick, body = I.entries[i].body;
            stop = t > tick && t < n_ticks;  // a later tick's: the tick's entries end before it
        }
        const int n = impulses_before(stop, s_wave);
        if (n == 0) break;
        work += 1;
        // the body of an entry of this tick, -1 for every other; its highest among the lanes before this one
        const int key = (tid < n && t == tick && body >= 0 && body < P.n) ? body : -1;
        int upto = key;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int o = __shfl_up(upto, d);
            if (lane >= d && o > upto) upto = o;
        }
        int below = __shfl_up(upto, 1);
        if (lane == 0) below = -1;
        if (lane == 63) s_max[wave] = upto;
        __syncthreads();
        int top = -1;
        for (int w = 0; w < VRT_PHYS_WAVES; w++) {
            const int m = s_max[w];
            if (w < wave && m > below) below = m;
            if (m > top) top = m;
        }
        // in order: no lower than any body before it in the tick.  The first of its body in the tile adds, and goes on alone
        const bool ordered = key >= 0 && key >= below && key >= carry;
        double v[3] = {0.0, 0.0, 0.0};
        if (ordered) v[0] = I.entries[i].vel[0], v[1] = I.entries[i].vel[1], v[2] = I.entries[i].vel[2];
        const bool good = ordered && impulse_finite(v);
        if (ordered && key > below) {
            vrt_body& b = P.bodies[key];
            double to[3] = {b.vel[0], b.vel[1], b.vel[2]};
            if (good) {
#pragma unroll
                for (int a = 0; a < 3; a++) to[a] = to[a] + v[a];
            }
            for (int j = i + 1; j < c + n; j++) {
                const vrt_impulse& e = I.entries[j];
                if (e.tick != tick) continue;
                const int other = e.body;
                if (other > key && other < P.n) break;  // the next body's: another lane's
                const double w[3] = {e.vel[0], e.vel[1], e.vel[2]};
                if (other == key && impulse_finite(w)) {
#pragma unroll
                    for (int a = 0; a < 3; a++) to[a] = to[a] + w[a];
                }
            }
#pragma unroll
            for (int a = 0; a < 3; a++) b.vel[a] = to[a];
        }
        applied += (unsigned)__syncthreads_count(good);  // (and every velocity of the tile is written)
        taken += (unsigned)n;
        carry = top > carry ? top : carry;
        c += n;
        if (n < VRT_PHYS_BLOCK) break;
    }
    if (tid == 0) Q.at = c, Q.applied += applied, Q.skipped += taken - applied;
}

template <bool LOG>
__global__ void __launch_bounds__(VRT_PHYS_BLOCK) physics_impulses_kernel(PhysParams P, vrt_physics_run_params R, int32_t* ticks_done,
                                                                          vrt_body_sample* trace, ContactLog L,
                                                                          unsigned long long* counts, ImpulseList I) {
    __shared__ PhysSelf S;
    __shared__ vrt_object s_self;
    __shared__ int s_cand[VRT_PHYS_BLOCK];
    __shared__ double s_terms[VRT_PHYS_BLOCK][2];
    __shared__ int s_key[VRT_PHYS_BLOCK];  // the log's: the candidate each contact of a pass belongs to, in order
    __shared__ int s_wave[VRT_PHYS_WAVES];
    __shared__ int s_max[VRT_PHYS_WAVES];  // the impulses': the highest body of each wave's entries
    __shared__ ImpulseState Q;
    __shared__ unsigned s_refused;
    const int tid = threadIdx.x;
    // ---- this workgroup's run: its bodies, its statistics, its rows of the trace, its word of ticks_done, its log
    const int64_t run = blockIdx.x;
    P.bodies += run * P.n;
    P.stats += run * VRT_NSTATS;
    if (trace) trace += run * R.n_ticks * P.n;
    if (LOG && L.records) L.records += run * L.capacity;
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
    unsigned long long logged = LOG ? counts[run] : 0ull;  // ... and so is the log's count (lane 0 writes it back after the last barrier)
    const unsigned long long tiles = ((unsigned long long)P.n + VRT_PHYS_BLOCK - 1) / VRT_PHYS_BLOCK;
    int tick = start;  // absolute: the trace is indexed by it, the log carries it, and the impulses are listed by it
    impulses_seek(I, run, start, R.n_ticks, Q, s_wave);
    for (;;) {
        // ---- the impulses of this tick: Object.accelerate for each, before anything of the tick looks at a body
        impulses_tick(I, P, tick, R.n_ticks, Q, s_wave, s_max, work);
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
                    int seen = -1;  // the log's: the candidate of this tile's last contact so far in this step
                    for (int64_t first = 0; first < total; first += VRT_PHYS_BLOCK) {
                        const int64_t idx = first + tid;
                        bool contact = false;
                        double tf = 0.0, te = 0.0;
                        int c = 0, met = 0, wx = 0, wy = 0, wz = 0, g = 0, h = 0;  // (kept for the record)
                        if (idx < total) {
                            c = (int)(idx / slab);
                            const int v = (int)(idx - (int64_t)c * slab);
                            const int zi = v % ext[2], yi = (v / ext[2]) % ext[1], xi = v / (ext[2] * ext[1]);
                            wx = lo[0] + xi, wy = lo[1] + yi, wz = lo[2] + zi;
                            met = s_cand[c];
                            const vrt_body& other = P.bodies[met];
                            const vrt_object& o = other.object;
                            g = physics_material(P, o, other.rim, wx - o.mins[0], wy - o.mins[1], wz - o.mins[2]);
                            if (g && P.matphys[g * 4] >= 1.0) {
                                h = physics_material(P, s_self, srim, wx - smin[0] - dir[0], wy - smin[1] - dir[1], wz - smin[2] - dir[2]);
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
                        if (LOG && contact) s_key[at] = c;
                        __syncthreads();
                        if (tid == 0) {
                            double fr = S.friction, el = S.elasticity;
                            for (int i = 0; i < n_hit; i++) fr = fr + s_terms[i][0], el = el + s_terms[i][1];
                            S.friction = fr, S.elasticity = el;
                            S.blocked = 1;
                            S.contacts += n_hit;
                        }
                        // 5. ... and the log takes those that pass its filters, in the same order
                        if constexpr (LOG)
                            contacts_log_pass(L, contact, at, n_hit, c, met, tick, k, iter, wx, wy, wz, dir, g, h, seen, logged, s_key, s_wave);
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
        P.stats[VRT_S_PHYSICS_IMPULSES] = Q.applied, P.stats[VRT_S_PHYSICS_IMPULSES_BAD] = Q.skipped;
        ticks_done[run] = tick;
        if (LOG) counts[run] = logged;
    }
}

// ---- the same with the reference's random draws: physics_batch_draws_kernel (vrt_physics_batch_draws.hip) restated, and the log ----
#define VRT_MT_N 624
#define VRT_MT_M 397
// a pass makes at most 2 * 1024 draws = 4096 outputs, from an index of at most 624: positions below 624 + 4096 = 4720 < 8 * 624
#define VRT_MT_BLOCKS 8

// MT19937's output tempering, CPython's random.random() from two outputs and the recurrence (restated from vrt_physics_draws.hip)
__device__ __forceinline__ uint32_t id_temper(uint32_t y) {
    y ^= (y >> 11);
    y ^= (y << 7) & 0x9d2c5680u;
    y ^= (y << 15) & 0xefc60000u;
    y ^= (y >> 18);
    return y;
}
__device__ __forceinline__ double id_res53(uint32_t a, uint32_t b) {
    // (a >> 5) * 2^26 + (b >> 6), an integer below 2^53, times 2^-53: every step is exact, written with exponent shifts
    return __builtin_ldexp(__builtin_ldexp((double)(a >> 5), 26) + (double)(b >> 6), -53);
}
__device__ __forceinline__ uint32_t id_twist(uint32_t hi, uint32_t lo, uint32_t far) {
    const uint32_t y = (hi & 0x80000000u) | (lo & 0x7fffffffu);
    return far ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
}
// draw `j` of the stream that starts at word `at` of block 0 (at <= 624, j < 2048: the words are inside the row)
__device__ __forceinline__ double id_at(const uint32_t* s_mt, int at, int j) {
    return id_res53(id_temper(s_mt[at + 2 * j]), id_temper(s_mt[at + 2 * j + 1]));
}

// lane 0, at body k's turn: the state of the body whose turn it is
__device__ __forceinline__ void id_take_turn(const PhysParams& P, int k, PhysSelf& S, vrt_object& s_self) {
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

template <bool LOG>
__global__ void __launch_bounds__(VRT_PHYS_BLOCK) physics_impulses_draws_kernel(PhysParams P, vrt_physics_run_params R, int32_t* ticks_done,
                                                                                vrt_body_sample* trace, uint32_t* rng,
                                                                                unsigned long long* tick_draws, ContactLog L,
                                                                                unsigned long long* counts, ImpulseList I) {
    __shared__ PhysSelf S;
    __shared__ vrt_object s_self;
    __shared__ int s_cand[VRT_PHYS_BLOCK];
    __shared__ double s_terms[VRT_PHYS_BLOCK][2];
    __shared__ int s_wave[VRT_PHYS_WAVES];
    __shared__ int s_one[VRT_PHYS_WAVES], s_two[VRT_PHYS_WAVES], s_open[VRT_PHYS_WAVES];  // per wave: tests of >= 1 draw, of 2, undecided
    __shared__ uint32_t s_mt[VRT_MT_BLOCKS * VRT_MT_N];
    __shared__ double s_open_solidity[VRT_PHYS_BLOCK];  // the undecided tests in order: the neighbour's solidity,
    __shared__ int s_open_least[VRT_PHYS_BLOCK];        // ... the least draws the tests before it make,
    __shared__ int s_open_more[VRT_PHYS_BLOCK + 1];     // ... and how many undecided tests before it made a second draw
    __shared__ unsigned s_refused;
    __shared__ uint32_t s_index;               // the next output of block 0: lane 0 writes it after a pass, every lane reads it
    __shared__ unsigned long long s_draws;     // ... after the barriers at the start of the next
    __shared__ unsigned long long s_total[7];  // lane 0's: bodies, steps, blocked, contacts, transfers, capped; s_draws at the tick's start
    __shared__ int s_start;                    // the ticks this run had behind it when the launch began
    __shared__ unsigned long long s_logged;    // the log's: the run's count (lane 0 writes it, every lane reads it after a barrier)
    __shared__ int s_seen;                     // ... and the candidate of the tile's last contact so far in this step
    __shared__ int s_max[VRT_PHYS_WAVES];      // the impulses': the highest body of each wave's entries
    __shared__ ImpulseState Q;                 // ... and the run's place in its list
    double* const s_draw = &s_terms[0][0];      // the draws of a pass, until its contacts are known
    int* const s_key = s_open_least;            // the log's: dead once a pass's draws are decided, the contacts' candidates after
    const int tid = threadIdx.x;
    // ---- this workgroup's run: its bodies, its statistics, its rows of the trace, its generator, its draw counts, its word
    // of ticks_done, its log
    const int64_t run = blockIdx.x;
    P.bodies += run * P.n;
    P.stats += run * VRT_NSTATS;
    if (trace) trace += run * R.n_ticks * P.n;
    rng += run * (VRT_MT_N + 1);
    if (tick_draws) tick_draws += run * R.n_ticks;
    ticks_done += run;
    if (LOG) counts += run;
    if (LOG && L.records) L.records += run * L.capacity;
    if (tid < VRT_NSTATS) P.stats[tid] = 0ull;
    if (tid == 0) s_refused = 0u, s_draws = 0ull, s_start = *ticks_done;
    __syncthreads();
    int tick = s_start;  // absolute: the trace and the draw counts are indexed by it
    if (tick < 0 || tick > R.n_ticks) {  // device data: the run counts as done, nothing of it is touched or read
        if (tid == 0) P.stats[VRT_S_PHYSICS_BATCH_BADTICK] = 1ull;
        return;
    }
    if (tick == R.n_ticks) return;  // done by an earlier launch: TICKS = 0, the generator is not looked at
    if (tid == 0) s_index = rng[VRT_MT_N];
    __syncthreads();
    // ---- the index is device data: checked before it is used for anything.  Out of range: no tick, nothing written
    if (s_index > VRT_MT_N) {
        if (tid == 0) P.stats[VRT_S_PHYSICS_RNG_INVALID] = 1ull;
        return;
    }
    if (P.n == 0) {  // nothing to do: every tick is done, and none drew
        if (tick_draws)
            for (int t = tick + tid; t < R.n_ticks; t += VRT_PHYS_BLOCK) tick_draws[t] = 0ull;
        if (tid == 0) P.stats[VRT_S_PHYSICS_TICKS] = (unsigned long long)(R.n_ticks - tick), *ticks_done = R.n_ticks;
        return;
    }
    for (int i = tid; i < VRT_MT_N; i += VRT_PHYS_BLOCK) s_mt[i] = rng[i];
    // (lane 0's totals live in LDS, as in the drawing run: held in registers of every lane for the whole launch they would
    // take the kernel past its 128 vector registers)
    if (tid < 7) s_total[tid] = 0ull;
    if (LOG && tid == 0) s_logged = *counts, s_seen = -1;  // (first read many barriers on)
    unsigned long long work = 0;   // every lane's, and the same in all of them
    const unsigned long long tiles = ((unsigned long long)P.n + VRT_PHYS_BLOCK - 1) / VRT_PHYS_BLOCK;
    impulses_seek(I, run, tick, R.n_ticks, Q, s_wave);
    for (;;) {
        // ---- the impulses of this tick: Object.accelerate for each, before anything of the tick looks at a body
        impulses_tick(I, P, tick, R.n_ticks, Q, s_wave, s_max, work);
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
            if (tid == 0) id_take_turn(P, k, S, s_self);
            __syncthreads();
            work += 1;
            if (!S.run) continue;
            for (int iter = 0;; iter++) {
                if (tid == 0) {
                    const double ref = __builtin_fmax(__builtin_fabs(S.va[0]), __builtin_fmax(__builtin_fabs(S.va[1]), __builtin_fabs(S.va[2])));
                    S.done = ref == 0.0 || iter >= VRT_PHYSICS_STEP_CAP;
                    if (ref != 0.0 && iter >= VRT_PHYSICS_STEP_CAP) s_total[5]++;
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
                        if (LOG) s_seen = -1;  // (the log's: no contact of this tile in this step yet; read barriers on)
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
                        // 3a. both materials, and how many draws the test makes: `one` at least one, `two` certainly two, `open` one
                        // or two (data.py:537 draws for a voxel of the neighbour, :539 for a voxel of the mover once :537 has passed)
                        int g = 0, h = 0;
                        double sg = 0.0, sh = 0.0;
                        if (idx < total) {
                            const int c = (int)(idx / slab);
                            const int v = (int)(idx - (int64_t)c * slab);
                            const int zi = v % ext[2], yi = (v / ext[2]) % ext[1], xi = v / (ext[2] * ext[1]);
                            const int wx = lo[0] + xi, wy = lo[1] + yi, wz = lo[2] + zi;
                            const vrt_body& other = P.bodies[s_cand[c]];
                            const vrt_object& o = other.object;
                            g = physics_material(P, o, other.rim, wx - o.mins[0], wy - o.mins[1], wz - o.mins[2]);
                            if (g) {
                                sg = P.matphys[g * 4];
                                h = physics_material(P, s_self, srim, wx - smin[0] - dir[0], wy - smin[1] - dir[1], wz - smin[2] - dir[2]);
                                if (h) sh = P.matphys[h * 4];
                            }
                        }
                        const bool one = g != 0;
                        const bool may = one && h != 0 && sg > 0.0;  // (a NaN is not > 0: one draw, which it fails)
                        const bool two = may && sg >= 1.0, open = may && !two;
                        // (the wave's number as a scalar: the comparisons with it below then cost no lane masks)
                        const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
                        const unsigned long long below = (1ull << lane) - 1ull;
                        __syncthreads();  // the counts of the pass before have been read
                        // 3b. the least draws before this test, and its place among the undecided ones
                        int least, rank;
                        {
                            const unsigned long long m_one = __ballot(one), m_two = __ballot(two), m_open = __ballot(open);
                            if (lane == 0) s_one[wave] = __popcll(m_one), s_two[wave] = __popcll(m_two), s_open[wave] = __popcll(m_open);
                            least = __popcll(m_one & below) + __popcll(m_two & below), rank = __popcll(m_open & below);
                        }
                        __syncthreads();
                        const int index = (int)s_index;
                        int n_least = 0, n_open = 0;
                        for (int w = 0; w < VRT_PHYS_WAVES; w++) {
                            const int d = s_one[w] + s_two[w], u = s_open[w];
                            if (w < wave) least += d, rank += u;
                            n_least += d, n_open += u;
                        }
                        if (n_least == 0) continue;  // no voxel of a neighbour in this pass: no draw (the same in every lane)
                        if (open) s_open_solidity[rank] = sg, s_open_least[rank] = least;
                        // 3c. the states the pass can reach: outputs index .. index + 2 * (n_least + n_open) - 1 of the row
                        const int last = (index + 2 * (n_least + n_open) - 1) / VRT_MT_N;  // <= 7
                        work += (unsigned long long)last + (n_open > 0 ? 1ull : 0ull);  // blocks regenerated, and a walk (uniform)
                        for (int b = 0; b < last; b++) {
                            const uint32_t* from = s_mt + b * VRT_MT_N;
                            uint32_t* to = s_mt + (b + 1) * VRT_MT_N;
                            // lane t < 227 makes words t, t + 227 and t + 454: the last of them, word 623, wraps to the new word 0
                            const int D = VRT_MT_N - VRT_MT_M;
                            const bool mine = tid < D;
                            __syncthreads();  // block b is complete
                            if (mine) to[tid] = id_twist(from[tid], from[tid + 1], from[tid + VRT_MT_M]);
                            __syncthreads();  // words 0..226
                            if (mine) to[tid + D] = id_twist(from[tid + D], from[tid + D + 1], to[tid]);
                            __syncthreads();  // words 227..453
                            if (mine && tid + 2 * D < VRT_MT_N) {
                                const int r = tid + 2 * D;
                                to[r] = id_twist(from[r], r + 1 < VRT_MT_N ? from[r + 1] : to[0], to[r - D]);
                            }
                        }
                        __syncthreads();  // the row is there
                        // every draw the pass can make, as a double: at most 2048, where the contact terms go afterwards
                        for (int d = tid; d < n_least + n_open; d += VRT_PHYS_BLOCK) s_draw[d] = id_at(s_mt, index, d);
                        __syncthreads();  // ... and so are the draws and the list of undecided tests
                        // 3d. the undecided tests in order: each one's first draw lies after every second draw made before it
                        if (tid == 0) {
                            int more = 0;
                            for (int i = 0; i < n_open; i++) {
                                s_open_more[i] = more;
                                more += s_open_solidity[i] > s_draw[s_open_least[i] + more];
                            }
                            s_open_more[n_open] = more;
                        }
                        __syncthreads();
                        // 3e. the draws of this test (data.py:537, 539)
                        const int at = least + s_open_more[rank];
                        const int n_pass = n_least + s_open_more[n_open];
                        bool contact = false;
                        double tf = 0.0, te = 0.0;
                        if (one && sg > s_draw[at] && h && sh > s_draw[at + 1]) {
                            contact = true;
                            tf = P.matphys[g * 4 + 1] * P.matphys[h * 4 + 1] * P.p.friction;
                            te = P.matphys[g * 4 + 2] * P.matphys[h * 4 + 2] * P.p.friction;
                        }
                        // 4. the contacts of this pass, compacted in order; one lane adds them as the reference does
                        const int n_hit = __syncthreads_count(contact);  // (every lane has read its draws)
                        // the generator after the pass: the state its last output came from, twisted no further than CPython has
                        const int end = index + 2 * n_pass;
                        const int turns = end > VRT_MT_N ? (end - 1) / VRT_MT_N : 0;  // <= last
                        if (turns && tid < VRT_MT_N) s_mt[tid] = s_mt[turns * VRT_MT_N + tid];
                        if (tid == 0) s_index = (uint32_t)(end - turns * VRT_MT_N), s_draws += (unsigned long long)n_pass;
                        if (n_hit == 0) continue;
                        const int hit_at = physics_slot(contact, s_wave);
                        if (contact) s_terms[hit_at][0] = tf, s_terms[hit_at][1] = te;
                        if (LOG && contact) s_key[hit_at] = (int)(idx / slab);
                        __syncthreads();
                        if (tid == 0) {
                            double fr = S.friction, el = S.elasticity;
                            for (int i = 0; i < n_hit; i++) fr = fr + s_terms[i][0], el = el + s_terms[i][1];
                            S.friction = fr, S.elasticity = el;
                            S.blocked = 1;
                            S.contacts += n_hit;
                        }
                        // 5. ... and the log takes those that pass its filters, in the same order
                        if constexpr (LOG)
                            contacts_log_pass_shared(L, contact, hit_at, n_hit, idx, slab, lo, ext, s_cand, tick, k, iter, dir, g, h, &s_seen,
                                                     &s_logged, s_key, s_wave);
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
                s_total[0]++, s_total[1] += S.steps, s_total[2] += S.blocked_steps, s_total[3] += S.contacts, s_total[4] += S.transfers;
            }
        }
        __syncthreads();  // the last body is back: the records are the tick's
        tick++;
        if (tid == 0) {  // (lane 0 alone writes s_draws, so it reads its own)
            if (tick_draws) tick_draws[tick - 1] = s_draws - s_total[6];
            s_total[6] = s_draws;
        }
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
    // the generator goes back once: block 0 is the state the last draw came from, `index` the next output in it
    for (int i = tid; i < VRT_MT_N; i += VRT_PHYS_BLOCK) rng[i] = s_mt[i];
    if (tid == 0) {
        rng[VRT_MT_N] = s_index;
        P.stats[VRT_S_PHYSICS_BODIES] = s_total[0], P.stats[VRT_S_PHYSICS_REFUSED] = s_refused, P.stats[VRT_S_PHYSICS_STEPS] = s_total[1];
        P.stats[VRT_S_PHYSICS_BLOCKED] = s_total[2], P.stats[VRT_S_PHYSICS_CONTACTS] = s_total[3];
        P.stats[VRT_S_PHYSICS_TRANSFERS] = s_total[4], P.stats[VRT_S_PHYSICS_CAPPED] = s_total[5];
        P.stats[VRT_S_PHYSICS_WORK] = work, P.stats[VRT_S_PHYSICS_TICKS] = (unsigned long long)(tick - s_start);
        P.stats[VRT_S_PHYSICS_DRAWS] = s_draws;
        P.stats[VRT_S_PHYSICS_IMPULSES] = Q.applied, P.stats[VRT_S_PHYSICS_IMPULSES_BAD] = Q.skipped;
        *ticks_done = tick;
        if (LOG) *counts = s_logged;
    }
}

extern "C" int vrt_physics_run_batch_impulses(vrt_body* d_bodies, int32_t n_runs, int32_t n_bodies, const uint8_t* d_models,
                                              int64_t models_bytes, const uint8_t* d_remap, int32_t remap_bytes, const double* d_matphys,
                                              int32_t n_materials, const vrt_physics_params* params, const vrt_physics_run_params* run,
                                              int32_t* d_ticks_done, vrt_body_sample* d_trace, uint64_t* d_stats, void* stream_,
                                              uint32_t* d_rng, uint64_t* d_tick_draws, const vrt_contact_log* log,
                                              const vrt_impulse_list* impulses) {
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
    if (log && !contacts_args_ok(log, n_runs)) return VRT_ERR_ARG;  // (no log is allowed here)
    // (d_rng chooses the tick: with it what vrt_physics_run_batch_draws refuses of its generators is refused here)
    if (d_rng && (((uintptr_t)d_rng & 3) != 0 || ((uintptr_t)d_tick_draws & 7) != 0)) return VRT_ERR_ARG;
    if (!impulses || !impulses->d_first || ((uintptr_t)impulses->d_first & 3) != 0) return VRT_ERR_ARG;
    if (impulses->total < 0 || impulses->total > VRT_PHYSICS_MAX_IMPULSES) return VRT_ERR_ARG;
    if ((impulses->total > 0 && !impulses->d_impulses) || ((uintptr_t)impulses->d_impulses & 7) != 0) return VRT_ERR_ARG;
    PhysParams P;
    P.bodies = d_bodies, P.models = d_models, P.remap = d_remap, P.matphys = d_matphys;
    P.stats = (unsigned long long*)d_stats;
    P.models_bytes = models_bytes;
    P.n = n_bodies, P.remap_bytes = remap_bytes, P.n_materials = n_materials;
    P.p = *params;
    ContactLog L;
    L.records = nullptr, L.mask = nullptr, L.capacity = 0, L.mode = VRT_CONTACTS_VOXELS;
    unsigned long long* counts = nullptr;
    if (log) L.records = log->d_records, L.mask = log->d_mask, L.capacity = log->capacity, L.mode = log->mode, counts = (unsigned long long*)log->d_counts;
    ImpulseList I;
    I.entries = impulses->d_impulses, I.first = impulses->d_first, I.total = impulses->total;
    // one workgroup per run, and none of them waits for another; without a log, the instance that has none of its statements
    if (d_rng && log)
        hipLaunchKernelGGL(physics_impulses_draws_kernel<true>, dim3(n_runs), dim3(VRT_PHYS_BLOCK), 0, stream, P, *run, d_ticks_done, d_trace,
                           d_rng, (unsigned long long*)d_tick_draws, L, counts, I);
    else if (d_rng)
        hipLaunchKernelGGL(physics_impulses_draws_kernel<false>, dim3(n_runs), dim3(VRT_PHYS_BLOCK), 0, stream, P, *run, d_ticks_done, d_trace,
                           d_rng, (unsigned long long*)d_tick_draws, L, counts, I);
    else if (log)
        hipLaunchKernelGGL(physics_impulses_kernel<true>, dim3(n_runs), dim3(VRT_PHYS_BLOCK), 0, stream, P, *run, d_ticks_done, d_trace, L,
                           counts, I);
    else
        hipLaunchKernelGGL(physics_impulses_kernel<false>, dim3(n_runs), dim3(VRT_PHYS_BLOCK), 0, stream, P, *run, d_ticks_done, d_trace, L,
                           counts, I);
    if (hipGetLastError() != hipSuccess) return VRT_ERR_HIP;
    return VRT_OK;
}
