// vrt_physics_contacts.h -- what the kernels of vrt_physics_contacts.hip add to the ticks they restate: the contact log of a run
// (vrt_contact_log, include/vrt.h).  Device helpers only, all forced inline; included after vrt_physics_common.h, which stays as
// it is: nothing here is seen by the other physics units.
#pragma once

static_assert(sizeof(vrt_contact) == 40 && alignof(vrt_contact) == 4 && sizeof(vrt_contact_log) == 32, "record sizes of include/vrt.h");

// the log of the run a workgroup owns: its rows of the records, the shared mask and the two settings
struct ContactLog {
    vrt_contact* records;  // [capacity] of this run, or NULL with capacity == 0
    const uint8_t* mask;   // [n] or NULL
    int32_t capacity, mode;
};

// One pass's contacts into the log.  Called by every lane after the pass's contacts were compacted in order (`at`: this lane's
// place among the `n_hit` contacts, n_hit > 0) and every contact lane has written the index of its met body among the tile's
// candidates to s_key[at], with a barrier since.  `seen`: the candidate of the last contact of the earlier passes of this
// tile of this step, -1 if there was none (the same in all lanes): a met body's tests are contiguous, so it is the only one
// whose first contact can lie in an earlier pass.  `logged`: the run's count so far, the same in all lanes.
// Three barriers; s_wave is physics_slot's.  Every store is a lane's own record, written with vector stores.
__device__ __forceinline__ void contacts_log_pass(const ContactLog& L, bool contact, int at, int n_hit, int c, int other, int tick, int mover,
                                                  int step, int wx, int wy, int wz, const int* dir, int g, int h, int& seen,
                                                  unsigned long long& logged, const int* s_key, int* s_wave) {
    bool logs = contact;
    if (L.mask) logs = logs && ((L.mask[mover] & 1) || (L.mask[other] & 2));  // (other: a candidate, so below n)
    if (L.mode == VRT_CONTACTS_PAIRS) logs = logs && (at == 0 ? c != seen : s_key[at - 1] != c);
    const int last = s_key[n_hit - 1];
    const int n_log = __syncthreads_count(logs);  // (s_key has been read)
    seen = last;
    if (n_log == 0) return;
    const int rank = physics_slot(logs, s_wave);
    const unsigned long long to = logged + (unsigned long long)rank;
    if (logs && to < (unsigned long long)L.capacity) {
        vrt_contact r;
        r.tick = tick, r.mover = mover, r.other = other, r.step = step;
        r.voxel[0] = wx, r.voxel[1] = wy, r.voxel[2] = wz;
        r.dir[0] = (int8_t)dir[0], r.dir[1] = (int8_t)dir[1], r.dir[2] = (int8_t)dir[2];
        r.mat_other = (uint8_t)g, r.mat_mover = (uint8_t)h;
#pragma unroll
        for (int i = 0; i < 7; i++) r.reserved[i] = 0;
        L.records[to] = r;
    }
    logged += (unsigned long long)n_log;
}

// The same for the drawing kernel, which has no register to spare (physics_batch_draws_kernel stands at 127 of the 128 a
// 1024-thread workgroup may use): `seen` and the run's count live in LDS (s_seen, s_logged: lane 0 writes them, every lane reads
// them after a barrier), and what the record needs besides the materials is worked out again from the test's number `idx` in the
// tile's tests instead of being kept across the compaction.  s_key is an array that is dead once a pass's draws are decided.
// Four barriers.  The caller sets *s_seen = -1 at the start of a tile's tests, with a barrier before the first pass reads it.
__device__ __forceinline__ void contacts_log_pass_shared(const ContactLog& L, bool contact, int at, int n_hit, int64_t idx, int64_t slab,
                                                         const int* lo, const int* ext, const int* s_cand, int tick, int mover, int step,
                                                         const int* dir, int g, int h, int* s_seen, unsigned long long* s_logged,
                                                         const int* s_key, int* s_wave) {
    const int c = contact ? (int)(idx / slab) : 0;
    bool logs = contact;
    int other = 0;
    if (contact) other = s_cand[c];
    if (L.mask) logs = logs && ((L.mask[mover] & 1) || (L.mask[other] & 2));  // (other: a candidate, so below n)
    if (L.mode == VRT_CONTACTS_PAIRS) logs = logs && (at == 0 ? c != *s_seen : s_key[at - 1] != c);
    const int last = s_key[n_hit - 1];
    const int n_log = __syncthreads_count(logs);  // (s_key and s_seen have been read)
    if (threadIdx.x == 0) *s_seen = last;
    if (n_log == 0) return;
    const int rank = physics_slot(logs, s_wave);
    const unsigned long long to = *s_logged + (unsigned long long)rank;
    if (logs && to < (unsigned long long)L.capacity) {
        const int v = (int)(idx - (int64_t)c * slab);
        vrt_contact r;
        r.tick = tick, r.mover = mover, r.other = other, r.step = step;
        r.voxel[0] = lo[0] + v / (ext[2] * ext[1]), r.voxel[1] = lo[1] + (v / ext[2]) % ext[1], r.voxel[2] = lo[2] + v % ext[2];
        r.dir[0] = (int8_t)dir[0], r.dir[1] = (int8_t)dir[1], r.dir[2] = (int8_t)dir[2];
        r.mat_other = (uint8_t)g, r.mat_mover = (uint8_t)h;
#pragma unroll
        for (int i = 0; i < 7; i++) r.reserved[i] = 0;
        L.records[to] = r;
    }
    __syncthreads();  // every lane has read the count
    if (threadIdx.x == 0) *s_logged += (unsigned long long)n_log;
}

// What vrt_physics_run_batch_contacts refuses of its log before any HIP call (include/vrt.h)
static inline bool contacts_args_ok(const vrt_contact_log* log, int32_t n_runs) {
    if (!log || log->capacity < 0 || (log->mode != VRT_CONTACTS_VOXELS && log->mode != VRT_CONTACTS_PAIRS)) return false;
    if (!log->d_counts || ((uintptr_t)log->d_counts & 7) != 0) return false;
    if ((log->capacity > 0 && !log->d_records) || ((uintptr_t)log->d_records & 7) != 0) return false;
    if ((int64_t)n_runs * log->capacity > 0x7fffffffll) return false;
    return true;
}
