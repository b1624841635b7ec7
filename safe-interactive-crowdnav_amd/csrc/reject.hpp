// Collision-free sampling: the device half of jmid_denoise_reject_seeded (include/jmid_hip.h states the rule).
//
// The reference's DiffusionTraj.sample (MID/models/diffusion.py:544-613) takes with_constraints and returns the counts of a rejection
// loop whose body is gone; check_collision_velocity (MID/models/collision_check_utils.py:100-108) is its predicate.  Here a joint sample
// is ACCEPTABLE iff collision_sample_kernel (collision_stats.hpp) gives it n_agents_colliding == 0 and a min_dist that is not NaN - read
// from that kernel's own fp64 per-sample values (CollisionStatsArgs::ws), so the predicate is the one jmid_collision_statistics reports.
// With walls (jmid_denoise_reject_walls_seeded) it must ALSO have n_agents_hitting == 0 and a min_clear that is not NaN in
// wall_sample_kernel's per-sample values (WallStatsArgs::ws, wall_stats.hpp); without walls that workspace is null and nothing else is read.
//
// A redraw is a whole episode (its K samples are one attention sequence).  Per round:
//   reject_init_kernel     round 0, one workgroup per episode: the slot table from the flags, the episode's counters
//   reject_accept_kernel   round j >= 1, one workgroup per RERUN episode: the i-th smallest bad slot takes the i-th smallest acceptable
//                          candidate of the rerun (positions and velocities), the slot table and the counters follow
//   reject_compact_kernel  one workgroup: the ascending list of the episodes that still have a bad slot, its length in front
//   reject_gather_kernel   one workgroup per listed episode: its ctx [A, ctx_dim] and p0 [A, 2] rows into the rerun's input block
// Ranks come from a block-wide exclusive scan over per-thread counts; a thread owns ceil(K / 256) CONSECUTIVE samples (episodes in the
// compaction), so ranks ascend with the index.  Fixed order, no atomics: an episode's rows depend on nothing but the episode.
//
// A padded batch (jmid_denoise_reject_padded_seeded) needs no rule of its own here: the flags come from the same two kernels run with
// the round's agent counts, the candidates' padded rows are quiet NaN and are copied as they are, and the gather moves whole [A, ...]
// rows - the row stride is the call's A in every round.
#pragma once
#include "common.hpp"

namespace jmid {

constexpr int REJ_THREADS = 256;
constexpr int REJ_MAX_K = 1024;
constexpr int REJ_SLOT_COLS = 3;       // round whose draw the slot holds, candidate index within that round, 1 = not acceptable
constexpr int REJ_EPISODE_COLS = 3;    // slots not acceptable at round 0, slots fixed, last round in which the episode was rerun

struct RejectArgs {
    const double* ws;                  // [Er, K, 2] min_dist, n_agents_colliding of the round's candidates (collision_sample_kernel)
    const double* ws_wall;             // [Er, K, 2] min_clear, n_agents_hitting of the round's candidates (wall_sample_kernel); null: no walls
    const float *cand_pos, *cand_vel;  // [Er, K, n] the rerun's output block (cand_vel null: no velocities were asked for)
    float *acc_pos, *acc_vel;          // [E, K, n] the accepted block
    int* slots;                        // [E, K, 3]
    int* episodes;                     // [E, 3]
    int* remaining;                    // [E] bad slots left
    int* cause;                        // [E, 2] slots whose round-0 sample fails the pedestrian predicate, the wall predicate
    int* list;                         // [1 + E] the number of episodes to rerun, then their indices, ascending
    const float *ctx, *p0;             // [E, A, ctx_dim], [E, A, 2]
    float *g_ctx, *g_p0;               // [Er, A, ctx_dim], [Er, A, 2] the rerun's input block
    int E, K, n, round;                // n = A * T * 2
    int n_ctx, n_p0;                   // A * ctx_dim, A * 2
};

// one predicate on one workspace: no agent counted and a clearance that is not NaN (ws null: nothing to fail)
__device__ __forceinline__ bool rej_clear(const double* ws, size_t sample) {
    if (!ws) return true;
    const double clearance = ws[sample * 2], n_agents = ws[sample * 2 + 1];
    return n_agents == 0.0 && clearance == clearance;
}
__device__ __forceinline__ bool rej_acceptable(const RejectArgs& g, size_t sample) {
    return rej_clear(g.ws, sample) && rej_clear(g.ws_wall, sample);
}

// exclusive scan of one count per thread over the thread index (sh [2 * REJ_THREADS]); *total: the sum, in every thread
__device__ __forceinline__ int rej_excl_scan(int v, int* sh, int tid, int* total) {
    int *a = sh, *b = sh + REJ_THREADS;
    __syncthreads();
    a[tid] = v;
    __syncthreads();
    for (int o = 1; o < REJ_THREADS; o <<= 1) {
        b[tid] = a[tid] + (tid >= o ? a[tid - o] : 0);
        __syncthreads();
        int* t = a; a = b; b = t;
    }
    const int incl = a[tid];
    *total = a[REJ_THREADS - 1];
    __syncthreads();
    return incl - v;
}

// round 0: the candidates ARE the accepted block (the denoise call wrote it); slot s holds (0, s, flag)
static __global__ __launch_bounds__(REJ_THREADS) void reject_init_kernel(RejectArgs g) {
    __shared__ int sh[2 * REJ_THREADS];
    const int tid = threadIdx.x, e = blockIdx.x, K = g.K;
    const int per = (K + REJ_THREADS - 1) / REJ_THREADS, s0 = min(tid * per, K), s1 = min(s0 + per, K);
    int nbad = 0, nped = 0, nwall = 0;
    for (int s = s0; s < s1; ++s) {
        const size_t q = (size_t)e * K + s;
        const int ped = rej_clear(g.ws, q) ? 0 : 1, wall = rej_clear(g.ws_wall, q) ? 0 : 1;
        const int bad = ped | wall;
        nped += ped;
        nwall += wall;
        g.slots[q * REJ_SLOT_COLS] = 0;
        g.slots[q * REJ_SLOT_COLS + 1] = s;
        g.slots[q * REJ_SLOT_COLS + 2] = bad;
        nbad += bad;
    }
    int total, tped, twall;
    rej_excl_scan(nbad, sh, tid, &total);
    rej_excl_scan(nped, sh, tid, &tped);
    rej_excl_scan(nwall, sh, tid, &twall);
    if (tid == 0) {
        g.cause[e * 2] = tped;
        g.cause[e * 2 + 1] = twall;
        g.episodes[e * REJ_EPISODE_COLS] = total;
        g.episodes[e * REJ_EPISODE_COLS + 1] = 0;
        g.episodes[e * REJ_EPISODE_COLS + 2] = 0;
        g.remaining[e] = total;
    }
}

// round j >= 1, block b: episode e = list[1 + b], whose K fresh candidates are block b of the rerun's output
static __global__ __launch_bounds__(REJ_THREADS) void reject_accept_kernel(RejectArgs g) {
    __shared__ int sh[2 * REJ_THREADS];
    __shared__ int bslot[REJ_MAX_K], good[REJ_MAX_K];
    const int tid = threadIdx.x, b = blockIdx.x, K = g.K, n = g.n;
    const int e = g.list[1 + b];
    const int per = (K + REJ_THREADS - 1) / REJ_THREADS, s0 = min(tid * per, K), s1 = min(s0 + per, K);
    int nb = 0, ng = 0;
    for (int s = s0; s < s1; ++s) {
        nb += g.slots[((size_t)e * K + s) * REJ_SLOT_COLS + 2];
        ng += rej_acceptable(g, (size_t)b * K + s) ? 1 : 0;
    }
    int tb, tg;
    int rb = rej_excl_scan(nb, sh, tid, &tb);      // (every flag has been read behind the scan's first barrier)
    int rg = rej_excl_scan(ng, sh, tid, &tg);
    for (int s = s0; s < s1; ++s) {
        if (g.slots[((size_t)e * K + s) * REJ_SLOT_COLS + 2]) bslot[rb++] = s;
        if (rej_acceptable(g, (size_t)b * K + s)) good[rg++] = s;
    }
    __syncthreads();
    const int np = min(tb, tg);
    for (size_t i = tid; i < (size_t)np * n; i += REJ_THREADS) {
        const size_t r = i / n, c = i - r * n;
        const size_t dst = ((size_t)e * K + bslot[r]) * n + c, src = ((size_t)b * K + good[r]) * n + c;
        g.acc_pos[dst] = g.cand_pos[src];
        if (g.cand_vel) g.acc_vel[dst] = g.cand_vel[src];
    }
    for (int r = tid; r < np; r += REJ_THREADS) {
        const size_t q = ((size_t)e * K + bslot[r]) * REJ_SLOT_COLS;
        g.slots[q] = g.round;
        g.slots[q + 1] = good[r];
        g.slots[q + 2] = 0;
    }
    if (tid == 0) {
        g.episodes[e * REJ_EPISODE_COLS + 1] += np;
        g.episodes[e * REJ_EPISODE_COLS + 2] = g.round;
        g.remaining[e] = tb - np;
    }
}

// list <- {count, the episodes with remaining > 0 in ascending order}
static __global__ __launch_bounds__(REJ_THREADS) void reject_compact_kernel(RejectArgs g) {
    __shared__ int sh[2 * REJ_THREADS];
    const int tid = threadIdx.x, E = g.E;
    const int per = (E + REJ_THREADS - 1) / REJ_THREADS, e0 = min(tid * per, E), e1 = min(e0 + per, E);
    int cnt = 0;
    for (int e = e0; e < e1; ++e) cnt += g.remaining[e] > 0 ? 1 : 0;
    int total;
    int r = rej_excl_scan(cnt, sh, tid, &total);
    for (int e = e0; e < e1; ++e)
        if (g.remaining[e] > 0) g.list[1 + r++] = e;
    if (tid == 0) g.list[0] = total;
}

// block b: the ctx and p0 rows of episode list[1 + b] into row block b of the rerun's inputs
static __global__ __launch_bounds__(REJ_THREADS) void reject_gather_kernel(RejectArgs g) {
    const int tid = threadIdx.x, b = blockIdx.x;
    const int e = g.list[1 + b];
    for (int i = tid; i < g.n_ctx; i += REJ_THREADS) g.g_ctx[(size_t)b * g.n_ctx + i] = g.ctx[(size_t)e * g.n_ctx + i];
    for (int i = tid; i < g.n_p0; i += REJ_THREADS) g.g_p0[(size_t)b * g.n_p0 + i] = g.p0[(size_t)e * g.n_p0 + i];
}

inline hipError_t launch_reject_init(const RejectArgs& g, hipStream_t st) {
    hipLaunchKernelGGL(reject_init_kernel, dim3(g.E), dim3(REJ_THREADS), 0, st, g);
    return hipGetLastError();
}
inline hipError_t launch_reject_accept(const RejectArgs& g, int n_rerun, hipStream_t st) {
    hipLaunchKernelGGL(reject_accept_kernel, dim3(n_rerun), dim3(REJ_THREADS), 0, st, g);
    return hipGetLastError();
}
inline hipError_t launch_reject_compact(const RejectArgs& g, hipStream_t st) {
    hipLaunchKernelGGL(reject_compact_kernel, dim3(1), dim3(REJ_THREADS), 0, st, g);
    return hipGetLastError();
}
inline hipError_t launch_reject_gather(const RejectArgs& g, int n_rerun, hipStream_t st) {
    hipLaunchKernelGGL(reject_gather_kernel, dim3(n_rerun), dim3(REJ_THREADS), 0, st, g);
    return hipGetLastError();
}

}  // namespace jmid
