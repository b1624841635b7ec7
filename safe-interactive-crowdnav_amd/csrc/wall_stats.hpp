// Wall statistics of joint samples: how close each agent's forecast path comes to every wall segment, and who walks into one.
//
// Reference: constrain_agent_action_exact (crowd_sim_plus/envs/crowd_sim_plus.py:885-893) takes an agent's step as a line segment and
// says it hits a wall when closest_distance_between_line_segments(wall, step) - radius < 0 (crowd_sim_plus/envs/utils/utils_plus.py:
// 205-338).  wls_segment_dist restates that function's branches in the plane, as crowd_env._closest_between_segments does, and keeps
// the distance only:
//     a segment shorter than 1e-8 is its first point, with a zero direction                                 (:222-231)
//     cross = _A x _B, denom = cross^2; denom == 0 exactly: the parallel branch                             (:233-291)
//         the step wholly before the wall's start / wholly behind its end: the end point of the step that is nearer along the wall
//         otherwise an overlap: the wall turned to run with the step, then b0 onto the wall or the wall's start onto the step
//     otherwise the crossing branch: the two projections, each clamped, each clamp re-projecting the other point   (:296-338)
// A zero-length wall therefore goes through the parallel branch with d0 = d1 = 0 and yields the distance to the step's END point; that
// is the reference's value and it is kept.  No other formula is substituted: near-parallel segments divide by the same tiny denom.
//
// Agent a of sample (e, k) walks pos[t-1] -> pos[t], t = 1 .. T-1, and with p0 the segment p0 -> pos[0] before them.  d(a, l) is the
// minimum over those segments, in step order, with a min that keeps a NaN (cls_min); a segment with a non-finite end is NaN.  The agent
// hits wall l iff d(a, l) - radius < 0 in fp64 (NaN never hits).
//
// fp64 on the fp32 inputs, like collision_stats.hpp.  One workgroup per (episode, sample): its A x T x 2 block, the episode's p0 rows
// and the walls go to LDS once, as fp64; the threads stride over (agent, wall) and walk the segments in step order.  The sample's
// reductions run per thread in index order and then as a binary tree over the thread index.  The per-sample {min_clear,
// n_agents_hitting} go to the fp64 workspace; the K samples of an episode are reduced by collision_scene_kernel, whose definitions the
// scene row shares ("hits a wall" for "collides").  No atomics; agent flags are plain byte stores of 1 in LDS.
//
// Padded batches (WallStatsArgs::n_agents, jmid_wall_statistics_padded): the workgroup of (episode e, sample k) loads and walks the
// n_e real agents only - the (agent, wall) order and the reductions are those of the plain call on the compacted episode -, writes quiet
// NaN into the padded agents' rows of dist_out and leaves their bytes 0; padded rows of pos and p0 are never read.  n_agents null: the
// plain call, bit for bit.
#pragma once
#include "collision_stats.hpp"

namespace jmid {

constexpr int WLS_THREADS = CLS_THREADS;
constexpr int WLS_SAMPLE_COLS = 3;    // min_clear, n_agents_hitting, n_hits
constexpr int WLS_SCENE_COLS = CLS_SCENE_COLS;      // wall_hit_rate, agent_wall_hit_rate, min_clear_min, min_clear_mean, min_clear_std
constexpr int WLS_MAX_L = 64;
constexpr int WLS_WS_COLS = CLS_WS_COLS;            // per sample, fp64: min_clear, n_agents_hitting
constexpr double WLS_DEGENERATE = 1e-8;

struct WallStatsArgs {
    const float* pos;             // [E, K, A, T, 2]
    const float* p0;              // [E, A, 2] or null
    const double* walls;          // [L, 4] {x1, y1, x2, y2}, on the device
    float* dist_out;              // [E, K, A, L] or null
    unsigned char* agent_out;     // [E, K, A] or null
    float* sample_out;            // [E, K, 3] or null
    float* scene_out;             // [E, 5] or null
    double* ws;                   // [E, K, 2]
    double radius;
    int E, A, K, T, L;
    const int* n_agents;          // [E] on the device: the real agents of a padded batch's episodes (1 <= n_e <= A), or null: A everywhere
};

// The [A, L] table of minima is NOT kept in LDS: every (agent, wall) value is consumed by the thread that computed it (its store, its
// flag, its share of the sample's minimum and counts), so the block is the points, the walls, one reduction row and the flags - 29.1 KB
// at A = 64, T = 24 with p0, L = 64.  launch_wall_stats passes exactly this.
inline size_t wall_sample_lds(int A, int T, bool with_p0, int L) {
    const size_t np = (size_t)T + (with_p0 ? 1 : 0);
    return sizeof(double) * ((size_t)A * np * 2 + (size_t)L * 4 + WLS_THREADS) + (((size_t)A + 7) / 8) * 8;
}

__device__ __forceinline__ double wls_dist(double px, double py, double qx, double qy) {
    const double dx = px - qx, dy = py - qy;
    return sqrt(dx * dx + dy * dy);
}

// closest distance between the wall a0 -> a1 and the step b0 -> b1 (closest_distance_between_line_segments, :205-338)
__device__ __forceinline__ double wls_segment_dist(double a0x, double a0y, double a1x, double a1y, double b0x, double b0y, double b1x,
                                                   double b1y) {
    if (!(isfinite(b0x) && isfinite(b0y) && isfinite(b1x) && isfinite(b1y))) return __builtin_nan("");
    double Ax = a1x - a0x, Ay = a1y - a0y, Bx = b1x - b0x, By = b1y - b0y;
    const double magA = sqrt(Ax * Ax + Ay * Ay), magB = sqrt(Bx * Bx + By * By);
    double uAx = 0.0, uAy = 0.0, uBx = 0.0, uBy = 0.0;
    if (magA < WLS_DEGENERATE) { a1x = a0x; a1y = a0y; }
    else { uAx = Ax / magA; uAy = Ay / magA; }
    if (magB < WLS_DEGENERATE) { b1x = b0x; b1y = b0y; }
    else { uBx = Bx / magB; uBy = By / magB; }
    const double cross = uAx * uBy - uAy * uBx;
    const double denom = cross * cross;
    if (denom == 0.0) {
        const double d0 = uAx * (b0x - a0x) + uAy * (b0y - a0y);
        const double d1 = uAx * (b1x - a0x) + uAy * (b1y - a0y);
        if (d0 <= 0.0 && 0.0 >= d1) return fabs(d0) < fabs(d1) ? wls_dist(a0x, a0y, b0x, b0y) : wls_dist(a0x, a0y, b1x, b1y);
        if (d0 >= magA && magA <= d1) return fabs(d0) < fabs(d1) ? wls_dist(a1x, a1y, b0x, b0y) : wls_dist(a1x, a1y, b1x, b1y);
        const bool same = wls_dist(uAx, uAy, uBx, uBy) < WLS_DEGENERATE || magB < WLS_DEGENERATE;
        const double fx = same ? a0x : a1x, fy = same ? a0y : a1y;
        const double ufx = same ? uAx : -uAx, ufy = same ? uAy : -uAy;
        const double d0f = ufx * (b0x - fx) + ufy * (b0y - fy);
        if (d0f >= 0.0) {
            const double t = ufx * (b0x - fx) + ufy * (b0y - fy);
            return wls_dist(fx + ufx * t, fy + ufy * t, b0x, b0y);
        }
        const double t = uBx * (fx - b0x) + uBy * (fy - b0y);
        return wls_dist(fx, fy, b0x + uBx * t, b0y + uBy * t);
    }
    const double tx = b0x - a0x, ty = b0y - a0y;
    const double t0 = cross * (tx * uBy - ty * uBx) / denom;
    const double t1 = cross * (tx * uAy - ty * uAx) / denom;
    double pAx = a0x + uAx * t0, pAy = a0y + uAy * t0, pBx = b0x + uBx * t1, pBy = b0y + uBy * t1;
    const bool outA = t0 < 0.0 || t0 > magA, outB = t1 < 0.0 || t1 > magB;
    if (t0 < 0.0) { pAx = a0x; pAy = a0y; }
    else if (t0 > magA) { pAx = a1x; pAy = a1y; }
    if (t1 < 0.0) { pBx = b0x; pBy = b0y; }
    else if (t1 > magB) { pBx = b1x; pBy = b1y; }
    if (outA) {
        double dot = uBx * (pAx - b0x) + uBy * (pAy - b0y);
        if (dot < 0.0) dot = 0.0;
        else if (dot > magB) dot = magB;
        pBx = b0x + uBx * dot; pBy = b0y + uBy * dot;
    }
    if (outB) {
        double dot = uAx * (pBx - a0x) + uAy * (pBy - a0y);
        if (dot < 0.0) dot = 0.0;
        else if (dot > magA) dot = magA;
        pAx = a0x + uAx * dot; pAy = a0y + uAy * dot;
    }
    return wls_dist(pAx, pAy, pBx, pBy);
}

// one workgroup per (episode, sample): dist_out[e, k, :, :], agent_out[e, k, :], sample_out[e, k, :], ws[e, k, :]
static __global__ __launch_bounds__(WLS_THREADS) void wall_sample_kernel(WallStatsArgs g) {
    extern __shared__ __attribute__((aligned(16))) unsigned char wls_lds_raw[];
    const int tid = threadIdx.x;
    const size_t blk = blockIdx.x;
    const int AA = g.A, T = g.T, L = g.L;                     // AA: the row stride; A: the real agents of this episode (uniform over the workgroup)
    const int A = g.n_agents ? g.n_agents[blk / (size_t)g.K] : AA;
    const int lead = g.p0 ? 1 : 0, NP = T + lead;             // points per agent; NP - 1 segments
    double* p = reinterpret_cast<double*>(wls_lds_raw);       // [A, NP, 2] the paths
    double* w = p + (size_t)A * NP * 2;                       // [L, 4] the walls
    double* red = w + (size_t)L * 4;                          // [WLS_THREADS]
    unsigned char* flag = reinterpret_cast<unsigned char*>(red + WLS_THREADS);        // [A]
    const float* src = g.pos + blk * ((size_t)AA * T * 2);    // (the real rows come first: padded rows are never read)
    for (int i = tid; i < A * T * 2; i += WLS_THREADS) {
        const int a = i / (T * 2), r = i - a * (T * 2);
        p[((size_t)a * NP + lead) * 2 + r] = (double)src[i];
    }
    if (lead) {
        const float* s0 = g.p0 + (blk / (size_t)g.K) * ((size_t)AA * 2);
        for (int i = tid; i < A * 2; i += WLS_THREADS) p[(size_t)(i >> 1) * NP * 2 + (i & 1)] = (double)s0[i];
    }
    for (int i = tid; i < L * 4; i += WLS_THREADS) w[i] = g.walls[i];
    for (int i = tid; i < AA; i += WLS_THREADS) flag[i] = 0;
    __syncthreads();
    double mn = INFINITY, n_hits = 0.0, n_agents = 0.0;
    for (int q = tid; q < A * L; q += WLS_THREADS) {
        const int a = q / L, l = q - a * L;
        const double* wl = w + l * 4;
        const double* pa = p + (size_t)a * NP * 2;
        double m = wls_segment_dist(wl[0], wl[1], wl[2], wl[3], pa[0], pa[1], pa[2], pa[3]);
        for (int s = 1; s < NP - 1; ++s)                      // in step order
            m = cls_min(m, wls_segment_dist(wl[0], wl[1], wl[2], wl[3], pa[2 * s], pa[2 * s + 1], pa[2 * s + 2], pa[2 * s + 3]));
        if (g.dist_out) g.dist_out[blk * ((size_t)AA * L) + q] = (float)m;
        if (m - g.radius < 0.0) {
            flag[a] = 1;
            n_hits += 1.0;
        }
        mn = cls_min(m, mn);
    }
    if (g.dist_out)      // the rows of the padded agents
        for (int q = A * L + tid; q < AA * L; q += WLS_THREADS) g.dist_out[blk * ((size_t)AA * L) + q] = __builtin_nanf("");
    __syncthreads();
    if (g.agent_out) {
        unsigned char* o = g.agent_out + blk * AA;
        for (int q = tid; q < AA; q += WLS_THREADS) o[q] = flag[q];      // (a padded agent's byte stays 0)
    }
    for (int q = tid; q < A; q += WLS_THREADS) n_agents += (double)flag[q];
    red[tid] = mn;
    __syncthreads();
    for (int o = WLS_THREADS / 2; o > 0; o >>= 1) {
        if (tid < o) red[tid] = cls_min(red[tid], red[tid + o]);
        __syncthreads();
    }
    const double min_clear = red[0];
    n_hits = evs_block_sum(n_hits, red, tid);
    n_agents = evs_block_sum(n_agents, red, tid);
    if (tid == 0) {
        g.ws[blk * WLS_WS_COLS] = min_clear;
        g.ws[blk * WLS_WS_COLS + 1] = n_agents;
        if (g.sample_out) {
            float* o = g.sample_out + blk * WLS_SAMPLE_COLS;
            o[0] = (float)min_clear;
            o[1] = (float)n_agents;
            o[2] = (float)n_hits;
        }
    }
}

inline hipError_t launch_wall_stats(const WallStatsArgs& g, hipStream_t st) {
    hipLaunchKernelGGL(wall_sample_kernel, dim3((unsigned)(g.E * g.K)), dim3(WLS_THREADS), wall_sample_lds(g.A, g.T, g.p0 != nullptr, g.L), st,
                       g);
    if (g.scene_out) {        // the scene row has collision_scene_kernel's definitions, on this entry's per-sample values
        CollisionStatsArgs c{};
        c.ws = g.ws; c.scene_out = g.scene_out; c.E = g.E; c.A = g.A; c.K = g.K; c.T = g.T; c.n_agents = g.n_agents;
        hipLaunchKernelGGL(collision_scene_kernel, dim3(g.E), dim3(CLS_THREADS), collision_scene_lds(g.K), st, c);
    }
    return hipGetLastError();
}

}  // namespace jmid
