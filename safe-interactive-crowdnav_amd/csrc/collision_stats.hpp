// Collision statistics of joint samples: how close the agents of one sampled future come to each other, and who collides.
//
// Reference: MID/models/collision_check_utils.py.  calc_min_dists (:58-80) takes each agent's path between consecutive horizon steps
// as a line segment; for every agent pair in pdist order (get_diffs_pred, :5-17: pos_i - pos_j, i < j) the distance between the two
// moving agents on one segment is the distance from the origin to the segment a -> b of their relative position (lineseg_dist, :20-55):
//     a == b exactly:  |a|                                                                                  (:52-53)
//     otherwise        d = (b - a) / |b - a| ;  s = a . d ;  t = -b . d ;  h = max(s, t, 0) ;  c = ((-a) x d)_z ;  hypot(h, |c|)   (:33-50)
// and the pair's value is the minimum over the T - 1 segments (:79).  get_agents_in_collision (:83-97) returns the agents of every pair
// closer than 0.2 m (a parameter here); check_collision_velocity (:100-108) is "any such agent" for one integrated sample.
// torch.min and torch.max propagate NaN: a segment with a non-finite end point is NaN here, and so are its pair and its sample's
// min_dist; NaN < threshold is false, so such a pair never collides.  T = 1 is not taken (there the reference collapses to one scalar
// over all pairs, :69-79).
//
// fp64 on the fp32 inputs, like eval_stats.hpp.  One workgroup per (episode, sample): its A x T x 2 block is contiguous in
// pos [E, K, A, T, 2] and goes to LDS once; the threads then stride over (pair, segment) - T - 1 neighbouring threads hold the segments
// of one pair, the first of them takes their minimum in step order.  The sample's reductions run per thread in index order and then
// as a binary tree over the thread index; a second kernel, one workgroup per episode, reduces the K samples the same way.  No
// atomics; agent flags are plain byte stores of 1 in LDS (every writer stores the same value).  A row depends on nothing but its own
// sample (or episode).
//
// Padded batches (CollisionStatsArgs::n_agents, jmid_collision_statistics_padded): episode e has n_e <= A real agents, rows a < n_e of its
// [A, T, 2] blocks.  A workgroup is one (episode, sample), so n_e is uniform over it: it loads the n_e real rows only, walks the
// n_e (n_e - 1) / 2 real pairs in pdist order at n_e - the loop, the reductions and their order are those of the plain call on the
// compacted episode - and writes pair (i, j) at its index at A, quiet NaN in the pairs of a padded agent, 0 in a padded agent's byte.
// The map from the index at n_e to the index at A is monotone, so the closest pair's tie rule carries over.  n_agents null: the plain
// call, bit for bit.
#pragma once
#include "common.hpp"
#include "eval_stats.hpp"

namespace jmid {

constexpr int CLS_THREADS = EVS_THREADS;
constexpr int CLS_SAMPLE_COLS = 4;    // min_dist, closest_pair, n_pairs_colliding, n_agents_colliding
constexpr int CLS_SCENE_COLS = 5;     // collision_rate, agent_collision_rate, min_dist_min, min_dist_mean, min_dist_std
constexpr int CLS_MAX_A = 64, CLS_MAX_T = 24, CLS_MAX_K = 1024;
constexpr int CLS_WS_COLS = 2;        // per sample, fp64, for the scene kernel: min_dist, n_agents_colliding

struct CollisionStatsArgs {
    const float* pos;             // [E, K, A, T, 2] (jmid_denoise's pos_out layout)
    float* pair_out;              // [E, K, P] or null
    unsigned char* agent_out;     // [E, K, A] or null
    float* sample_out;            // [E, K, 4] or null
    float* scene_out;             // [E, 5] or null
    double* ws;                   // [E, K, 2]
    double threshold;
    int E, A, K, T;
    const int* n_agents;          // [E] on the device: the real agents of a padded batch's episodes (1 <= n_e <= A), or null: A everywhere
};

// pdist order at n agents: p(i, j) = i n - i (i + 1) / 2 + (j - i - 1), i < j, and its inverse
__device__ __forceinline__ int cls_pair_index(int i, int j, int n) { return i * n - i * (i + 1) / 2 + (j - i - 1); }
__device__ __forceinline__ void cls_pair_agents(int pr, int n, int* i_out, int* j_out) {
    int i = 0, rem = pr;
    while (rem >= n - 1 - i) { rem -= n - 1 - i; ++i; }
    *i_out = i;
    *j_out = i + 1 + rem;
}

inline size_t collision_sample_lds(int A, int T) {
    const size_t P = (size_t)A * (A - 1) / 2;
    return sizeof(double) * ((size_t)A * T * 2 + P + 2 * CLS_THREADS) + sizeof(int) * CLS_THREADS + (((size_t)A + 7) / 8) * 8;
}
inline size_t collision_scene_lds(int K) { return sizeof(double) * ((size_t)K + CLS_THREADS); }

// min that keeps a NaN (np.min / torch.min), unlike fmin
__device__ __forceinline__ double cls_min(double a, double b) { return (a != a || a < b) ? a : b; }
// is (v1, i1) ahead of (v2, i2) as the closest pair: a NaN first (it decides the minimum), then the smaller value, then the lower index
__device__ __forceinline__ bool cls_ahead(double v1, int i1, double v2, int i2) {
    const bool n1 = v1 != v1, n2 = v2 != v2;
    if (n1 || n2) return n1 && (!n2 || i1 < i2);
    return v1 < v2 || (v1 == v2 && i1 < i2);
}

// distance of the origin from the segment a -> b (lineseg_dist, :20-55)
__device__ __forceinline__ double cls_segment_dist(double ax, double ay, double bx, double by) {
    if (!(isfinite(ax) && isfinite(ay) && isfinite(bx) && isfinite(by))) return __builtin_nan("");
    if (ax == bx && ay == by) return sqrt(ax * ax + ay * ay);
    const double ux = bx - ax, uy = by - ay;
    const double n = sqrt(ux * ux + uy * uy);
    const double dx = ux / n, dy = uy / n;
    const double s = ax * dx + ay * dy;
    const double t = (-bx) * dx + (-by) * dy;
    const double h = fmax(fmax(s, t), 0.0);
    const double c = (-ax) * dy - (-ay) * dx;
    return hypot(h, fabs(c));
}

// one workgroup per (episode, sample): pair_out[e, k, :], agent_out[e, k, :], sample_out[e, k, :], ws[e, k, :]
static __global__ __launch_bounds__(CLS_THREADS) void collision_sample_kernel(CollisionStatsArgs g) {
    extern __shared__ __attribute__((aligned(16))) unsigned char cls_lds_raw[];
    const int tid = threadIdx.x;
    const size_t blk = blockIdx.x;
    const int AA = g.A, T = g.T, G = T - 1;                   // AA: the row stride; A: the real agents of this episode (uniform over the workgroup)
    const int A = g.n_agents ? g.n_agents[blk / (size_t)g.K] : AA;
    const int P = A * (A - 1) / 2, n_in = A * T * 2, PA = AA * (AA - 1) / 2;
    double* p = reinterpret_cast<double*>(cls_lds_raw);       // [A, T, 2] the sample's real rows
    double* pmin = p + n_in;                                  // [P] the pair minima, in pdist order at A
    double* seg = pmin + P;                                   // [CLS_THREADS] the segment distances of one pass
    double* red = seg + CLS_THREADS;                          // [CLS_THREADS]
    int* redi = reinterpret_cast<int*>(red + CLS_THREADS);    // [CLS_THREADS]
    unsigned char* flag = reinterpret_cast<unsigned char*>(redi + CLS_THREADS);       // [A]
    const float* src = g.pos + blk * ((size_t)AA * T * 2);    // (the real rows come first: padded rows are never read)
    for (int i = tid; i < n_in; i += CLS_THREADS) p[i] = (double)src[i];
    for (int i = tid; i < AA; i += CLS_THREADS) flag[i] = 0;
    __syncthreads();
    // G neighbouring threads per pair, per_pass pairs at a time
    const int per_pass = CLS_THREADS / G, lp = tid / G, s = tid - lp * G;
    for (int p0 = 0; p0 < P; p0 += per_pass) {                // (uniform trip count)
        const int pr = p0 + lp;
        const bool on = lp < per_pass && pr < P;
        int i = 0, j = 0;
        if (on) {
            cls_pair_agents(pr, A, &i, &j);
            const double* pi = p + ((size_t)i * T + s) * 2;
            const double* pj = p + ((size_t)j * T + s) * 2;
            seg[tid] = cls_segment_dist(pi[0] - pj[0], pi[1] - pj[1], pi[2] - pj[2], pi[3] - pj[3]);
        }
        __syncthreads();
        if (on && s == 0) {
            double m = seg[tid];
            for (int q = 1; q < G; ++q) m = cls_min(m, seg[tid + q]);     // in step order
            pmin[pr] = m;
            if (m < g.threshold) { flag[i] = 1; flag[j] = 1; }
        }
        __syncthreads();
    }
    if (g.pair_out && A == AA) {
        float* o = g.pair_out + blk * P;
        for (int q = tid; q < P; q += CLS_THREADS) o[q] = (float)pmin[q];
    } else if (g.pair_out) {      // a padded episode: NaN everywhere, then the real pairs at their index at AA (uniform branch)
        float* o = g.pair_out + blk * PA;
        for (int q = tid; q < PA; q += CLS_THREADS) o[q] = __builtin_nanf("");
        __syncthreads();
        for (int q = tid; q < P; q += CLS_THREADS) {
            int i, j;
            cls_pair_agents(q, A, &i, &j);
            o[cls_pair_index(i, j, AA)] = (float)pmin[q];
        }
    }
    if (g.agent_out) {
        unsigned char* o = g.agent_out + blk * AA;
        for (int q = tid; q < AA; q += CLS_THREADS) o[q] = flag[q];      // (a padded agent's byte stays 0)
    }
    // the closest pair (the lowest index on an exact tie), the number of colliding pairs and of colliding agents
    double bv = INFINITY, n_pairs = 0.0, n_agents = 0.0;
    int bi = P;
    for (int q = tid; q < P; q += CLS_THREADS) {
        const double v = pmin[q];
        if (cls_ahead(v, q, bv, bi)) { bv = v; bi = q; }
        n_pairs += v < g.threshold ? 1.0 : 0.0;
    }
    for (int q = tid; q < A; q += CLS_THREADS) n_agents += (double)flag[q];
    __syncthreads();
    red[tid] = bv; redi[tid] = bi;
    __syncthreads();
    for (int o = CLS_THREADS / 2; o > 0; o >>= 1) {
        if (tid < o && cls_ahead(red[tid + o], redi[tid + o], red[tid], redi[tid])) { red[tid] = red[tid + o]; redi[tid] = redi[tid + o]; }
        __syncthreads();
    }
    const double min_dist = red[0];
    int closest = redi[0];
    n_pairs = evs_block_sum(n_pairs, red, tid);
    n_agents = evs_block_sum(n_agents, red, tid);
    if (tid == 0) {
        g.ws[blk * CLS_WS_COLS] = min_dist;
        g.ws[blk * CLS_WS_COLS + 1] = n_agents;
        if (g.sample_out) {
            float* o = g.sample_out + blk * CLS_SAMPLE_COLS;
            const bool none = min_dist != min_dist || closest >= P;
            if (!none && A != AA) {                           // the pair's index at the row stride
                int i, j;
                cls_pair_agents(closest, A, &i, &j);
                closest = cls_pair_index(i, j, AA);
            }
            o[0] = (float)min_dist;
            o[1] = none ? -1.0f : (float)closest;
            o[2] = (float)n_pairs;
            o[3] = (float)n_agents;
        }
    }
}

// one workgroup per episode: scene_out[e, :] from ws[e, :, :]
static __global__ __launch_bounds__(CLS_THREADS) void collision_scene_kernel(CollisionStatsArgs g) {
    extern __shared__ __attribute__((aligned(16))) unsigned char cls_lds_raw[];
    const int tid = threadIdx.x, e = blockIdx.x;
    const int A = g.n_agents ? g.n_agents[e] : g.A, K = g.K;  // the rate of the agent flags is over the episode's real agents
    double* v = reinterpret_cast<double*>(cls_lds_raw);       // [K] min_dist of the samples
    double* red = v + K;                                      // [CLS_THREADS]
    const double* w = g.ws + (size_t)e * K * CLS_WS_COLS;
    double mn = INFINITY, sm = 0.0, hit = 0.0, agents = 0.0;
    for (int s = tid; s < K; s += CLS_THREADS) {
        const double d = w[s * CLS_WS_COLS], n = w[s * CLS_WS_COLS + 1];
        v[s] = d;
        mn = cls_min(d, mn);
        sm += d;
        hit += n > 0.0 ? 1.0 : 0.0;                           // an agent collides exactly when a pair does
        agents += n;
    }
    __syncthreads();
    red[tid] = mn;
    __syncthreads();
    for (int o = CLS_THREADS / 2; o > 0; o >>= 1) {
        if (tid < o) red[tid] = cls_min(red[tid], red[tid + o]);
        __syncthreads();
    }
    mn = red[0];
    const double mean = evs_block_sum(sm, red, tid) / (double)K;
    hit = evs_block_sum(hit, red, tid);
    agents = evs_block_sum(agents, red, tid);
    double sq = 0.0;
    for (int s = tid; s < K; s += CLS_THREADS) {
        const double c = v[s] - mean;                         // (+inf - +inf = NaN with A = 1: np.std gives NaN there too)
        sq += c * c;
    }
    const double var = evs_block_sum(sq, red, tid) / (double)K;
    if (tid == 0) {
        float* o = g.scene_out + (size_t)e * CLS_SCENE_COLS;
        o[0] = (float)(hit / (double)K);
        o[1] = (float)(agents / ((double)K * (double)A));
        o[2] = (float)mn;
        o[3] = (float)mean;
        o[4] = (float)sqrt(var);
    }
}

inline hipError_t launch_collision_stats(const CollisionStatsArgs& g, hipStream_t st) {
    hipLaunchKernelGGL(collision_sample_kernel, dim3((unsigned)(g.E * g.K)), dim3(CLS_THREADS), collision_sample_lds(g.A, g.T), st, g);
    if (g.scene_out) hipLaunchKernelGGL(collision_scene_kernel, dim3(g.E), dim3(CLS_THREADS), collision_scene_lds(g.K), st, g);
    return hipGetLastError();
}

}  // namespace jmid
