// Collision repair: the device half of jmid_repair_collisions (include/jmid_hip.h states the rule).
//
// The reference's DiffusionTraj.sample (MID/models/diffusion.py:544-613) takes constraint_type next to with_constraints, and every
// shipped config sets constraint_type: opt_softplus (test_time_configs/mid_jp.yaml:34); the stripped sampler has no body for it.  Here it
// is a small fp64 optimisation on the FINISHED samples: a joint sample that collision_sample_kernel (collision_stats.hpp) flags at
// `threshold` is pushed apart under tau * softplus((threshold + margin - d) / tau) on the distance d of every pair's relative segment
// until the closest segment is threshold + margin / 2 away, rounded to fp32, and kept only when the predicate's own device function
// (cls_segment_dist) then accepts it; otherwise the sample comes back as it went in.
//
// One workgroup per (episode, sample).  It reads the two fp64 values collision_sample_kernel left for the sample (CollisionStatsArgs::ws:
// min_dist, n_agents_colliding - the lean form the rejection loop reads) and is done at once with a sample that needs nothing.  The
// sample's n x T points lie in LDS as fp64, twice (the Jacobi step reads one copy and writes the other); a thread owns the points
// tid, tid + 256, ... and walks a point's partners in ascending order, per partner the segment that ends in the point and then the one
// that starts there, so every sum has one fixed order.  One block-wide minimum per iteration decides whether the step is taken.  No
// atomics, no download; a row of the outputs depends on nothing but its own sample.
//
// With walls (jmid_repair_collisions_walls, repair_sample_kernel<true>): the sample is a candidate for either cause - the second pair of
// fp64 values is wall_sample_kernel's (WallStatsArgs::ws: min_clear, n_agents_hitting) -, every point adds, behind its partners, the terms
// of the walls in ascending order (per wall the step that ends in the point, then the one that starts there; rpr_wall_segment), the
// iteration stops when both minima clear their stop value, and the rounded sample is kept only when cls_segment_dist AND wls_segment_dist
// accept it.  The walls [L, 4] and the episode's p0 rows (the fixed first point of every path) lie in LDS as fp64 behind the reduction row.
// On top of the kernel's 62.0 KB at A = 64, T = 24 that would pass the 64 KB a workgroup gets without asking, so this instance keeps no fp32
// block of its own: the rounded sample goes into the iterate's second copy, which is dead once the iteration has ended - 53.0 KB at
// A = 64, T = 24, L = 64 with p0.  repair_sample_kernel<false> is the kernel as it was.
#pragma once
#include <type_traits>

#include "wall_stats.hpp"

namespace jmid {

constexpr int RPR_THREADS = CLS_THREADS;
constexpr int RPR_SAMPLE_COLS = 4;     // min_dist before, min_dist after, iterations used, state
constexpr int RPR_EPISODE_COLS = 3;    // samples colliding on entry, samples repaired, the largest iteration count
constexpr int RPR_MAX_ITER = 1024;
enum RepairState { RPR_UNTOUCHED = 0, RPR_REPAIRED = 1, RPR_REVERTED = 2, RPR_NAN = 3 };

struct RepairArgs {
    const double* ws;             // [E, K, 2] min_dist, n_agents_colliding of the input (collision_sample_kernel)
    const float* src;             // [E, K, A, T, 2] the samples
    float* dst;                   // [E, K, A, T, 2] where they go: src itself (in place), another block, or null (the flags only)
    const float* p0;              // [E, A, 2] or null: no velocities
    float *vel, *vel2;            // [E, K, A, T, 2] or null: velocity blocks whose rows of REPAIRED samples are rewritten
    float* sample;                // [E, K, 4]
    int* episode;                 // [E, 3] or null
    const int* n_agents;          // [E] on the device (a padded batch), or null: A everywhere
    double threshold, margin, tau, step, dt;
    int E, A, K, T, max_iter;
};

// what the kernel with walls takes on top (jmid_repair_collisions_walls)
struct RepairWallArgs : RepairArgs {
    const double* wws;            // [E, K, 2] min_clear, n_agents_hitting of the input (wall_sample_kernel, with RepairArgs::p0 as its p0)
    const double* walls;          // [L, 4] {x1, y1, x2, y2}, on the device
    float* wall_out;              // [E, K, 2] min_clear before, min_clear after (of the sample that comes back), or null
    double wall_radius;
    int L;
};
constexpr int RPR_WALL_COLS = 2;

inline size_t repair_lds(int A, int T) {
    return sizeof(double) * ((size_t)A * T * 2 * 2 + RPR_THREADS) + sizeof(float) * ((size_t)A * T * 2);
}
inline size_t repair_walls_lds(int A, int T, int L) {      // the two copies, the reduction row, the walls, the p0 rows (no fp32 block)
    return sizeof(double) * ((size_t)A * T * 2 * 2 + RPR_THREADS + (size_t)L * 4 + (size_t)A * 2);
}

// minimum of one value per thread (no NaN among them: the points of a candidate are finite); every thread gets the result
__device__ __forceinline__ double rpr_block_min(double v, double* red, int tid) {
    __syncthreads();
    red[tid] = v;
    __syncthreads();
    for (int o = RPR_THREADS / 2; o > 0; o >>= 1) {
        if (tid < o && red[tid + o] < red[tid]) red[tid] = red[tid + o];
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

// One segment s of the pair (lo, hi), lo < hi, in closest-point form: the distance d, the parameter u of the closest point, the unit
// normal n = c / d ((1, 0) where the two coincide), and sigma = sigmoid((m - d) / tau) without overflow
struct RprSegment {
    double d, u, nx, ny, sigma;
};
__device__ __forceinline__ RprSegment rpr_segment(const double* lo, const double* hi, double m, double tau) {
    const double ax = lo[0] - hi[0], ay = lo[1] - hi[1], bx = lo[2] - hi[2], by = lo[3] - hi[3];
    const double abx = bx - ax, aby = by - ay;
    const double den = abx * abx + aby * aby;
    double u = 0.0;
    if (den > 0.0) {
        u = -(ax * abx + ay * aby) / den;
        u = u < 0.0 ? 0.0 : u > 1.0 ? 1.0 : u;
    }
    const double cx = ax + u * abx, cy = ay + u * aby;
    RprSegment r;
    r.u = u;
    r.d = sqrt(cx * cx + cy * cy);
    if (r.d > 0.0) { r.nx = cx / r.d; r.ny = cy / r.d; }
    else { r.nx = 1.0; r.ny = 0.0; }
    const double z = (m - r.d) / tau;
    const double e = exp(-fabs(z));
    r.sigma = z >= 0.0 ? 1.0 / (1.0 + e) : e / (1.0 + e);
    return r;
}

// One step b0 -> b1 against one wall w = {x1, y1, x2, y2} in closest-point form (the rule's "Wall term"; NOT the predicate's branchy
// wls_segment_dist, which judges the result): the nearest, by squared distance, of four clamped projections in fixed order, the first
// winning a tie - b0 onto the wall, b1 onto the wall, the wall's start onto the step, the wall's end onto the step -, each in rpr_segment's
// closed form on the difference vectors (c points from the wall to the path).  w0 / w1: the weights of b0 / b1.  A step that properly
// crosses the wall takes the b1-onto-wall candidate with d negated and the normal reversed: the far end is pulled back to b0's side.
struct RprWallSegment {
    double d, w0, w1, nx, ny, sigma;
};
struct RprClosest {
    double u, cx, cy, s;
};
__device__ __forceinline__ RprClosest rpr_closest(double ax, double ay, double bx, double by) {
    const double abx = bx - ax, aby = by - ay;
    const double den = abx * abx + aby * aby;
    double u = 0.0;
    if (den > 0.0) {
        u = -(ax * abx + ay * aby) / den;
        u = u < 0.0 ? 0.0 : u > 1.0 ? 1.0 : u;
    }
    RprClosest r;
    r.u = u;
    r.cx = ax + u * abx;
    r.cy = ay + u * aby;
    r.s = r.cx * r.cx + r.cy * r.cy;
    return r;
}
__device__ __forceinline__ RprWallSegment rpr_wall_segment(const double* w, const double* b0, const double* b1, double m, double tau) {
    const double p00x = b0[0] - w[0], p00y = b0[1] - w[1], p01x = b0[0] - w[2], p01y = b0[1] - w[3];
    const double p10x = b1[0] - w[0], p10y = b1[1] - w[1], p11x = b1[0] - w[2], p11y = b1[1] - w[3];
    const RprClosest c0 = rpr_closest(p00x, p00y, p01x, p01y), c1 = rpr_closest(p10x, p10y, p11x, p11y);
    const RprClosest c2 = rpr_closest(p00x, p00y, p10x, p10y), c3 = rpr_closest(p01x, p01y, p11x, p11y);
    const double Wx = w[2] - w[0], Wy = w[3] - w[1], Bx = b1[0] - b0[0], By = b1[1] - b0[1];
    const double o1 = Wx * p00y - Wy * p00x, o2 = Wx * p10y - Wy * p10x;
    const double o3 = By * p00x - Bx * p00y, o4 = By * p01x - Bx * p01y;
    const bool cross = ((o1 > 0.0 && o2 < 0.0) || (o1 < 0.0 && o2 > 0.0)) && ((o3 > 0.0 && o4 < 0.0) || (o3 < 0.0 && o4 > 0.0));
    double cx = c0.cx, cy = c0.cy, s = c0.s;
    RprWallSegment r;
    r.w0 = 1.0; r.w1 = 0.0;
    if (c1.s < s) { cx = c1.cx; cy = c1.cy; s = c1.s; r.w0 = 0.0; r.w1 = 1.0; }
    if (c2.s < s) { cx = c2.cx; cy = c2.cy; s = c2.s; r.w0 = 1.0 - c2.u; r.w1 = c2.u; }
    if (c3.s < s) { cx = c3.cx; cy = c3.cy; s = c3.s; r.w0 = 1.0 - c3.u; r.w1 = c3.u; }
    if (cross) { cx = c1.cx; cy = c1.cy; s = c1.s; r.w0 = 0.0; r.w1 = 1.0; }
    r.d = sqrt(s);
    if (r.d > 0.0) { r.nx = cx / r.d; r.ny = cy / r.d; }
    else { r.nx = 1.0; r.ny = 0.0; }
    if (cross) { r.d = -r.d; r.nx = -r.nx; r.ny = -r.ny; }
    const double z = (m - r.d) / tau;
    const double e = exp(-fabs(z));
    r.sigma = z >= 0.0 ? 1.0 / (1.0 + e) : e / (1.0 + e);
    return r;
}

// WALLS = false: jmid_repair_collisions' kernel, the code it always was.  WALLS = true: the wall terms and the second gate on top
template <bool WALLS>
static __global__ __launch_bounds__(RPR_THREADS) void repair_sample_kernel(std::conditional_t<WALLS, RepairWallArgs, RepairArgs> g) {
    extern __shared__ __attribute__((aligned(16))) unsigned char rpr_lds_raw[];
    const int tid = threadIdx.x;
    const size_t blk = blockIdx.x;
    const int AA = g.A, T = g.T;                              // AA: the row stride; n: the real agents of this episode
    const size_t e = blk / (size_t)g.K;
    const int n = g.n_agents ? g.n_agents[e] : AA;
    const int n_all = AA * T * 2, n_pt = n * T, n_in = n_pt * 2;
    const float* src = g.src + blk * (size_t)n_all;
    float* dst = g.dst ? g.dst + blk * (size_t)n_all : nullptr;
    float* so = g.sample + blk * RPR_SAMPLE_COLS;
    const double before = g.ws[blk * CLS_WS_COLS], hit = g.ws[blk * CLS_WS_COLS + 1];
    // what is not repaired goes through as it is, the rows of padded agents always (the bits, whatever they are)
    if (dst && dst != src) {
        const unsigned* s32 = reinterpret_cast<const unsigned*>(src);
        unsigned* d32 = reinterpret_cast<unsigned*>(dst);
        for (int i = tid; i < n_all; i += RPR_THREADS) d32[i] = s32[i];
    }
    bool is_nan = before != before, cand = hit > 0.0 && n >= 2;
    double wbefore = INFINITY;
    if constexpr (WALLS) {                                    // a candidate for either cause, a single agent included; a NaN in either minimum
        wbefore = g.wws[blk * WLS_WS_COLS];
        is_nan = is_nan || wbefore != wbefore;
        cand = cand || g.wws[blk * WLS_WS_COLS + 1] > 0.0;
    }
    if (is_nan || !cand) {                                    // (uniform over the workgroup)
        if (tid == 0) {
            so[0] = (float)before; so[1] = (float)before; so[2] = 0.0f;
            so[3] = is_nan ? (float)RPR_NAN : (float)RPR_UNTOUCHED;
            if constexpr (WALLS)
                if (g.wall_out) g.wall_out[blk * RPR_WALL_COLS] = g.wall_out[blk * RPR_WALL_COLS + 1] = (float)wbefore;
        }
        return;
    }
    double* x = reinterpret_cast<double*>(rpr_lds_raw);       // [n, T, 2] the iterate
    double* xn = x + (size_t)AA * T * 2;                      // [n, T, 2] the next one
    double* red = xn + (size_t)AA * T * 2;                    // [RPR_THREADS]
    // [n, T, 2] the iterate rounded to fp32: a block of its own, or (WALLS) null until the iteration has ended - then the dead copy
    float* r32 = WALLS ? nullptr : reinterpret_cast<float*>(red + RPR_THREADS);
    for (int i = tid; i < n_in; i += RPR_THREADS) x[i] = (double)src[i];
    const double* wl = nullptr;                               // [L, 4] the walls
    const double* lead = nullptr;                             // [n, 2] p0: the fixed first point of every path, or null
    if constexpr (WALLS) {
        double* wls = red + RPR_THREADS;
        double* p0s = wls + (size_t)g.L * 4;
        for (int i = tid; i < g.L * 4; i += RPR_THREADS) wls[i] = g.walls[i];
        if (g.p0) {
            const float* s0 = g.p0 + e * (size_t)AA * 2;
            for (int i = tid; i < n * 2; i += RPR_THREADS) p0s[i] = (double)s0[i];
            lead = p0s;
        }
        wl = wls;
    }
    const double m = g.threshold + g.margin, stop = g.threshold + g.margin * 0.5;
    int iters = 0;
    for (int it = 0; it < g.max_iter; ++it) {                 // (uniform trip count: the exit below is block-wide)
        double dmin = INFINITY, wmin = INFINITY;
        __syncthreads();
        for (int pt = tid; pt < n_pt; pt += RPR_THREADS) {
            const int a = pt / T, t = pt - a * T;
            double gx = 0.0, gy = 0.0;
            for (int b = 0; b < n; ++b) {
                if (b == a) continue;
                const bool first = a < b;                     // the pair is (lo, hi) = (min, max): i subtracts, j adds
                const double* lo = x + ((size_t)(first ? a : b) * T) * 2;
                const double* hi = x + ((size_t)(first ? b : a) * T) * 2;
                if (t > 0) {                                  // segment t - 1: this point is its far end
                    const RprSegment sg = rpr_segment(lo + (t - 1) * 2, hi + (t - 1) * 2, m, g.tau);
                    const double w = sg.sigma * sg.u;
                    const double px = w * sg.nx, py = w * sg.ny;
                    if (first) { gx = gx - px; gy = gy - py; }
                    else { gx = gx + px; gy = gy + py; }
                    dmin = sg.d < dmin ? sg.d : dmin;
                }
                if (t < T - 1) {                              // segment t: this point is its near end
                    const RprSegment sg = rpr_segment(lo + t * 2, hi + t * 2, m, g.tau);
                    const double w = sg.sigma * (1.0 - sg.u);
                    const double px = w * sg.nx, py = w * sg.ny;
                    if (first) { gx = gx - px; gy = gy - py; }
                    else { gx = gx + px; gy = gy + py; }
                    dmin = sg.d < dmin ? sg.d : dmin;
                }
            }
            if constexpr (WALLS) {                            // behind the partners: walls ascending, the step that ends here, then the one that starts here
                const double mw = g.wall_radius + g.margin;
                const double* cur = x + (size_t)pt * 2;
                const double* prev = t > 0 ? cur - 2 : lead ? lead + a * 2 : nullptr;
                for (int l = 0; l < g.L; ++l) {
                    if (prev) {
                        const RprWallSegment sg = rpr_wall_segment(wl + l * 4, prev, cur, mw, g.tau);
                        const double w = sg.sigma * sg.w1;
                        const double px = w * sg.nx, py = w * sg.ny;
                        gx = gx - px; gy = gy - py;
                        wmin = sg.d < wmin ? sg.d : wmin;
                    }
                    if (t < T - 1) {
                        const RprWallSegment sg = rpr_wall_segment(wl + l * 4, cur, cur + 2, mw, g.tau);
                        const double w = sg.sigma * sg.w0;
                        const double px = w * sg.nx, py = w * sg.ny;
                        gx = gx - px; gy = gy - py;
                        wmin = sg.d < wmin ? sg.d : wmin;
                    }
                }
            }
            xn[pt * 2] = x[pt * 2] - g.step * gx;
            xn[pt * 2 + 1] = x[pt * 2 + 1] - g.step * gy;
        }
        dmin = rpr_block_min(dmin, red, tid);
        if constexpr (WALLS) {
            wmin = rpr_block_min(wmin, red, tid);
            if (dmin >= stop && wmin >= g.wall_radius + g.margin * 0.5) break;
        } else {
            if (dmin >= stop) break;
        }
        double* sw = x; x = xn; xn = sw;
        ++iters;
    }
    __syncthreads();
    if constexpr (WALLS) r32 = reinterpret_cast<float*>(xn);  // (the copy that does not hold the final iterate: nobody reads it again)
    for (int i = tid; i < n_in; i += RPR_THREADS) r32[i] = (float)x[i];
    __syncthreads();
    // the predicate on the rounded sample, with its own function: every (pair, segment), a NaN kept
    const int G = T - 1, P = n * (n - 1) / 2;
    double after = INFINITY;
    for (int q = tid; q < P * G; q += RPR_THREADS) {
        const int pr = q / G, s = q - pr * G;
        int i, j;
        cls_pair_agents(pr, n, &i, &j);
        const float* pi = r32 + ((size_t)i * T + s) * 2;
        const float* pj = r32 + ((size_t)j * T + s) * 2;
        const double d = cls_segment_dist((double)pi[0] - (double)pj[0], (double)pi[1] - (double)pj[1], (double)pi[2] - (double)pj[2],
                                          (double)pi[3] - (double)pj[3]);
        after = cls_min(d, after);
    }
    __syncthreads();
    red[tid] = after;
    __syncthreads();
    for (int o = RPR_THREADS / 2; o > 0; o >>= 1) {
        if (tid < o) red[tid] = cls_min(red[tid], red[tid + o]);
        __syncthreads();
    }
    after = red[0];
    bool ok = after == after && !(after < g.threshold);
    double wafter = INFINITY;
    if constexpr (WALLS) {       // the wall predicate on the rounded sample, with its own function: every (agent, wall), the steps in order
        const int L = g.L;
        for (int q = tid; q < n * L; q += RPR_THREADS) {
            const int a = q / L, l = q - a * L;
            const double* w = wl + l * 4;
            const float* pa = r32 + (size_t)a * T * 2;
            double mn = lead ? wls_segment_dist(w[0], w[1], w[2], w[3], lead[a * 2], lead[a * 2 + 1], (double)pa[0], (double)pa[1]) : INFINITY;
            for (int s = 0; s < T - 1; ++s)
                mn = cls_min(mn, wls_segment_dist(w[0], w[1], w[2], w[3], (double)pa[2 * s], (double)pa[2 * s + 1], (double)pa[2 * s + 2],
                                                  (double)pa[2 * s + 3]));
            wafter = cls_min(mn, wafter);
        }
        __syncthreads();
        red[tid] = wafter;
        __syncthreads();
        for (int o = RPR_THREADS / 2; o > 0; o >>= 1) {
            if (tid < o) red[tid] = cls_min(red[tid], red[tid + o]);
            __syncthreads();
        }
        wafter = red[0];
        ok = ok && wafter == wafter && !(wafter - g.wall_radius < 0.0);
    }
    if (ok) {
        if (dst)
            for (int i = tid; i < n_in; i += RPR_THREADS) dst[i] = r32[i];
        if (g.p0 && (g.vel || g.vel2)) {
            const float* p0 = g.p0 + e * (size_t)AA * 2;
            for (int i = tid; i < n_in; i += RPR_THREADS) {
                const int pt = i >> 1, c = i & 1, a = pt / T, t = pt - a * T;
                const double prev = t > 0 ? (double)r32[i - 2] : (double)p0[a * 2 + c];
                const float v = (float)(((double)r32[i] - prev) / g.dt);
                if (g.vel) g.vel[blk * (size_t)n_all + i] = v;
                if (g.vel2) g.vel2[blk * (size_t)n_all + i] = v;
            }
        }
    }
    if (tid == 0) {
        so[0] = (float)before; so[1] = ok ? (float)after : (float)before; so[2] = (float)iters;
        so[3] = ok ? (float)RPR_REPAIRED : (float)RPR_REVERTED;
        if constexpr (WALLS)
            if (g.wall_out) {
                g.wall_out[blk * RPR_WALL_COLS] = (float)wbefore;
                g.wall_out[blk * RPR_WALL_COLS + 1] = ok ? (float)wafter : (float)wbefore;
            }
    }
}

// one workgroup per episode: episode[e, :] from sample[e, :, :]
static __global__ __launch_bounds__(RPR_THREADS) void repair_episode_kernel(RepairArgs g) {
    __shared__ int sh[3][RPR_THREADS];
    const int tid = threadIdx.x, e = blockIdx.x, K = g.K;
    int tried = 0, fixed = 0, most = 0;
    for (int s = tid; s < K; s += RPR_THREADS) {
        const float* so = g.sample + ((size_t)e * K + s) * RPR_SAMPLE_COLS;
        const int state = (int)so[3], it = (int)so[2];
        tried += state == RPR_REPAIRED || state == RPR_REVERTED ? 1 : 0;
        fixed += state == RPR_REPAIRED ? 1 : 0;
        most = it > most ? it : most;
    }
    sh[0][tid] = tried; sh[1][tid] = fixed; sh[2][tid] = most;
    __syncthreads();
    for (int o = RPR_THREADS / 2; o > 0; o >>= 1) {
        if (tid < o) {
            sh[0][tid] += sh[0][tid + o];
            sh[1][tid] += sh[1][tid + o];
            sh[2][tid] = sh[2][tid + o] > sh[2][tid] ? sh[2][tid + o] : sh[2][tid];
        }
        __syncthreads();
    }
    if (tid == 0) {
        g.episode[e * RPR_EPISODE_COLS] = sh[0][0];
        g.episode[e * RPR_EPISODE_COLS + 1] = sh[1][0];
        g.episode[e * RPR_EPISODE_COLS + 2] = sh[2][0];
    }
}

inline hipError_t launch_repair(const RepairArgs& g, hipStream_t st) {
    hipLaunchKernelGGL(repair_sample_kernel<false>, dim3((unsigned)(g.E * g.K)), dim3(RPR_THREADS), repair_lds(g.A, g.T), st, g);
    if (g.episode) hipLaunchKernelGGL(repair_episode_kernel, dim3(g.E), dim3(RPR_THREADS), 0, st, g);
    return hipGetLastError();
}

// wall_out of a call without walls: min_clear is +inf before and after (what jmid_wall_statistics gives at L = 0)
static __global__ void repair_wall_fill_kernel(float* wall_out, size_t count) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) wall_out[i] = INFINITY;
}

// L = 0: the launches of launch_repair and nothing else of the kernel with walls (g.wws may then be null)
inline hipError_t launch_repair_walls(const RepairWallArgs& g, hipStream_t st) {
    if (g.L == 0) {
        const size_t count = (size_t)g.E * g.K * RPR_WALL_COLS;
        if (g.wall_out) hipLaunchKernelGGL(repair_wall_fill_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, st, g.wall_out, count);
        return launch_repair(g, st);
    }
    hipLaunchKernelGGL(repair_sample_kernel<true>, dim3((unsigned)(g.E * g.K)), dim3(RPR_THREADS), repair_walls_lds(g.A, g.T, g.L), st, g);
    if (g.episode) hipLaunchKernelGGL(repair_episode_kernel, dim3(g.E), dim3(RPR_THREADS), 0, st, static_cast<const RepairArgs&>(g));
    return hipGetLastError();
}

}  // namespace jmid
