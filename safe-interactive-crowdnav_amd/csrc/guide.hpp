// Guided sampling: the device half of jmid_guide_step / jmid_denoise_guided (include/jmid_hip.h states the rule).
//
// The repair (repair.hpp) moves a FINISHED sample, so the net never sees the correction.  Guidance runs between the denoise steps: after
// the sampler update of a step-table entry the loop's velocity state x [E, K*A, T, 2] is integrated to positions in fp64, pushed apart by at
// most n_inner Jacobi steps of the repair's own iteration (step := the entry's weight in metres), and the displacement goes back into x as
// velocity differences - the remaining steps of the net run on the corrected state.  There is no "End" stage: nothing is rounded, judged or
// reverted, and a sample that needs no iteration is not written at all.
//
// One workgroup per (episode, sample) of a chunk.  The sample's n x T points lie in LDS as fp64, twice (the Jacobi step reads one copy and
// writes the other), the reduction row behind them and, with walls, the walls [L, 4] and the episode's p0 rows - the footprint of
// repair_walls_lds: 53.0 KB at A = 64, T = 24, L = 64.  The iteration is repair_sample_kernel's, thread ownership and summation order
// included (points tid, tid + 256, ...; partners ascending, segment t - 1 before t; then the walls ascending), through the same device
// functions rpr_segment, rpr_wall_segment and rpr_block_min.  The integration and the write-back are one thread per (agent, coordinate),
// ascending t: q_initial is recomputed from x for the write-back, not kept.  No atomics: a row of guide_out belongs to one workgroup, and
// the launches of one call follow each other on one stream.
#pragma once
#include "repair.hpp"

namespace jmid {

constexpr int GDE_COLS = 2;            // steps at which the sample iterated, iterations in total
constexpr int GDE_MAX_INNER = 64;

struct GuideArgs {
    float* x;                     // [E, K*A, T, 2] the velocity state, in place: row (e*K + s)*A + a
    const float* p0;              // [E, A, 2]
    const int* n_agents;          // [E] on the device (a padded batch), or null: A everywhere
    const double* walls;          // [L, 4] {x1, y1, x2, y2} on the device (WALLS only)
    float* out;                   // [E, K, 2] accumulated over the launches of a call, or null
    double threshold, margin, tau, weight, dt, wall_radius;
    int E, A, K, T, n_inner, L;
};

inline size_t guide_lds(int A, int T, int L) { return repair_walls_lds(A, T, L); }

template <bool WALLS>
static __global__ __launch_bounds__(RPR_THREADS) void guide_sample_kernel(GuideArgs g) {
    extern __shared__ __attribute__((aligned(16))) unsigned char gde_lds_raw[];
    const int tid = threadIdx.x;
    const size_t blk = blockIdx.x;
    const int AA = g.A, T = g.T;                              // AA: the row stride; n: the real agents of this episode
    const size_t e = blk / (size_t)g.K;
    const int n = g.n_agents ? g.n_agents[e] : AA;
    const int n_pt = n * T;
    float* xs = g.x + blk * (size_t)AA * T * 2;
    const float* p0 = g.p0 + e * (size_t)AA * 2;
    double* x = reinterpret_cast<double*>(gde_lds_raw);       // [n, T, 2] the iterate
    double* xn = x + (size_t)AA * T * 2;                      // [n, T, 2] the next one
    double* red = xn + (size_t)AA * T * 2;                    // [RPR_THREADS]
    // ---- 1. integrate: one thread per (agent, coordinate), ascending t; a point that is not finite leaves the sample untouched
    double bad = 0.0;
    for (int i = tid; i < n * 2; i += RPR_THREADS) {
        const int a = i >> 1, c = i & 1;
        const double lead = (double)p0[i];
        double acc = 0.0;
        for (int t = 0; t < T; ++t) {
            acc = acc + (double)xs[((size_t)a * T + t) * 2 + c];
            const double q = lead + g.dt * acc;
            x[((size_t)a * T + t) * 2 + c] = q;
            if (!(fabs(q) <= 1.7976931348623157e308)) bad = -1.0;
        }
    }
    const double* wl = nullptr;
    const double* lead = nullptr;
    if constexpr (WALLS) {
        double* wls = red + RPR_THREADS;
        double* p0s = wls + (size_t)g.L * 4;
        for (int i = tid; i < g.L * 4; i += RPR_THREADS) wls[i] = g.walls[i];
        for (int i = tid; i < n * 2; i += RPR_THREADS) p0s[i] = (double)p0[i];
        wl = wls;
        lead = p0s;
    }
    if (rpr_block_min(bad, red, tid) < 0.0) return;           // (uniform over the workgroup)
    // ---- 2. iterate: the Iteration of jmid_repair_collisions(_walls) with step := weight, at most n_inner times
    const double m = g.threshold + g.margin, stop = g.threshold + g.margin * 0.5;
    int iters = 0;
    for (int it = 0; it < g.n_inner; ++it) {                  // (uniform trip count: the exit below is block-wide)
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
                const double* prev = t > 0 ? cur - 2 : lead + a * 2;
                for (int l = 0; l < g.L; ++l) {
                    {
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
            xn[pt * 2] = x[pt * 2] - g.weight * gx;
            xn[pt * 2 + 1] = x[pt * 2 + 1] - g.weight * gy;
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
    if (iters == 0) return;                                   // (uniform) not written at all
    // ---- 3. write back: D = q_final - q_initial (recomputed from x, the same sums), x += (D[t] - D[t-1]) / dt, one rounding per point
    for (int i = tid; i < n * 2; i += RPR_THREADS) {
        const int a = i >> 1, c = i & 1;
        const double ld = (double)p0[i];
        double acc = 0.0, dprev = 0.0;
        for (int t = 0; t < T; ++t) {
            const size_t k = ((size_t)a * T + t) * 2 + c;
            const double v = (double)xs[k];
            acc = acc + v;
            const double q0 = ld + g.dt * acc;
            const double d = x[k] - q0;
            xs[k] = (float)(v + (d - dprev) / g.dt);
            dprev = d;
        }
    }
    if (tid == 0 && g.out) {
        float* o = g.out + blk * GDE_COLS;
        o[0] = o[0] + 1.0f;
        o[1] = o[1] + (float)iters;
    }
}

// weight > 0 (the caller launches nothing otherwise).  L = 0: the instance without walls
inline hipError_t launch_guide(const GuideArgs& g, hipStream_t st) {
    const size_t lds = guide_lds(g.A, g.T, g.L);
    if (g.L > 0) hipLaunchKernelGGL(guide_sample_kernel<true>, dim3((unsigned)(g.E * g.K)), dim3(RPR_THREADS), lds, st, g);
    else hipLaunchKernelGGL(guide_sample_kernel<false>, dim3((unsigned)(g.E * g.K)), dim3(RPR_THREADS), lds, st, g);
    return hipGetLastError();
}

}  // namespace jmid
