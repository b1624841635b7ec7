// The evaluation statistics of the reference's test loop for a batch of episodes, computed where the samples already are.
//
// Reference: compute_batch_statistics (MID/evaluation/evaluation.py:456-739, the branch without is_eval_hst), per (scene, agent):
//     d[s, t] = || pos[s, t] - gt[t] || ;  ade[s] = mean_t d[s, t] ;  fde[s] = d[s, T - 1]                (compute_ade / compute_fde, :11-36)
//     min, mean, np.std of ade and fde over the K samples                                                  (:590-602)
//     KDE-NLL (compute_kde_nll, :191-232): per horizon step a 2-D scipy.stats.gaussian_kde of the K sampled points with its
//         defaults - C = cov(points, divisor K - 1) * K^(-2/6) (Scott's factor n^(-1/(d+4)), d = 2, squared),
//         logpdf(x) = logsumexp_s(-1/2 (x - p_s)^T C^-1 (x - p_s)) - ln K - 1/2 ln det(2 pi C) - evaluated at the ground truth,
//         clipped below at -20, averaged over the steps, negated
//     the most likely sample (get_most_likely_trajectory_idx -> _calc_kde_nll_for_each_traj, :259-285, 445-453): the same KDEs
//         evaluated at their own K points, the sample with the highest step-mean clipped log-pdf (the first one on an exact tie),
//         and its ade / fde                                                                                (:573-582)
// and per scene (:717-737): sade[s] = mean_a ade[s, a], sfde[s] = mean_a fde[s, a]; min, mean, np.std over the samples.
// scipy factors the covariance of the DATA (Cholesky, lower) and raises LinAlgError when a pivot is not positive; compute_kde_nll
// turns that into nan (:229-230).  Here a step whose factorisation fails makes the row's kde_nll NaN, its ml_idx -1 and its
// ade_ml / fde_ml NaN (the reference's get_most_likely_trajectory_idx lets the exception escape); the other columns are unaffected.
//
// fp64 on the fp32 inputs, like kde.hpp: the work is tiny (per step a 2 x 2 covariance and K (K + 1) exponentials) and the fp32
// outputs are then the roundings of the reference's float64 values.  One workgroup per (episode, agent), the K points of the
// current step in LDS; one workgroup per episode for the scene block.  Every sum runs in an order fixed by (K, A, T) alone - per
// thread in index order, then a binary tree over the threads - and there are no atomics: a row does not depend on the batch it is in.
#pragma once
#include "common.hpp"

namespace jmid {

constexpr int EVS_THREADS = 256;
constexpr int EVS_AGENT_COLS = 10;    // ade_min, ade_mean, ade_std, ade_ml, fde_min, fde_mean, fde_std, fde_ml, kde_nll, ml_idx
constexpr int EVS_SCENE_COLS = 6;     // sade_min, sade_mean, sade_std, sfde_min, sfde_mean, sfde_std
constexpr double EVS_LOG_PDF_FLOOR = -20.0;      // log_pdf_lower_bound (:203, :271)

struct EvalStatsArgs {
    const float* pos;     // [E, K, A, T, 2] (jmid_denoise's pos_out layout)
    const float* gt;      // [E, A, T, 2]
    float* agent_out;     // [E, A, 10]
    float* scene_out;     // [E, 6] or null
    int E, A, K, T;
};

inline size_t eval_stats_agent_lds(int K) { return sizeof(double) * ((size_t)5 * K + 1 + EVS_THREADS) + sizeof(int) * EVS_THREADS; }
inline size_t eval_stats_scene_lds(int K) { return sizeof(double) * ((size_t)2 * K + EVS_THREADS); }

// sum of one value per thread: a binary tree over the thread index (red [EVS_THREADS]); every thread gets the result
__device__ __forceinline__ double evs_block_sum(double v, double* red, int tid) {
    __syncthreads();
    red[tid] = v;
    __syncthreads();
    for (int o = EVS_THREADS / 2; o > 0; o >>= 1) {
        if (tid < o) red[tid] += red[tid + o];
        __syncthreads();
    }
    return red[0];
}
__device__ __forceinline__ double evs_block_min(double v, double* red, int tid) {
    __syncthreads();
    red[tid] = v;
    __syncthreads();
    for (int o = EVS_THREADS / 2; o > 0; o >>= 1) {
        if (tid < o) red[tid] = fmin(red[tid], red[tid + o]);
        __syncthreads();
    }
    return red[0];
}
// {min, mean, population std} of v[0 .. K) (np.min, np.mean, np.std: sqrt(mean((v - mean)^2)))
__device__ __forceinline__ void evs_min_mean_std(const double* v, int K, double* red, int tid, double* out3) {
    // the mean as v[0] + mean(v - v[0]): the sum of small differences loses nothing to the common magnitude of the values, and K equal
    // values (the samples of a degenerate agent) have exactly their value as mean and exactly 0 as deviation, as in the reference
    const double shift = v[0];
    double mn = INFINITY, sm = 0.0;
    for (int s = tid; s < K; s += EVS_THREADS) {
        mn = fmin(mn, v[s]);
        sm += v[s] - shift;
    }
    mn = evs_block_min(mn, red, tid);
    const double mean = shift + evs_block_sum(sm, red, tid) / (double)K;
    double sq = 0.0;
    for (int s = tid; s < K; s += EVS_THREADS) {
        const double c = v[s] - mean;
        sq += c * c;
    }
    const double var = evs_block_sum(sq, red, tid) / (double)K;
    out3[0] = mn; out3[1] = mean; out3[2] = sqrt(var);
}

// one workgroup per (episode, agent): agent_out[e, a, :]
static __global__ __launch_bounds__(EVS_THREADS) void eval_stats_agent_kernel(EvalStatsArgs g) {
    extern __shared__ __attribute__((aligned(16))) unsigned char evs_lds_raw[];
    const int tid = threadIdx.x, blk = blockIdx.x;
    const int e = blk / g.A, a = blk - e * g.A;
    const int A = g.A, K = g.K, T = g.T;
    double* px = reinterpret_cast<double*>(evs_lds_raw);      // [K] the points of the current step
    double* py = px + K;                                      // [K]
    double* ade = py + K;                                     // [K] sum_t d[s, t], then the mean
    double* fde = ade + K;                                    // [K]
    double* sll = fde + K;                                    // [K + 1] sum_t of the clipped log-pdf at sample s; [K]: at the ground truth
    double* red = sll + K + 1;                                // [EVS_THREADS]
    int* redi = reinterpret_cast<int*>(red + EVS_THREADS);    // [EVS_THREADS]
    const float* pe = g.pos + ((size_t)e * K * A + a) * T * 2;          // sample s: + s * A * T * 2
    const float* ge = g.gt + ((size_t)e * A + a) * T * 2;
    for (int i = tid; i <= K; i += EVS_THREADS) {
        sll[i] = 0.0;
        if (i < K) ade[i] = 0.0;
    }
    bool bad = false;         // the Cholesky factorisation of some step's covariance failed (uniform over the workgroup)
    const double scott = pow((double)K, -1.0 / 6.0);          // gaussian_kde.scotts_factor: n^(-1 / (d + 4)), d = 2
    for (int t = 0; t < T; ++t) {
        const double gx = (double)ge[2 * t], gy = (double)ge[2 * t + 1];
        __syncthreads();                                      // (the previous step's readers of px / py are done)
        double sx = 0.0, sy = 0.0;
        for (int s = tid; s < K; s += EVS_THREADS) {
            const float* p = pe + ((size_t)s * A * T + t) * 2;
            const double x = (double)p[0], y = (double)p[1];
            px[s] = x; py[s] = y;
            const double dx = x - gx, dy = y - gy;
            const double d = sqrt(dx * dx + dy * dy);
            ade[s] += d;
            fde[s] = d;                                       // (the last step's value stays)
            sx += x; sy += y;
        }
        const double mx = evs_block_sum(sx, red, tid) / (double)K;
        const double my = evs_block_sum(sy, red, tid) / (double)K;
        double cxx = 0.0, cxy = 0.0, cyy = 0.0;
        for (int s = tid; s < K; s += EVS_THREADS) {
            const double ux = px[s] - mx, uy = py[s] - my;
            cxx += ux * ux; cxy += ux * uy; cyy += uy * uy;
        }
        cxx = evs_block_sum(cxx, red, tid) / (double)(K - 1);
        cxy = evs_block_sum(cxy, red, tid) / (double)(K - 1);
        cyy = evs_block_sum(cyy, red, tid) / (double)(K - 1);
        // lower Cholesky factor of the data covariance, as LAPACK's potrf takes it: a pivot that is not positive (or NaN) fails
        if (!(cxx > 0.0)) { bad = true; continue; }
        const double l11d = sqrt(cxx), l21d = cxy / l11d, piv = cyy - l21d * l21d;
        if (!(piv > 0.0)) { bad = true; continue; }
        const double l11 = l11d * scott, l21 = l21d * scott, l22 = sqrt(piv) * scott;     // factor of C = cov * scott^2
        const double lognorm = log((double)K) + log(2.0 * 3.14159265358979323846) + log(l11 * l22);      // ln K + 1/2 ln det(2 pi C)
        // log-pdf at the K samples and at the ground truth (i = K): one thread per evaluation point, the K terms in sample order
        const double i11 = 1.0 / l11, i22 = 1.0 / l22;
        for (int i = tid; i <= K; i += EVS_THREADS) {
            const double x = i < K ? px[i] : gx, y = i < K ? py[i] : gy;
            double m = 0.0;                                   // a sample's largest exponent is its own, 0: no shift needed
            if (i == K) {                                     // the ground truth may be far from every sample
                m = -INFINITY;
                for (int s = 0; s < K; ++s) {
                    const double y0 = (x - px[s]) * i11, y1 = ((y - py[s]) - l21 * y0) * i22;
                    m = fmax(m, -0.5 * (y0 * y0 + y1 * y1));
                }
            }
            double acc = 0.0;
            for (int s = 0; s < K; ++s) {
                const double y0 = (x - px[s]) * i11, y1 = ((y - py[s]) - l21 * y0) * i22;
                acc += exp(-0.5 * (y0 * y0 + y1 * y1) - m);
            }
            const double lp = m == -INFINITY ? m : m + log(acc) - lognorm;      // (every exponent overflowed: the pdf is 0)
            sll[i] += fmax(lp, EVS_LOG_PDF_FLOOR);            // a NaN log-pdf (non-finite inputs) stays NaN: np.clip keeps it too
        }
    }
    __syncthreads();
    for (int s = tid; s < K; s += EVS_THREADS) ade[s] /= (double)T;
    __syncthreads();
    double st_a[3], st_f[3];
    evs_min_mean_std(ade, K, red, tid, st_a);
    evs_min_mean_std(fde, K, red, tid, st_f);
    // argmax_s of the step-mean log-pdf at the own samples, the lowest index on an exact tie (min(dict, key = nll) keeps the first);
    // a NaN never wins
    double bv = -INFINITY;
    int bi = K;
    for (int s = tid; s < K; s += EVS_THREADS) {
        const double v = sll[s] / (double)T;
        if (v > bv) { bv = v; bi = s; }
    }
    __syncthreads();
    red[tid] = bv; redi[tid] = bi;
    __syncthreads();
    for (int o = EVS_THREADS / 2; o > 0; o >>= 1) {
        if (tid < o) {
            const double v = red[tid + o];
            const int j = redi[tid + o];
            if (v > red[tid] || (v == red[tid] && j < redi[tid])) { red[tid] = v; redi[tid] = j; }
        }
        __syncthreads();
    }
    if (tid == 0) {
        const int ml = redi[0];
        const bool has_ml = !bad && ml < K;
        const double nan = __builtin_nan("");
        float* o = g.agent_out + (size_t)blk * EVS_AGENT_COLS;
        o[0] = (float)st_a[0]; o[1] = (float)st_a[1]; o[2] = (float)st_a[2];
        o[3] = (float)(has_ml ? ade[ml] : nan);
        o[4] = (float)st_f[0]; o[5] = (float)st_f[1]; o[6] = (float)st_f[2];
        o[7] = (float)(has_ml ? fde[ml] : nan);
        o[8] = (float)(bad ? nan : -(sll[K] / (double)T));
        o[9] = has_ml ? (float)ml : -1.0f;
    }
}

// one workgroup per episode: scene_out[e, :]
static __global__ __launch_bounds__(EVS_THREADS) void eval_stats_scene_kernel(EvalStatsArgs g) {
    extern __shared__ __attribute__((aligned(16))) unsigned char evs_lds_raw[];
    const int tid = threadIdx.x, e = blockIdx.x;
    const int A = g.A, K = g.K, T = g.T;
    double* sade = reinterpret_cast<double*>(evs_lds_raw);    // [K]
    double* sfde = sade + K;                                  // [K]
    double* red = sfde + K;                                   // [EVS_THREADS]
    for (int s = tid; s < K; s += EVS_THREADS) {
        double sa = 0.0, sf = 0.0;                            // sade = ade_0 + ade_1 + ... in agent order (:717-725)
        for (int a = 0; a < A; ++a) {
            const float* p = g.pos + (((size_t)e * K + s) * A + a) * T * 2;
            const float* q = g.gt + ((size_t)e * A + a) * T * 2;
            double acc = 0.0, last = 0.0;
            for (int t = 0; t < T; ++t) {
                const double dx = (double)p[2 * t] - (double)q[2 * t], dy = (double)p[2 * t + 1] - (double)q[2 * t + 1];
                last = sqrt(dx * dx + dy * dy);
                acc += last;
            }
            sa += acc / (double)T;
            sf += last;
        }
        sade[s] = sa / (double)A;
        sfde[s] = sf / (double)A;
    }
    __syncthreads();
    double st_a[3], st_f[3];
    evs_min_mean_std(sade, K, red, tid, st_a);
    evs_min_mean_std(sfde, K, red, tid, st_f);
    if (tid == 0) {
        float* o = g.scene_out + (size_t)e * EVS_SCENE_COLS;
        o[0] = (float)st_a[0]; o[1] = (float)st_a[1]; o[2] = (float)st_a[2];
        o[3] = (float)st_f[0]; o[4] = (float)st_f[1]; o[5] = (float)st_f[2];
    }
}

inline hipError_t launch_eval_stats(const EvalStatsArgs& g, hipStream_t st) {
    hipLaunchKernelGGL(eval_stats_agent_kernel, dim3(g.E * g.A), dim3(EVS_THREADS), eval_stats_agent_lds(g.K), st, g);
    if (g.scene_out) hipLaunchKernelGGL(eval_stats_scene_kernel, dim3(g.E), dim3(EVS_THREADS), eval_stats_scene_lds(g.K), st, g);
    return hipGetLastError();
}

// ================================================================================================ the masked form (is_eval_hst)
// Reference: the is_eval_hst branch of compute_batch_statistics (:540-545, :556-558, :566-568, :573-577, :624-715).  Per agent a
// boolean interpolated_future [T] (1 = the ground truth of that step is interpolated or absent: not scored):
//     ade[s] = the mean of d[s, t] over the scored steps; fde[s] = d[s, T - 1], absent (array([None])) when the last step is not scored
//     KDE-NLL and the most likely sample: as above over the scored steps only (np.compress, :212-214, :262-266); one step is enough
//     an agent without a scored step, or whose history is all interpolated (skip), is left out of everything (:544-545)
//     per cut-off step c (the reference hard-codes 2, 5, 8 for T = 12; all columns absent when step c is not scored):
//         ade at c = d[s, c]: its min and mean over the samples and its value at the most likely sample of the full masked horizon
//         kde at c: compute_kde_nll(cutoff_idx = c) slices the ground truth to shape [2] and then loops "time steps" over its two
//         entries (:209-222) - what it returns is the mean of two 1-D gaussian_kde negative log-pdfs, each floored at -20: one of the
//         K x-coordinates at the ground truth's x, one of the y-coordinates at its y (scipy's 1-D defaults: variance with divisor
//         K - 1, Scott's factor K^(-1/5)), NOT a 2-D single-step density.  Reproduced as it is.
// The scene block (:717-737) averages over the agents that were kept.  Where the reference raises instead of computing (TypeError
// when a kept agent has no fde, IndexError when no agent is kept) this project's conventions apply: sfde runs over the kept agents
// with a scored last step, and columns without any qualifying agent are NaN.
// A failed factorisation follows the rule above: 2-D (any scored step) -> kde_nll NaN, ml_idx -1 and every *_ml column NaN; 1-D (x or
// y of a cut-off step has no variance) -> that cut-off's kde NaN.  The two flag columns and the cut-offs' valid column tell "absent"
// from "NaN because scipy would have raised".
// Separate kernels: the unmasked pair above stays instruction for instruction what it was.  With nothing masked the first ten agent
// columns and the scene row come out of the same operations in the same order as there.
constexpr int EVS_MASKED_AGENT_COLS = 12;    // the ten above, n_valid (scored steps; 0 = the agent is left out), fde_valid (0 / 1)
constexpr int EVS_CUT_COLS = 5;              // ade_min, ade_mean, ade_ml, kde, valid
constexpr int EVS_MAX_CUTS = 4;

struct EvalStatsMaskedArgs {
    const float* pos;               // [E, K, A, T, 2]
    const float* gt;                // [E, A, T, 2]
    const unsigned char* interp;    // [E, A, T] 1 = not scored
    const unsigned char* skip;      // [E, A] 1 = agent left out, or null
    float* agent_out;               // [E, A, 12]
    float* cut_out;                 // [E, A, n_cut, 5] (null when n_cut = 0)
    float* scene_out;               // [E, 6] or null
    int E, A, K, T, n_cut;
    int cutoffs[EVS_MAX_CUTS];      // each in [0, T)
};

inline size_t eval_stats_masked_agent_lds(int K) { return sizeof(double) * ((size_t)5 * K + 5 + EVS_THREADS) + sizeof(int) * EVS_THREADS; }

// one workgroup per (episode, agent): agent_out[e, a, :], cut_out[e, a, :, :]
static __global__ __launch_bounds__(EVS_THREADS) void eval_stats_masked_agent_kernel(EvalStatsMaskedArgs g) {
    extern __shared__ __attribute__((aligned(16))) unsigned char evs_lds_raw[];
    const int tid = threadIdx.x, blk = blockIdx.x;
    const int e = blk / g.A, a = blk - e * g.A;
    const int A = g.A, K = g.K, T = g.T;
    double* px = reinterpret_cast<double*>(evs_lds_raw);      // [K] the points of the current step
    double* py = px + K;                                      // [K]
    double* ade = py + K;                                     // [K] sum over the scored steps of d[s, t], then the mean
    double* dist = ade + K;                                   // [K] d[s, t] of the current step; after the loop: of the last scored step
    double* sll = dist + K;                                   // [K + 1] sum_t of the clipped log-pdf at sample s; [K]: at the ground truth
    double* lp1 = sll + K + 1;                                // [2] a cut-off step's clipped 1-D log-pdfs (x, y) at the ground truth
    double* red = lp1 + 4;                                    // [EVS_THREADS]
    int* redi = reinterpret_cast<int*>(red + EVS_THREADS);    // [EVS_THREADS]
    const float* pe = g.pos + ((size_t)e * K * A + a) * T * 2;          // sample s: + s * A * T * 2
    const float* ge = g.gt + ((size_t)e * A + a) * T * 2;
    const unsigned char* me = g.interp + ((size_t)e * A + a) * T;
    float* o = g.agent_out + (size_t)blk * EVS_MASKED_AGENT_COLS;
    float* oc = g.n_cut ? g.cut_out + (size_t)blk * g.n_cut * EVS_CUT_COLS : nullptr;
    const double nan = __builtin_nan("");
    int n_valid = 0;
    for (int t = 0; t < T; ++t) n_valid += me[t] ? 0 : 1;
    if (g.skip && g.skip[blk]) n_valid = 0;
    // rows of absent things first: the whole agent, or the cut-offs at steps that are not scored (everything here is uniform)
    if (tid == 0) {
        for (int j = 0; j < g.n_cut; ++j) {
            if (n_valid && !me[g.cutoffs[j]]) continue;
            for (int c = 0; c < 4; ++c) oc[j * EVS_CUT_COLS + c] = (float)nan;
            oc[j * EVS_CUT_COLS + 4] = 0.0f;
        }
        if (!n_valid) {
            for (int c = 0; c < 9; ++c) o[c] = (float)nan;
            o[9] = -1.0f; o[10] = 0.0f; o[11] = 0.0f;
        }
    }
    if (!n_valid) return;
    for (int i = tid; i <= K; i += EVS_THREADS) {
        sll[i] = 0.0;
        if (i < K) ade[i] = 0.0;
    }
    bool bad = false;         // the Cholesky factorisation of some scored step's covariance failed (uniform over the workgroup)
    const double scott = pow((double)K, -1.0 / 6.0);          // gaussian_kde.scotts_factor: n^(-1 / (d + 4)), d = 2
    const double scott1 = pow((double)K, -1.0 / 5.0);         // d = 1
    for (int t = 0; t < T; ++t) {
        if (me[t]) continue;
        bool is_cut = false;
        for (int j = 0; j < g.n_cut; ++j) is_cut = is_cut || g.cutoffs[j] == t;
        const double gx = (double)ge[2 * t], gy = (double)ge[2 * t + 1];
        __syncthreads();                                      // (the previous step's readers of px / py / dist are done)
        double sx = 0.0, sy = 0.0;
        for (int s = tid; s < K; s += EVS_THREADS) {
            const float* p = pe + ((size_t)s * A * T + t) * 2;
            const double x = (double)p[0], y = (double)p[1];
            px[s] = x; py[s] = y;
            const double dx = x - gx, dy = y - gy;
            const double d = sqrt(dx * dx + dy * dy);
            ade[s] += d;
            dist[s] = d;
            sx += x; sy += y;
        }
        const double mx = evs_block_sum(sx, red, tid) / (double)K;
        const double my = evs_block_sum(sy, red, tid) / (double)K;
        double cxx = 0.0, cxy = 0.0, cyy = 0.0;
        for (int s = tid; s < K; s += EVS_THREADS) {
            const double ux = px[s] - mx, uy = py[s] - my;
            cxx += ux * ux; cxy += ux * uy; cyy += uy * uy;
        }
        cxx = evs_block_sum(cxx, red, tid) / (double)(K - 1);
        cxy = evs_block_sum(cxy, red, tid) / (double)(K - 1);
        cyy = evs_block_sum(cyy, red, tid) / (double)(K - 1);
        double st_c[3] = {0.0, 0.0, 0.0};
        if (is_cut) evs_min_mean_std(dist, K, red, tid, st_c);          // min and mean of d[s, c] (:634-646)
        // lower Cholesky factor of the data covariance, as LAPACK's potrf takes it: a pivot that is not positive (or NaN) fails
        bool ok2 = cxx > 0.0;
        double l11 = 1.0, l21 = 0.0, l22 = 1.0;
        if (ok2) {
            const double l11d = sqrt(cxx), l21d = cxy / l11d, piv = cyy - l21d * l21d;
            ok2 = piv > 0.0;
            if (ok2) { l11 = l11d * scott; l21 = l21d * scott; l22 = sqrt(piv) * scott; }       // factor of C = cov * scott^2
        }
        if (!ok2) bad = true;
        const double lognorm = log((double)K) + log(2.0 * 3.14159265358979323846) + log(l11 * l22);      // ln K + 1/2 ln det(2 pi C)
        const double i11 = 1.0 / l11, i22 = 1.0 / l22;
        // log-pdf at the K samples and at the ground truth (i = K): one thread per evaluation point, the K terms in sample order;
        // on a cut-off step two more points: the 1-D densities of the x (i = K + 1) and y (i = K + 2) coordinates at the ground truth
        for (int i = tid; i < K + (is_cut ? 3 : 1); i += EVS_THREADS) {
            if (i <= K) {
                if (!ok2) continue;
                const double x = i < K ? px[i] : gx, y = i < K ? py[i] : gy;
                double m = 0.0;                               // a sample's largest exponent is its own, 0: no shift needed
                if (i == K) {                                 // the ground truth may be far from every sample
                    m = -INFINITY;
                    for (int s = 0; s < K; ++s) {
                        const double y0 = (x - px[s]) * i11, y1 = ((y - py[s]) - l21 * y0) * i22;
                        m = fmax(m, -0.5 * (y0 * y0 + y1 * y1));
                    }
                }
                double acc = 0.0;
                for (int s = 0; s < K; ++s) {
                    const double y0 = (x - px[s]) * i11, y1 = ((y - py[s]) - l21 * y0) * i22;
                    acc += exp(-0.5 * (y0 * y0 + y1 * y1) - m);
                }
                const double lp = m == -INFINITY ? m : m + log(acc) - lognorm;  // (every exponent overflowed: the pdf is 0)
                sll[i] += fmax(lp, EVS_LOG_PDF_FLOOR);        // a NaN log-pdf (non-finite inputs) stays NaN: np.clip keeps it too
            } else {
                const int dim = i - K - 1;
                const double* q = dim ? py : px;
                const double var = dim ? cyy : cxx, x = dim ? gy : gx;
                double lp = nan;
                if (var > 0.0) {                              // the 1 x 1 Cholesky factor exists
                    const double l = sqrt(var) * scott1, il = 1.0 / l;
                    double m = -INFINITY;
                    for (int s = 0; s < K; ++s) {
                        const double y0 = (x - q[s]) * il;
                        m = fmax(m, -0.5 * (y0 * y0));
                    }
                    double acc = 0.0;
                    for (int s = 0; s < K; ++s) {
                        const double y0 = (x - q[s]) * il;
                        acc += exp(-0.5 * (y0 * y0) - m);
                    }
                    lp = m == -INFINITY ? m : m + log(acc) - (log((double)K) + 0.5 * log(2.0 * 3.14159265358979323846) + log(l));
                    lp = fmax(lp, EVS_LOG_PDF_FLOOR);
                }
                lp1[dim] = lp;
            }
        }
        if (is_cut) {
            __syncthreads();
            if (tid == 0) {
                for (int j = 0; j < g.n_cut; ++j) {
                    if (g.cutoffs[j] != t) continue;
                    float* r = oc + j * EVS_CUT_COLS;
                    r[0] = (float)st_c[0]; r[1] = (float)st_c[1];
                    r[3] = (float)(-(lp1[0] / 2.0 + lp1[1] / 2.0));     // kde_ll += pdf / num_timesteps over the two "steps", negated
                    r[4] = 1.0f;
                }
            }
        }
    }
    __syncthreads();
    for (int s = tid; s < K; s += EVS_THREADS) ade[s] /= (double)n_valid;
    __syncthreads();
    const bool fde_valid = !me[T - 1];
    double st_a[3], st_f[3] = {nan, nan, nan};
    evs_min_mean_std(ade, K, red, tid, st_a);
    if (fde_valid) evs_min_mean_std(dist, K, red, tid, st_f);
    // argmax_s of the step-mean log-pdf at the own samples, the lowest index on an exact tie; a NaN never wins
    double bv = -INFINITY;
    int bi = K;
    for (int s = tid; s < K; s += EVS_THREADS) {
        const double v = sll[s] / (double)n_valid;
        if (v > bv) { bv = v; bi = s; }
    }
    __syncthreads();
    red[tid] = bv; redi[tid] = bi;
    __syncthreads();
    for (int w = EVS_THREADS / 2; w > 0; w >>= 1) {
        if (tid < w) {
            const double v = red[tid + w];
            const int j = redi[tid + w];
            if (v > red[tid] || (v == red[tid] && j < redi[tid])) { red[tid] = v; redi[tid] = j; }
        }
        __syncthreads();
    }
    if (tid == 0) {
        const int ml = redi[0];
        const bool has_ml = !bad && ml < K;
        o[0] = (float)st_a[0]; o[1] = (float)st_a[1]; o[2] = (float)st_a[2];
        o[3] = (float)(has_ml ? ade[ml] : nan);
        o[4] = (float)st_f[0]; o[5] = (float)st_f[1]; o[6] = (float)st_f[2];
        o[7] = (float)(has_ml && fde_valid ? dist[ml] : nan);
        o[8] = (float)(bad ? nan : -(sll[K] / (double)n_valid));
        o[9] = has_ml ? (float)ml : -1.0f;
        o[10] = (float)n_valid;
        o[11] = fde_valid ? 1.0f : 0.0f;
        for (int j = 0; j < g.n_cut; ++j) {                   // d[ml, c] of the scored cut-off steps (:647-653)
            const int c = g.cutoffs[j];
            if (me[c]) continue;
            double d = nan;
            if (has_ml) {
                const float* p = pe + ((size_t)ml * A * T + c) * 2;
                const double dx = (double)p[0] - (double)ge[2 * c], dy = (double)p[1] - (double)ge[2 * c + 1];
                d = sqrt(dx * dx + dy * dy);
            }
            oc[j * EVS_CUT_COLS + 2] = (float)d;
        }
    }
}

// one workgroup per episode: scene_out[e, :]
static __global__ __launch_bounds__(EVS_THREADS) void eval_stats_masked_scene_kernel(EvalStatsMaskedArgs g) {
    extern __shared__ __attribute__((aligned(16))) unsigned char evs_lds_raw[];
    const int tid = threadIdx.x, e = blockIdx.x;
    const int A = g.A, K = g.K, T = g.T;
    double* sade = reinterpret_cast<double*>(evs_lds_raw);    // [K]
    double* sfde = sade + K;                                  // [K]
    double* red = sfde + K;                                   // [EVS_THREADS]
    const unsigned char* me = g.interp + (size_t)e * A * T;
    auto scored_steps = [&](int a) {                          // 0: the agent is left out
        if (g.skip && g.skip[(size_t)e * A + a]) return 0;
        int n = 0;
        for (int t = 0; t < T; ++t) n += me[(size_t)a * T + t] ? 0 : 1;
        return n;
    };
    int n_kept = 0, n_last = 0;                               // kept agents; kept agents whose last step is scored (uniform)
    for (int a = 0; a < A; ++a) {
        if (!scored_steps(a)) continue;
        ++n_kept;
        n_last += me[(size_t)a * T + T - 1] ? 0 : 1;
    }
    for (int s = tid; s < K; s += EVS_THREADS) {
        double sa = 0.0, sf = 0.0;                            // sade = ade_0 + ade_1 + ... over the kept agents in agent order (:717-725)
        for (int a = 0; a < A; ++a) {
            const int n = scored_steps(a);
            if (!n) continue;
            const float* p = g.pos + (((size_t)e * K + s) * A + a) * T * 2;
            const float* q = g.gt + ((size_t)e * A + a) * T * 2;
            const unsigned char* m = me + (size_t)a * T;
            double acc = 0.0, last = 0.0;
            for (int t = 0; t < T; ++t) {
                if (m[t]) continue;
                const double dx = (double)p[2 * t] - (double)q[2 * t], dy = (double)p[2 * t + 1] - (double)q[2 * t + 1];
                last = sqrt(dx * dx + dy * dy);
                acc += last;
            }
            sa += acc / (double)n;
            if (!m[T - 1]) sf += last;
        }
        sade[s] = sa / (double)n_kept;
        sfde[s] = sf / (double)n_last;
    }
    __syncthreads();
    const double nan = __builtin_nan("");
    double st_a[3] = {nan, nan, nan}, st_f[3] = {nan, nan, nan};
    if (n_kept) evs_min_mean_std(sade, K, red, tid, st_a);
    if (n_last) evs_min_mean_std(sfde, K, red, tid, st_f);
    if (tid == 0) {
        float* o = g.scene_out + (size_t)e * EVS_SCENE_COLS;
        o[0] = (float)st_a[0]; o[1] = (float)st_a[1]; o[2] = (float)st_a[2];
        o[3] = (float)st_f[0]; o[4] = (float)st_f[1]; o[5] = (float)st_f[2];
    }
}

inline hipError_t launch_eval_stats_masked(const EvalStatsMaskedArgs& g, hipStream_t st) {
    hipLaunchKernelGGL(eval_stats_masked_agent_kernel, dim3(g.E * g.A), dim3(EVS_THREADS), eval_stats_masked_agent_lds(g.K), st, g);
    if (g.scene_out) hipLaunchKernelGGL(eval_stats_masked_scene_kernel, dim3(g.E), dim3(EVS_THREADS), eval_stats_scene_lds(g.K), st, g);
    return hipGetLastError();
}

}  // namespace jmid
