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

}  // namespace jmid
